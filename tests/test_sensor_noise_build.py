"""Sensor noise (rmav_set_sensor_noise), what can be checked without a GPU: the three entry points are declared, exported and bound; the
new kernel families exist for the four quadrotor kinds with the members stated here, use no scratch and spill no vector register
(`make asm`); their names match no pre-existing family prefix and the older families keep their members; registers and occupancy are
what was observed (profiles/r19/sensor_noise.md has the table beside the disturbed kernels they are cut from); and no kernel evaluates
the draw more often than its body says."""
import re

import pytest

import buildinfo as B
from test_disturbance_build import DISTURB, POLICY
from test_frame_skip_build import SKIP
from test_reward_build import REWARD

NEW = {"rmav_set_sensor_noise": ("int", 2), "rmav_get_sensor_noise": ("int", 3), "rmav_observe": ("int", 4)}
# family prefix -> members (six families per kind): k_step_sn<K, TL, RW>; k_rollout_sn<K, MODE in (buffer, random, controller), TL, RW> (one store policy);
# k_observe<K>; the policy rollouts k_rollout_nrm_sn / k_rollout_pair_sn / k_rollout_pair_shared_sn<K, BOOT, RW> (rmav_sensor_policy_abi).
SENSOR = {"_ZN4rmav9k_step_snILi": 4 * 2 * 2, "_ZN4rmav12k_rollout_snILi": 4 * 3 * 2 * 2, "_ZN4rmav9k_observeILi": 4}
SENSOR_POLICY = {"_ZN4rmav16k_rollout_nrm_snILi": 4 * 2 * 2, "_ZN4rmav17k_rollout_pair_snILi": 4 * 2 * 2, "_ZN4rmav24k_rollout_pair_shared_snILi": 4 * 2 * 2}
MATRIX_CORE_BAD = ("ds_bpermute", "ds_permute", "v_pk_mul_f32", "v_pk_mov_b32")   # buildinfo.assert_matrix_core_clean's forms
SET = "_ZN4rmav18k_set_sensor_noiseEPjNS_10SensorArgsEj"   # the launch that rewrites the handle's device copy of the spec


def count(body):
    return sum(1 for ln in body.split("\n") if ln.startswith("\t") and not ln.startswith("\t."))


def sensor_family(prefix):
    h = B.hits(prefix)
    assert len(h) == {**SENSOR, **SENSOR_POLICY}[prefix], (prefix, sorted(h))
    return h


def test_sensor_entry_points_are_declared_exported_and_bound(built):
    A, _ = B.assert_entry_points(NEW)
    import ctypes as C

    S = A.SensorNoiseSpec
    assert C.sizeof(S) == 64 and S.sigma.offset == 0 and S.sigma.size == 64


@pytest.mark.parametrize("prefix", sorted({**SENSOR, **SENSOR_POLICY}))
def test_every_new_family_exists_for_every_kind_and_is_clean(prefix):
    h = sensor_family(prefix)
    for kind in range(4):
        mine = [n for n in h if n.startswith(f"{prefix}{kind}E")]
        assert len(mine) == len(h) // 4, (prefix, kind, mine)
    for n, u in h.items():
        assert B.clean(u), (n, u)
        # the spec by value; the policy kernel reads the handle's device copy - and does not take ActRuleArgs as a parameter
        assert ("PolicySensorArgs" if prefix in SENSOR_POLICY else "_10SensorArgsE") in n, n
        assert "ActRuleArgs" not in n, n


def test_no_new_name_matches_an_older_prefix():
    seen = {**B.family(*B.FAMILIES)}
    for census in (SKIP, REWARD, DISTURB, POLICY):
        for p in census:
            h = B.hits(p)
            assert len(h) == census[p], (p, sorted(h))
            seen.update(h)
    new = {}
    for p in SENSOR:
        new.update(sensor_family(p))
    assert len(new) == 68 and not set(new) & set(seen)
    assert set(B.bodies("rmav_sensor_abi")) == set(new), "the unit holds the new kernels and nothing else"
    pol = {}
    for p in SENSOR_POLICY:
        pol.update(sensor_family(p))
    assert len(pol) == 48 and not set(pol) & set(seen)
    kernels = {n for n in B.bodies("rmav_sensor_policy_abi") if "k_" in n}
    assert kernels == set(pol) | {SET}, "the policy unit holds the three new actors and the spec's copy kernel"
    # rmav_disturb_abi's listing is what it was
    assert len(B.bodies("rmav_disturb_abi")) == 69


def test_the_units_only_launch():
    for unit in ("rmav_sensor_abi", "rmav_sensor_policy_abi"):
        src = open(B.os.path.join(B.PKG, "csrc", unit + ".hip")).read()
        assert 'extern "C"' not in src, unit
        assert unit in open(B.os.path.join(B.PKG, "Makefile")).read()


# (kind, registers and occupancy of k_step_sn as observed; k_step_ds beside them: 49 / 7, 83 / 5, 47 / 7, 105 / 4)
@pytest.mark.parametrize("kind,vgpr,occ", [(0, 51, 7), (1, 86, 5), (2, 61, 7), (3, 108, 4)])
def test_single_step_kernels(kind, vgpr, occ):
    hits = B.hits(f"_ZN4rmav9k_step_snILi{kind}E")
    assert len(hits) == 4, sorted(hits)
    for n, u in hits.items():
        assert u["vgpr"] <= vgpr and u["occ"] == occ, (n, u)


# (kind, registers and occupancy of k_observe as observed)
@pytest.mark.parametrize("kind,vgpr", [(0, 30), (1, 38), (2, 30), (3, 38)])
def test_observe_kernels(kind, vgpr):
    (n, u), = B.hits(f"_ZN4rmav9k_observeILi{kind}E").items()
    assert B.clean(u) and u["vgpr"] <= vgpr and u["occ"] == 8, (n, u)


# (kind, {mode: (registers, minimum occupancy)} of k_rollout_sn as observed: +2 .. 13 over k_rollout_ds - the observation row beside
# the state while it is stored; quadrotor3d with caller actions drops from 5 to 4 waves per SIMD)
@pytest.mark.parametrize("kind,budget", [(0, {0: (90, 5), 1: (89, 5), 2: (109, 4)}), (1, {0: (133, 3), 1: (133, 3), 2: (155, 3)}),
                                         (2, {0: (101, 4), 1: (96, 5), 2: (109, 4)}), (3, {0: (165, 3), 1: (163, 3), 2: (181, 2)})])
def test_fused_noisy_kernels(kind, budget):
    for mode, (vgpr, occ) in budget.items():
        hits = B.hits(f"_ZN4rmav12k_rollout_snILi{kind}ELi{mode}E")
        assert len(hits) == 4, (kind, mode, sorted(hits))
        for n, u in hits.items():
            assert B.clean(u) and u["vgpr"] <= vgpr and u["occ"] >= occ, (n, u)


# (kind, registers of the three noisy actors as observed - all four (BOOT, RW) members within the figure - and their minimum occupancy; the
# disturbed counterparts: tests/test_disturbance_build.py, profiles/r19/sensor_noise.md)
@pytest.mark.parametrize("kind,budget", [(0, {"16k_rollout_nrm_sn": (148, 3), "17k_rollout_pair_sn": (188, 2), "24k_rollout_pair_shared_sn": (156, 3)}),
                                         (1, {"16k_rollout_nrm_sn": (170, 2), "17k_rollout_pair_sn": (213, 2), "24k_rollout_pair_shared_sn": (178, 2)}),
                                         (2, {"16k_rollout_nrm_sn": (158, 2), "17k_rollout_pair_sn": (200, 2), "24k_rollout_pair_shared_sn": (168, 3)}),
                                         (3, {"16k_rollout_nrm_sn": (200, 2), "17k_rollout_pair_sn": (231, 2), "24k_rollout_pair_shared_sn": (196, 2)})])
def test_noisy_policy_kernels(kind, budget):
    for fam, (vgpr, occ) in budget.items():
        hits = B.hits(f"_ZN4rmav{fam}ILi{kind}E")
        assert len(hits) == 4, (kind, fam, sorted(hits))
        for n, u in hits.items():
            assert B.clean(u) and u["vgpr"] <= vgpr and u["occ"] >= occ and u["vgpr"] + u["agpr"] <= 256, (n, u)
            if "pair" in fam:
                assert u["occ"] >= 2, (n, u)


def test_the_policy_kernels_are_matrix_core_clean():
    """buildinfo.assert_matrix_core_clean's check in the unit these kernels live in (the helper reads rmav_policy_abi only): lanes are
    exchanged with v_permlane32_swap, never through LDS permutes, and the compiler-only packed-fp32 forms stay out - in the 48 kernels
    and in the unit's weak copies of the non-inlined fp32 nets (mlp_mfma32) the fp32 actor calls."""
    bodies = B.bodies("rmav_sensor_policy_abi")
    seen = {n: b for n, b in bodies.items() if re.match(r"_ZN4rmav(16k_rollout_nrm|17k_rollout_pair|24k_rollout_pair_shared)_snILi", n)}
    nets = {n: b for n, b in bodies.items() if n.startswith("_ZN4rmav10mlp_mfma32I")}
    assert len(seen) == 48 and len(nets) == 6
    for name, body in {**seen, **nets}.items():
        for bad in MATRIX_CORE_BAD:
            assert bad not in body, (name, bad)
    # the helper's own forms have not drifted from the tuple above: on the old policy unit it passes, and names these strings
    src = open(B.__file__).read()
    assert all(f'"{bad}"' in src for bad in MATRIX_CORE_BAD)


def test_no_kernel_duplicates_the_draw():
    """D_K = the instructions of k_observe<K>'s body - one evaluation of the draw and little else.  Each *_sn kernel has at most
    (sites + 1) D_K more instructions than the *_ds kernel it is cut from, sites = the places its body evaluates the draw:
      k_step_sn      1   (behind the dynamics: one z for final_obs and obs)
      k_rollout_sn   1   (in the loop, at the obs store)
      the three policy families without BOOT  2   (the prologue at t0; in the loop, behind the reset)
      the three policy families with BOOT     3   (... and the terminal observation of a truncated step)
    Observed: 0.55 .. 1.16, 1.28 .. 1.44 and 1.94 .. 2.16 D_K."""
    sn, snp, ds, pol = (B.bodies(u) for u in ("rmav_sensor_abi", "rmav_sensor_policy_abi", "rmav_disturb_abi", "rmav_policy_abi"))

    def body(bodies, prefix):
        return count(next(b for n, b in bodies.items() if n.startswith(prefix)))

    for kind in range(4):
        d_k = body(sn, f"_ZN4rmav9k_observeILi{kind}E")
        for tl in (0, 1):
            for rw in (0, 1):
                extra = body(sn, f"_ZN4rmav9k_step_snILi{kind}ELb{tl}ELb{rw}E") - body(ds, f"_ZN4rmav9k_step_dsILi{kind}ELb{tl}ELb{rw}E")
                assert 0 < extra <= 2 * d_k, ("step", kind, tl, rw, extra, d_k)
                for mode in range(3):
                    extra = (body(sn, f"_ZN4rmav12k_rollout_snILi{kind}ELi{mode}ELb{tl}ELb{rw}E") -
                             body(ds, f"_ZN4rmav12k_rollout_dsILi{kind}ELi{mode}ELb{tl}ELb{rw}E"))
                    assert 0 < extra <= 2 * d_k, ("rollout", kind, mode, tl, rw, extra, d_k)
        for fam in ("16k_rollout_nrm", "17k_rollout_pair", "24k_rollout_pair_shared"):
            for boot, sites in ((0, 2), (1, 3)):
                for rw in (0, 1):
                    extra = (body(snp, f"_ZN4rmav{fam}_snILi{kind}ELb{boot}ELb{rw}E") - body(pol, f"_ZN4rmav{fam}_dsILi{kind}ELb{boot}ELb{rw}E"))
                    assert 0 < extra <= (sites + 1) * d_k, (fam, kind, boot, rw, extra, d_k)

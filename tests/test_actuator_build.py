"""Actuator lag (rmav_set_actuator), what can be checked without a GPU: the four entry points are declared, exported and bound; the new
kernel families exist for the four quadrotor kinds with the members stated here, use no scratch and spill no vector register (`make asm`);
their names match no pre-existing family prefix and the older families keep their members; the two new units only launch; registers and
occupancy are what was observed (profiles/r20/actuator.md has the table beside the noisy kernels they are cut from)."""
import re

import pytest

import buildinfo as B
from test_disturbance_build import DISTURB, POLICY
from test_frame_skip_build import SKIP
from test_reward_build import REWARD
from test_sensor_noise_build import SENSOR, SENSOR_POLICY

NEW = {"rmav_set_actuator": ("int", 2), "rmav_get_actuator": ("int", 3), "rmav_get_actuator_state": ("int", 4), "rmav_set_actuator_state": ("int", 4)}
# family prefix -> members: k_step_al<K, TL, RW>; k_rollout_al<K, MODE in (buffer, random, controller), TL, RW> (one store policy);
# the policy rollouts k_rollout_nrm_al / k_rollout_pair_al / k_rollout_pair_shared_al<K, BOOT, RW> (rmav_actuator_policy_abi).
ACTUATOR = {"_ZN4rmav9k_step_alILi": 4 * 2 * 2, "_ZN4rmav12k_rollout_alILi": 4 * 3 * 2 * 2}
ACTUATOR_POLICY = {"_ZN4rmav16k_rollout_nrm_alILi": 4 * 2 * 2, "_ZN4rmav17k_rollout_pair_alILi": 4 * 2 * 2, "_ZN4rmav24k_rollout_pair_shared_alILi": 4 * 2 * 2}
# the two small launches that keep the handle's device data: every env's m = init, and the policy kernels' copy of the coefficients
SMALL = {"_ZN4rmav15k_actuator_fillEPfliNS_12ActuatorCoefE", "_ZN4rmav14k_set_actuatorEPjNS_12ActuatorCoefEj"}
MATRIX_CORE_BAD = ("ds_bpermute", "ds_permute", "v_pk_mul_f32", "v_pk_mov_b32")   # buildinfo.assert_matrix_core_clean's forms


def actuator_family(prefix):
    h = B.hits(prefix)
    assert len(h) == {**ACTUATOR, **ACTUATOR_POLICY}[prefix], (prefix, sorted(h))
    return h


def test_actuator_entry_points_are_declared_exported_and_bound(built):
    A, _ = B.assert_entry_points(NEW)
    import ctypes as C

    S = A.ActuatorSpec
    assert C.sizeof(S) == 32 and (S.tau.offset, S.tau.size, S.init.offset, S.init.size) == (0, 16, 16, 16)
    # RMAV_VERSION, the tuning keys and the set of public headers are what they were
    assert A.lib().rmav_version() == 101 and len(A.TUNE) == 9
    assert sorted(f for f in B.os.listdir(B.os.path.join(B.ROOT, "include"))) == ["rmav.h", "rmav_comm.h", "rmav_ppo.h"]


@pytest.mark.parametrize("prefix", sorted({**ACTUATOR, **ACTUATOR_POLICY}))
def test_every_new_family_exists_for_every_kind_and_is_clean(prefix):
    h = actuator_family(prefix)
    for kind in range(4):
        mine = [n for n in h if n.startswith(f"{prefix}{kind}E")]
        assert len(mine) == len(h) // 4, (prefix, kind, mine)
    for n, u in h.items():
        assert B.clean(u), (n, u)
        # alpha / beta / init by value; the policy kernels read the handle's device copy - and do not take ActRuleArgs as a parameter
        assert ("PolicyActuatorArgs" if prefix in ACTUATOR_POLICY else "_12ActuatorArgsE") in n, n
        assert "ActRuleArgs" not in n, n
    for n in SMALL:
        assert B.clean(B.usage()[n]), n


def test_no_new_name_matches_an_older_prefix():
    seen = {**B.family(*B.FAMILIES)}
    for census in (SKIP, REWARD, DISTURB, POLICY, SENSOR, SENSOR_POLICY):
        for p in census:
            h = B.hits(p)
            assert len(h) == census[p], (p, sorted(h))
            seen.update(h)
    new = {}
    for p in ACTUATOR:
        new.update(actuator_family(p))
    assert len(new) == 64 and not set(new) & set(seen)
    assert set(B.bodies("rmav_actuator_abi")) == set(new) | SMALL, "the unit holds the new kernels and nothing else"
    pol = {}
    for p in ACTUATOR_POLICY:
        pol.update(actuator_family(p))
    assert len(pol) == 48 and not set(pol) & set(seen)
    kernels = {n for n in B.bodies("rmav_actuator_policy_abi") if "k_" in n}
    assert kernels == set(pol), "the policy unit holds the three new actors and nothing else"
    # the listings of the units these kernels are cut from are what they were
    assert len(B.bodies("rmav_sensor_abi")) == 68 and len(B.bodies("rmav_disturb_abi")) == 69
    assert len({n for n in B.bodies("rmav_sensor_policy_abi") if "k_" in n}) == 49


def test_the_units_only_launch():
    mk = open(B.os.path.join(B.PKG, "Makefile")).read()
    for unit in ("rmav_actuator_abi", "rmav_actuator_policy_abi"):
        src = open(B.os.path.join(B.PKG, "csrc", unit + ".hip")).read()
        assert 'extern "C"' not in src, unit
        assert unit in mk
    # the filter statement is ONE function, in a header the host test program compiles too
    hdr = open(B.os.path.join(B.PKG, "csrc", "rmav_actuator.hpp")).read()
    assert hdr.count("__builtin_fmaf") == 1 and "RMAV_HD float actuator_filter" in hdr
    assert "rmav_actuator.hpp" in open(B.os.path.join(B.ROOT, "tests", "actuator_host", "actuator_host.hip")).read()


# (kind, registers and occupancy of k_step_al as observed; k_step_sn beside them: 51 / 7, 86 / 5, 61 / 7, 108 / 4)
@pytest.mark.parametrize("kind,vgpr,occ", [(0, 54, 7), (1, 86, 5), (2, 65, 7), (3, 112, 4)])
def test_single_step_kernels(kind, vgpr, occ):
    hits = B.hits(f"_ZN4rmav9k_step_alILi{kind}E")
    assert len(hits) == 4, sorted(hits)
    for n, u in hits.items():
        assert u["vgpr"] <= vgpr and u["occ"] == occ, (n, u)


# (kind, {mode: (registers, minimum occupancy)} of k_rollout_al as observed: +0 .. 5 over k_rollout_sn - the filter state beside the state;
# quadrotor3d with random actions drops from 5 to 4 waves per SIMD)
@pytest.mark.parametrize("kind,budget", [(0, {0: (91, 5), 1: (90, 5), 2: (111, 4)}), (1, {0: (135, 3), 1: (133, 3), 2: (155, 3)}),
                                         (2, {0: (105, 4), 1: (101, 4), 2: (113, 4)}), (3, {0: (168, 3), 1: (165, 3), 2: (184, 2)})])
def test_fused_lagged_kernels(kind, budget):
    for mode, (vgpr, occ) in budget.items():
        hits = B.hits(f"_ZN4rmav12k_rollout_alILi{kind}ELi{mode}E")
        assert len(hits) == 4, (kind, mode, sorted(hits))
        for n, u in hits.items():
            assert B.clean(u) and u["vgpr"] <= vgpr and u["occ"] >= occ, (n, u)


# (kind, registers of the three lagged actors as observed - all four (BOOT, RW) members within the figure - and their minimum occupancy; the
# noisy counterparts: tests/test_sensor_noise_build.py, profiles/r20/actuator.md)
@pytest.mark.parametrize("kind,budget", [(0, {"16k_rollout_nrm_al": (152, 3), "17k_rollout_pair_al": (188, 2), "24k_rollout_pair_shared_al": (156, 3)}),
                                         (1, {"16k_rollout_nrm_al": (173, 2), "17k_rollout_pair_al": (213, 2), "24k_rollout_pair_shared_al": (179, 2)}),
                                         (2, {"16k_rollout_nrm_al": (163, 2), "17k_rollout_pair_al": (204, 2), "24k_rollout_pair_shared_al": (171, 2)}),
                                         (3, {"16k_rollout_nrm_al": (205, 2), "17k_rollout_pair_al": (235, 2), "24k_rollout_pair_shared_al": (199, 2)})])
def test_lagged_policy_kernels(kind, budget):
    for fam, (vgpr, occ) in budget.items():
        hits = B.hits(f"_ZN4rmav{fam}ILi{kind}E")
        assert len(hits) == 4, (kind, fam, sorted(hits))
        for n, u in hits.items():
            assert B.clean(u) and u["vgpr"] <= vgpr and u["occ"] >= occ and u["vgpr"] + u["agpr"] <= 256, (n, u)
            if "pair" in fam:
                assert u["occ"] >= 2, (n, u)


def test_the_policy_kernels_are_matrix_core_clean():
    """buildinfo.assert_matrix_core_clean's check in the unit these kernels live in: lanes are exchanged with v_permlane32_swap, never
    through LDS permutes, and the compiler-only packed-fp32 forms stay out - in the 48 kernels and in the unit's copies of the non-inlined
    fp32 nets (mlp_mfma32) the fp32 actor calls."""
    bodies = B.bodies("rmav_actuator_policy_abi")
    seen = {n: b for n, b in bodies.items() if re.match(r"_ZN4rmav(16k_rollout_nrm|17k_rollout_pair|24k_rollout_pair_shared)_alILi", n)}
    nets = {n: b for n, b in bodies.items() if n.startswith("_ZN4rmav10mlp_mfma32I")}
    assert len(seen) == 48 and len(nets) == 6
    for name, body in {**seen, **nets}.items():
        for bad in MATRIX_CORE_BAD:
            assert bad not in body, (name, bad)

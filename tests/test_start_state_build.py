"""Start-state ranges (rmav_set_start_state), what can be checked without a GPU: the two entry points are declared, exported and bound; the
new kernel families exist for the four quadrotor kinds with the members stated here, use no scratch and spill no vector register
(`make asm`); their names match no pre-existing family prefix and the older families and units keep their members; the two new units only
launch; the map is one function with one fma; registers and occupancy are what was observed - never below the lagged kernel each member is
cut from (profiles/r21/start_state.md has the table)."""
import re

import pytest

import buildinfo as B
from test_actuator_build import ACTUATOR, ACTUATOR_POLICY
from test_actuator_build import SMALL as ACTUATOR_SMALL
from test_disturbance_build import DISTURB, POLICY
from test_frame_skip_build import SKIP
from test_reward_build import REWARD
from test_sensor_noise_build import SENSOR, SENSOR_POLICY

NEW = {"rmav_set_start_state": ("int", 2), "rmav_get_start_state": ("int", 3)}
# family prefix -> members: k_step_ss<K, TL, RW>; k_rollout_ss<K, MODE in (buffer, random, controller), TL, RW> (one store policy);
# the policy rollouts k_rollout_nrm_ss / k_rollout_pair_ss / k_rollout_pair_shared_ss<K, BOOT, RW> (rmav_start_policy_abi); k_reset_ss<K>.
START = {"_ZN4rmav9k_step_ssILi": 4 * 2 * 2, "_ZN4rmav12k_rollout_ssILi": 4 * 3 * 2 * 2, "_ZN4rmav10k_reset_ssILi": 4}
START_POLICY = {"_ZN4rmav16k_rollout_nrm_ssILi": 4 * 2 * 2, "_ZN4rmav17k_rollout_pair_ssILi": 4 * 2 * 2, "_ZN4rmav24k_rollout_pair_shared_ssILi": 4 * 2 * 2}
# the small launch that keeps the handle's device copy of the coefficients
SMALL = {"_ZN4rmav17k_set_start_stateEPjNS_9StartCoefEj"}
MATRIX_CORE_BAD = ("ds_bpermute", "ds_permute", "v_pk_mul_f32", "v_pk_mov_b32")   # buildinfo.assert_matrix_core_clean's forms


def start_family(prefix):
    h = B.hits(prefix)
    assert len(h) == {**START, **START_POLICY}[prefix], (prefix, sorted(h))
    return h


def lagged(name):
    """the usage of the *_al kernel a *_ss kernel is cut from: the same template arguments"""
    m = re.match(r"_ZN4rmav(\d+)(k_\w+?)_ssI(.*?)EEv", name)
    twin = [n for n in B.usage() if n.startswith(f"_ZN4rmav{m.group(1)}{m.group(2)}_alI{m.group(3)}EEv")]
    assert len(twin) == 1, (name, twin)
    return B.usage()[twin[0]]


def test_start_state_entry_points_are_declared_exported_and_bound(built):
    A, _ = B.assert_entry_points(NEW)
    import ctypes as C

    S = A.StartStateSpec
    assert C.sizeof(S) == 128 and (S.lo.offset, S.lo.size, S.hi.offset, S.hi.size) == (0, 64, 64, 64)
    # RMAV_VERSION, the tuning keys and the set of public headers are what they were
    assert A.lib().rmav_version() == 101 and len(A.TUNE) == 9
    assert sorted(f for f in B.os.listdir(B.os.path.join(B.ROOT, "include"))) == ["rmav.h", "rmav_comm.h", "rmav_ppo.h"]
    import gym_reinmav_amd as g

    assert g.StartState is not None and callable(g.check_start_state)


@pytest.mark.parametrize("prefix", sorted({**START, **START_POLICY}))
def test_every_new_family_exists_for_every_kind_and_is_clean(prefix):
    h = start_family(prefix)
    for kind in range(4):
        mine = [n for n in h if n.startswith(f"{prefix}{kind}E")]
        assert len(mine) == len(h) // 4, (prefix, kind, mine)
    for n, u in h.items():
        assert B.clean(u), (n, u)
        # h / m by value; the policy kernels read the handle's device copy - and do not take ActRuleArgs as a parameter
        if prefix in START_POLICY:
            assert "PolicyStartArgs" in n, n
        elif "k_reset_ss" in n:
            assert n.endswith("NS_9StartCoefE"), n
        else:
            assert n.endswith("_12ActuatorArgsENS_9StartArgsE"), n
        assert "ActRuleArgs" not in n, n
    for n in SMALL:
        assert B.clean(B.usage()[n]), n


def test_no_new_name_matches_an_older_prefix():
    seen = {**B.family(*B.FAMILIES)}
    for census in (SKIP, REWARD, DISTURB, POLICY, SENSOR, SENSOR_POLICY, ACTUATOR, ACTUATOR_POLICY):
        for p in census:
            h = B.hits(p)
            assert len(h) == census[p], (p, sorted(h))
            seen.update(h)
    new = {}
    for p in START:
        new.update(start_family(p))
    assert len(new) == 16 + 48 + 4 and not set(new) & set(seen)
    assert set(B.bodies("rmav_start_abi")) == set(new) | SMALL, "the unit holds the new kernels and nothing else"
    pol = {}
    for p in START_POLICY:
        pol.update(start_family(p))
    assert len(pol) == 3 * 16 and not set(pol) & set(seen)
    kernels = {n for n in B.bodies("rmav_start_policy_abi") if "k_" in n}
    assert kernels == set(pol), "the policy unit holds the three new actors and nothing else"
    # no kernel of the library carries the new suffix outside the two units
    assert {n for n in B.usage() if re.search(r"_ssI|k_set_start_state", n)} == set(new) | set(pol) | SMALL
    # the listings of the units these kernels are cut from are what they were
    assert set(B.bodies("rmav_actuator_abi")) == {n for p in ACTUATOR for n in B.hits(p)} | ACTUATOR_SMALL
    assert len({n for n in B.bodies("rmav_actuator_policy_abi") if "k_" in n}) == 48
    assert len(B.bodies("rmav_sensor_abi")) == 68 and len(B.bodies("rmav_disturb_abi")) == 69
    assert len({n for n in B.bodies("rmav_sensor_policy_abi") if "k_" in n}) == 49


def test_the_units_only_launch():
    mk = open(B.os.path.join(B.PKG, "Makefile")).read()
    for unit in ("rmav_start_abi", "rmav_start_policy_abi"):
        src = open(B.os.path.join(B.PKG, "csrc", unit + ".hip")).read()
        assert 'extern "C"' not in src, unit
        assert unit in mk
    # the map statement is ONE function with ONE fma, in a header the host test program compiles too
    hdr = open(B.os.path.join(B.PKG, "csrc", "rmav_start.hpp")).read()
    assert hdr.count("__builtin_fmaf") == 1 and "RMAV_HD float start_map" in hdr
    assert "rmav_start.hpp" in open(B.os.path.join(B.ROOT, "tests", "start_host", "start_host.hip")).read()
    # ... which every site goes through: the six places a fresh state is produced (the launch-head spare has an LDS and a register form)
    csrc = B.os.path.join(B.PKG, "csrc")
    uses = {f: open(B.os.path.join(csrc, f)).read().count("start_apply<NS>(") for f in B.os.listdir(csrc)}
    assert {f: c for f, c in uses.items() if c} == {"rmav_rollout_body.inc": 2, "rmav_rollout_reset.inc": 1, "rmav_pair_env_load.inc": 1, "rmav_pair_episode.inc": 1,
                                                    "rmav_kernels.hpp": 2}, uses
    for f in B.os.listdir(csrc):
        if f != "rmav_start.hpp":
            assert "start_map(" not in open(B.os.path.join(csrc, f)).read(), f


# (kind, registers and occupancy of k_step_ss as observed; k_step_al beside them: 54 / 7, 86 / 5, 65 / 7, 112 / 4)
@pytest.mark.parametrize("kind,vgpr,occ", [(0, 54, 7), (1, 87, 5), (2, 65, 7), (3, 112, 4)])
def test_single_step_kernels(kind, vgpr, occ):
    hits = B.hits(f"_ZN4rmav9k_step_ssILi{kind}E")
    assert len(hits) == 4, sorted(hits)
    for n, u in hits.items():
        assert u["vgpr"] <= vgpr and u["occ"] == occ and u["occ"] >= lagged(n)["occ"], (n, u)


@pytest.mark.parametrize("kind", range(4))
def test_the_reset_kernel(kind):
    (n, u), = B.hits(f"_ZN4rmav10k_reset_ssILi{kind}E").items()
    assert B.clean(u) and u["occ"] == 8 and u["vgpr"] <= 36, (n, u)


# (kind, {mode: (registers, minimum occupancy)} of k_rollout_ss as observed: +0 .. 1 over k_rollout_al, the same occupancy in every member)
@pytest.mark.parametrize("kind,budget", [(0, {0: (92, 5), 1: (90, 5), 2: (111, 4)}), (1, {0: (135, 3), 1: (133, 3), 2: (155, 3)}),
                                         (2, {0: (105, 4), 1: (101, 4), 2: (113, 4)}), (3, {0: (168, 3), 1: (165, 3), 2: (184, 2)})])
def test_fused_start_state_kernels(kind, budget):
    for mode, (vgpr, occ) in budget.items():
        hits = B.hits(f"_ZN4rmav12k_rollout_ssILi{kind}ELi{mode}E")
        assert len(hits) == 4, (kind, mode, sorted(hits))
        for n, u in hits.items():
            assert B.clean(u) and u["vgpr"] <= vgpr and u["occ"] >= occ and u["occ"] >= lagged(n)["occ"], (n, u, lagged(n))


# (kind, registers of the three actors as observed - all four (BOOT, RW) members within the figure - and their minimum occupancy; the lagged
# counterparts: tests/test_actuator_build.py, profiles/r21/start_state.md)
@pytest.mark.parametrize("kind,budget", [(0, {"16k_rollout_nrm_ss": (152, 3), "17k_rollout_pair_ss": (188, 2), "24k_rollout_pair_shared_ss": (156, 3)}),
                                         (1, {"16k_rollout_nrm_ss": (173, 2), "17k_rollout_pair_ss": (214, 2), "24k_rollout_pair_shared_ss": (179, 2)}),
                                         (2, {"16k_rollout_nrm_ss": (163, 2), "17k_rollout_pair_ss": (204, 2), "24k_rollout_pair_shared_ss": (171, 2)}),
                                         (3, {"16k_rollout_nrm_ss": (205, 2), "17k_rollout_pair_ss": (236, 2), "24k_rollout_pair_shared_ss": (200, 2)})])
def test_start_state_policy_kernels(kind, budget):
    for fam, (vgpr, occ) in budget.items():
        hits = B.hits(f"_ZN4rmav{fam}ILi{kind}E")
        assert len(hits) == 4, (kind, fam, sorted(hits))
        for n, u in hits.items():
            assert B.clean(u) and u["vgpr"] <= vgpr and u["occ"] >= occ and u["vgpr"] + u["agpr"] <= 256, (n, u)
            assert u["occ"] >= lagged(n)["occ"], (n, u, lagged(n))
            if "pair" in fam:
                assert u["occ"] >= 2, (n, u)


def test_the_policy_kernels_are_matrix_core_clean():
    """buildinfo.assert_matrix_core_clean's check in the unit these kernels live in: lanes are exchanged with v_permlane32_swap, never
    through LDS permutes, and the compiler-only packed-fp32 forms stay out - in the 48 kernels and in the unit's copies of the non-inlined
    fp32 nets (mlp_mfma32) the fp32 actor calls."""
    bodies = B.bodies("rmav_start_policy_abi")
    seen = {n: b for n, b in bodies.items() if re.match(r"_ZN4rmav(16k_rollout_nrm|17k_rollout_pair|24k_rollout_pair_shared)_ssILi", n)}
    nets = {n: b for n, b in bodies.items() if n.startswith("_ZN4rmav10mlp_mfma32I")}
    assert len(seen) == 48 and len(nets) == 6
    for name, body in {**seen, **nets}.items():
        for bad in MATRIX_CORE_BAD:
            assert bad not in body, (name, bad)

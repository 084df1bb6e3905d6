"""Termination rules (rmav_set_termination), what can be checked without a GPU: the two entry points are declared, exported and bound; the
new kernel families exist for the four quadrotor kinds with the members stated here, use no scratch and spill no vector register
(`make asm`); their names match no pre-existing family prefix and the older families and units keep their members; the two new units only
launch; the rule is one function, called from the three guarded sites; registers and occupancy are what was observed, beside the kernel of
a start-state spec each member is cut from (profiles/r22/termination.md has the table)."""
import re

import pytest

import buildinfo as B
from test_actuator_build import ACTUATOR, ACTUATOR_POLICY
from test_disturbance_build import DISTURB, POLICY
from test_frame_skip_build import SKIP
from test_reward_build import REWARD
from test_sensor_noise_build import SENSOR, SENSOR_POLICY
from test_start_state_build import SMALL as START_SMALL
from test_start_state_build import START, START_POLICY

NEW = {"rmav_set_termination": ("int", 2), "rmav_get_termination": ("int", 3)}
# family prefix -> members: k_step_tc<K, TL, RW>; k_rollout_tc<K, MODE in (buffer, random, controller), TL, RW> (one store policy);
# the policy rollouts k_rollout_nrm_tc / k_rollout_pair_tc / k_rollout_pair_shared_tc<K, BOOT, RW> (rmav_term_policy_abi).
TERM = {"_ZN4rmav9k_step_tcILi": 4 * 2 * 2, "_ZN4rmav12k_rollout_tcILi": 4 * 3 * 2 * 2}
TERM_POLICY = {"_ZN4rmav16k_rollout_nrm_tcILi": 4 * 2 * 2, "_ZN4rmav17k_rollout_pair_tcILi": 4 * 2 * 2, "_ZN4rmav24k_rollout_pair_shared_tcILi": 4 * 2 * 2}
# the small launch that keeps the handle's device copy of the thresholds
SMALL = {"_ZN4rmav17k_set_terminationEPjNS_8TermArgsEj"}
MATRIX_CORE_BAD = ("ds_bpermute", "ds_permute", "v_pk_mul_f32", "v_pk_mov_b32")   # buildinfo.assert_matrix_core_clean's forms


def term_family(prefix):
    h = B.hits(prefix)
    assert len(h) == {**TERM, **TERM_POLICY}[prefix], (prefix, sorted(h))
    return h


def started(name):
    """the usage of the *_ss kernel a *_tc kernel is cut from: the same template arguments"""
    m = re.match(r"_ZN4rmav(\d+)(k_\w+?)_tcI(.*?)EEv", name)
    twin = [n for n in B.usage() if n.startswith(f"_ZN4rmav{m.group(1)}{m.group(2)}_ssI{m.group(3)}EEv")]
    assert len(twin) == 1, (name, twin)
    return B.usage()[twin[0]]


# The members whose occupancy is below their start-state twin's, as observed: the quadrotor3d-slungload buffer rollouts with the tracking
# reward sit one register over the three-wave line (169 against 168: the seven thresholds live in scalar registers through the step loop of
# a kernel that already spills scalars into vector lanes; profiles/r22/termination.md).
LOWER = ("_ZN4rmav12k_rollout_tcILi3ELi0ELb0ELb1E", "_ZN4rmav12k_rollout_tcILi3ELi0ELb1ELb1E")


def occ_ok(name, u):
    """not below the start-state twin's, but for the members listed in LOWER, which are one wave below"""
    twin = started(name)
    if name.startswith(LOWER):
        return u["occ"] == twin["occ"] - 1
    return u["occ"] >= twin["occ"]


def test_termination_entry_points_are_declared_exported_and_bound(built):
    A, _ = B.assert_entry_points(NEW)
    import ctypes as C

    S = A.TerminationSpec
    assert C.sizeof(S) == 32
    assert (S.pos_lo.offset, S.pos_lo.size, S.pos_hi.offset, S.pos_hi.size, S.max_tilt.offset, S._reserved.offset) == (0, 12, 12, 12, 24, 28)
    # RMAV_VERSION, the tuning keys and the set of public headers are what they were
    assert A.lib().rmav_version() == 101 and len(A.TUNE) == 9
    assert sorted(f for f in B.os.listdir(B.os.path.join(B.ROOT, "include"))) == ["rmav.h", "rmav_comm.h", "rmav_ppo.h"]
    import gym_reinmav_amd as g

    assert g.Termination is not None and callable(g.check_termination)


@pytest.mark.parametrize("prefix", sorted({**TERM, **TERM_POLICY}))
def test_every_new_family_exists_for_every_kind_and_is_clean(prefix):
    h = term_family(prefix)
    for kind in range(4):
        mine = [n for n in h if n.startswith(f"{prefix}{kind}E")]
        assert len(mine) == len(h) // 4, (prefix, kind, mine)
    for n, u in h.items():
        assert B.clean(u), (n, u)
        # the thresholds by value; the policy kernels read the handle's device copy - and do not take ActRuleArgs as a parameter
        if prefix in TERM_POLICY:
            assert n.endswith("NS_14PolicyTermArgsE"), n
        else:
            assert n.endswith("_12ActuatorArgsENS_9StartArgsENS_8TermArgsE"), n
        assert "ActRuleArgs" not in n, n
    for n in SMALL:
        assert B.clean(B.usage()[n]), n


def test_no_new_name_matches_an_older_prefix():
    seen = {**B.family(*B.FAMILIES)}
    for census in (SKIP, REWARD, DISTURB, POLICY, SENSOR, SENSOR_POLICY, ACTUATOR, ACTUATOR_POLICY, START, START_POLICY):
        for p in census:
            h = B.hits(p)
            assert len(h) == census[p], (p, sorted(h))
            seen.update(h)
    new = {}
    for p in TERM:
        new.update(term_family(p))
    assert len(new) == 16 + 48 and not set(new) & set(seen)
    assert set(B.bodies("rmav_term_abi")) == set(new) | SMALL, "the unit holds the new kernels and nothing else"
    pol = {}
    for p in TERM_POLICY:
        pol.update(term_family(p))
    assert len(pol) == 3 * 16 and not set(pol) & set(seen)
    kernels = {n for n in B.bodies("rmav_term_policy_abi") if "k_" in n}
    assert kernels == set(pol), "the policy unit holds the three new actors and nothing else"
    # no kernel of the library carries the new suffix outside the two units
    assert {n for n in B.usage() if re.search(r"_tcI|k_set_termination", n)} == set(new) | set(pol) | SMALL
    # the listings of the units these kernels are cut from are what they were
    assert set(B.bodies("rmav_start_abi")) == {n for p in START for n in B.hits(p)} | START_SMALL
    assert len({n for n in B.bodies("rmav_start_policy_abi") if "k_" in n}) == 48
    # sixteen translation units: the most a build may compile side by side
    mk = open(B.os.path.join(B.PKG, "Makefile")).read()
    units = re.search(r"^ABI_UNITS\s*:=(.*)$", mk, re.M).group(1).split() + re.search(r"^POLICY_UNITS\s*:=(.*)$", mk, re.M).group(1).split()
    assert len(units) == 16 and units[-1] == "rmav_term_policy_abi" and "rmav_term_abi" in units


def test_the_units_only_launch():
    mk = open(B.os.path.join(B.PKG, "Makefile")).read()
    for unit in ("rmav_term_abi", "rmav_term_policy_abi"):
        src = open(B.os.path.join(B.PKG, "csrc", unit + ".hip")).read()
        assert 'extern "C"' not in src, unit
        assert unit in mk
    # the rule is ONE function template, in a header the host test program compiles too
    hdr = open(B.os.path.join(B.PKG, "csrc", "rmav_term.hpp")).read()
    assert hdr.count("RMAV_HD bool term_rule(") == 1 and "struct TermArgs" in hdr and "sizeof(TermArgs) == 32" in hdr
    assert "rmav_term.hpp" in open(B.os.path.join(B.ROOT, "tests", "term_host", "term_host.hip")).read()
    # ... which is called from the three guarded sites and nowhere else: one statement each, behind Env<K>::step
    csrc = B.os.path.join(B.PKG, "csrc")
    def calls(f):
        return sum("term_rule<K>(s, " in ln and not ln.lstrip().startswith("//") for ln in open(B.os.path.join(csrc, f)).read().split("\n"))

    uses = {f: calls(f) for f in B.os.listdir(csrc)}
    assert {f: c for f, c in uses.items() if c and f != "rmav_term.hpp"} == {"rmav_rollout_body.inc": 1, "rmav_pair_dynamics.inc": 1, "rmav_kernels.hpp": 1}, uses
    for f, guard in (("rmav_rollout_body.inc", "#if RMAV_ROLLOUT_TC"), ("rmav_pair_dynamics.inc", "#if RMAV_PAIR_TC"), ("rmav_kernels.hpp", "if constexpr (TC)")):
        lines = open(B.os.path.join(csrc, f)).read().split("\n")
        at, = [i for i, ln in enumerate(lines) if "term_rule<K>(s, " in ln and not ln.lstrip().startswith("//")]
        assert any(guard in ln for ln in lines[at - 4:at + 1]), (f, lines[at - 4:at + 1])
        assert any("Env<K>::step(" in ln for ln in lines[at - 10:at]), f
    # the guards default to 0
    assert "#define RMAV_ROLLOUT_TC 0" in open(B.os.path.join(csrc, "rmav_kernels.hpp")).read()
    assert "#define RMAV_PAIR_TC 0" in open(B.os.path.join(csrc, "rmav_policy_pair.hpp")).read()


# (kind, registers and occupancy of k_step_tc as observed; k_step_ss beside them: 54 / 7, 87 / 5, 65 / 7, 112 / 4)
@pytest.mark.parametrize("kind,vgpr,occ", [(0, 54, 7), (1, 87, 5), (2, 67, 7), (3, 112, 4)])
def test_single_step_kernels(kind, vgpr, occ):
    hits = B.hits(f"_ZN4rmav9k_step_tcILi{kind}E")
    assert len(hits) == 4, sorted(hits)
    for n, u in hits.items():
        assert u["vgpr"] <= vgpr and u["occ"] == occ and occ_ok(n, u), (n, u)


# (kind, {mode: (registers, minimum occupancy)} of k_rollout_tc as observed: +0 .. 1 over k_rollout_ss)
@pytest.mark.parametrize("kind,budget", [(0, {0: (92, 5), 1: (91, 5), 2: (111, 4)}), (1, {0: (135, 3), 1: (133, 3), 2: (155, 3)}),
                                         (2, {0: (105, 4), 1: (101, 4), 2: (113, 4)}), (3, {0: (169, 2), 1: (165, 3), 2: (184, 2)})])
def test_fused_termination_kernels(kind, budget):
    for mode, (vgpr, occ) in budget.items():
        hits = B.hits(f"_ZN4rmav12k_rollout_tcILi{kind}ELi{mode}E")
        assert len(hits) == 4, (kind, mode, sorted(hits))
        for n, u in hits.items():
            assert B.clean(u) and u["vgpr"] <= vgpr and u["occ"] >= occ and occ_ok(n, u), (n, u, started(n))


# (kind, registers of the three actors as observed - all four (BOOT, RW) members within the figure - and their minimum occupancy)
@pytest.mark.parametrize("kind,budget", [(0, {"16k_rollout_nrm_tc": (152, 3), "17k_rollout_pair_tc": (188, 2), "24k_rollout_pair_shared_tc": (156, 3)}),
                                         (1, {"16k_rollout_nrm_tc": (173, 2), "17k_rollout_pair_tc": (214, 2), "24k_rollout_pair_shared_tc": (179, 2)}),
                                         (2, {"16k_rollout_nrm_tc": (163, 2), "17k_rollout_pair_tc": (204, 2), "24k_rollout_pair_shared_tc": (171, 2)}),
                                         (3, {"16k_rollout_nrm_tc": (205, 2), "17k_rollout_pair_tc": (236, 2), "24k_rollout_pair_shared_tc": (200, 2)})])
def test_termination_policy_kernels(kind, budget):
    for fam, (vgpr, occ) in budget.items():
        hits = B.hits(f"_ZN4rmav{fam}ILi{kind}E")
        assert len(hits) == 4, (kind, fam, sorted(hits))
        for n, u in hits.items():
            assert B.clean(u) and u["vgpr"] <= vgpr and u["occ"] >= occ and u["vgpr"] + u["agpr"] <= 256, (n, u)
            assert occ_ok(n, u), (n, u, started(n))
            if "pair" in fam:
                assert u["occ"] >= 2, (n, u)


def test_the_policy_kernels_are_matrix_core_clean():
    """buildinfo.assert_matrix_core_clean's check in the unit these kernels live in: lanes are exchanged with v_permlane32_swap, never
    through LDS permutes, and the compiler-only packed-fp32 forms stay out - in the 48 kernels and in the unit's copies of the non-inlined
    fp32 nets (mlp_mfma32) the fp32 actor calls."""
    bodies = B.bodies("rmav_term_policy_abi")
    seen = {n: b for n, b in bodies.items() if re.match(r"_ZN4rmav(16k_rollout_nrm|17k_rollout_pair|24k_rollout_pair_shared)_tcILi", n)}
    nets = {n: b for n, b in bodies.items() if n.startswith("_ZN4rmav10mlp_mfma32I")}
    assert len(seen) == 48 and len(nets) == 6
    for name, body in {**seen, **nets}.items():
        for bad in MATRIX_CORE_BAD:
            assert bad not in body, (name, bad)

"""Frame skip (rmav_set_frame_skip), what can be checked without a GPU: the two entry points are declared, exported and bound; the five
new kernel families exist for the four quadrotor kinds with the members stated here, use no scratch and keep the occupancy of the
kernels they are cut from (`make asm`); and their names match no pre-existing family prefix, so the census of tests/buildinfo.py holds."""
import pytest

import buildinfo as B

NEW = {"rmav_set_frame_skip": ("int", 2), "rmav_get_frame_skip": ("int", 2)}
# family prefix -> members: k_step_fs<K, TL>; k_rollout_fs<K, MODE in (buffer, random, controller), ST in (default, write-through, stream),
# TL>; the three policy families <K, BOOT>
SKIP = {"_ZN4rmav9k_step_fsILi": 4 * 2, "_ZN4rmav12k_rollout_fsILi": 4 * 3 * 3 * 2, "_ZN4rmav16k_rollout_nrm_fsILi": 4 * 2,
        "_ZN4rmav17k_rollout_pair_fsILi": 4 * 2, "_ZN4rmav24k_rollout_pair_shared_fsILi": 4 * 2}


def skip_family(prefix):
    h = B.hits(prefix)
    assert len(h) == SKIP[prefix], (prefix, sorted(h))
    return h


def test_frame_skip_entry_points_are_declared_exported_and_bound(built):
    B.assert_entry_points(NEW)


@pytest.mark.parametrize("prefix", sorted(SKIP))
def test_every_new_family_exists_for_every_kind_and_is_clean(prefix):
    h = skip_family(prefix)
    for kind in range(4):
        mine = [n for n in h if n.startswith(f"{prefix}{kind}E")]
        assert len(mine) == SKIP[prefix] // 4, (prefix, kind, mine)
    for n, u in h.items():
        assert B.clean(u), (n, u)
        assert "FrameSkipArgs" in n or "PolicySkipArgs" in n, n   # the loop bound is a trailing argument of its own


def test_single_step_kernel_of_quadrotor3d_stays_at_full_occupancy():
    hits = B.hits("_ZN4rmav9k_step_fsILi2E")
    assert len(hits) == 2, sorted(hits)
    for n, u in hits.items():
        assert u["vgpr"] <= 48 and u["occ"] == 8, (n, u)


# (kind, register budget of test_fused_ranged_kernels, its occupancy)
@pytest.mark.parametrize("kind,ranged_budget,min_occ", [(0, 72, 7), (1, 116, 4), (2, 80, 6), (3, 144, 3)])
def test_fused_frame_skip_kernels(kind, ranged_budget, min_occ):
    """k_rollout_fs<K, MODE, ST, TL>: the caller- and random-action kernels reach the occupancy of the ranged kernels they are cut from
    (test_domain_rand_build.py::test_fused_ranged_kernels) within its budgets + 4 registers.  Observed increase over k_rollout_dr:
    +2 (quadrotor2d: 70 -> 72), +4 (quadrotor2d-slungload: 109 / 113 -> 113 / 117), +0 .. 1 (quadrotor3d: 69 / 71 -> 70 / 71), +4 .. 5
    (quadrotor3d-slungload: 133 / 134 -> 137 / 138) - the held action, the accumulated reward and the sub-step counter stay live across
    the one rolled call site of Env<K>::step, and the `live` predicate takes a scalar pair."""
    for mode in (0, 1, 2):
        hits = B.hits(f"_ZN4rmav12k_rollout_fsILi{kind}ELi{mode}E")
        assert len(hits) == 6, (kind, mode, sorted(hits))
        for n, u in hits.items():
            assert B.clean(u), (n, u)
            if mode != 2:
                assert u["vgpr"] <= ranged_budget + 4 and u["occ"] >= min_occ, (n, u)


def test_policy_frame_skip_kernels():
    """k_rollout_nrm_fs, k_rollout_pair_fs, k_rollout_pair_shared_fs <K, BOOT>: no scratch; at most 256 registers; the pair actors at two
    wavefronts per SIMD or more; no LDS permutes and no compiler-packed fp32 in the matrix-core kernels."""
    one = skip_family("_ZN4rmav16k_rollout_nrm_fsILi")
    pairs = {**skip_family("_ZN4rmav17k_rollout_pair_fsILi"), **skip_family("_ZN4rmav24k_rollout_pair_shared_fsILi")}
    for n, u in {**one, **pairs}.items():
        assert B.clean(u) and u["vgpr"] + u["agpr"] <= 256, (n, u)
    for n, u in pairs.items():
        assert u["occ"] >= 2, (n, u)
    B.assert_matrix_core_clean(r"_ZN4rmav(16k_rollout_nrm_fs|17k_rollout_pair_fs|24k_rollout_pair_shared_fs)ILi", 24)


def test_the_sub_step_loop_is_rolled():
    """One call site of the dynamics per kernel: the fp64 slung-load step is inlined once, so a frame-skip kernel is not k times the size
    of the ranged kernel it is cut from (bound: 1.5 x its instruction count)."""
    skip, ranged = B.bodies("rmav_skip_abi"), B.bodies("rmav_range_abi")
    count = lambda body: sum(1 for ln in body.split("\n") if ln.startswith("\t") and not ln.startswith("\t."))
    for kind in range(4):
        s = next(b for n, b in skip.items() if n.startswith(f"_ZN4rmav12k_rollout_fsILi{kind}ELi1ELi0ELb0E"))
        r = next(b for n, b in ranged.items() if n.startswith(f"_ZN4rmav12k_rollout_drILi{kind}ELi1ELi0ELb0E"))
        assert count(s) <= 1.5 * count(r), (kind, count(s), count(r))


def test_the_census_of_the_other_families_is_unchanged():
    """No pre-existing prefix matches a new symbol, and the new unit holds exactly the step and one-wavefront rollout kernels."""
    seen = B.family(*B.FAMILIES)
    new = {}
    for p in SKIP:
        new.update(skip_family(p))
    assert len(new) == 104 and not set(new) & set(seen)
    assert {n for n in B.bodies("rmav_skip_abi") if "k_step_fs" in n or "k_rollout_fs" in n} == \
        set(skip_family("_ZN4rmav9k_step_fsILi")) | set(skip_family("_ZN4rmav12k_rollout_fsILi"))

"""Per-episode domain randomisation, what can be checked without a GPU: the three entry points are declared, exported and bound, the
ranged kernels exist for K = 0..3 with the resource budgets of the kernels they stand beside (`make asm`, as test_time_limit_build.py),
and no pre-existing kernel family gained or lost a member."""
import os

import pytest

import buildinfo as B

NEW = {name: ("int", None) for name in ("rmav_set_env_param_range", "rmav_get_env_param_range", "rmav_get_env_param")}


def test_domain_rand_entry_points_are_declared_exported_and_bound(built):
    B.assert_entry_points(NEW)
    # the RNG table documents the stream
    assert "(4<<24)" in open(os.path.join(B.ROOT, "include", "rmav.h")).read()


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_single_step_ranged_kernels(kind):
    """k_step_dr<K, CTRL, TL>: no scratch, no spills, and no bigger than the time-limited single-step kernel of the same kind plus the
    few registers of the draw (k_step_tl of quadrotor3d: <= 48 VGPRs at occupancy 8)."""
    hits = B.hits(f"_ZN4rmav9k_step_drILi{kind}E")
    assert len(hits) == 4, sorted(hits)
    for n, u in hits.items():
        assert B.clean(u), (n, u)
    if kind == 2:
        u = next(iter(B.hits("_ZN4rmav9k_step_drILi2ELb0ELb0E").values()))
        assert u["vgpr"] <= 48 and u["occ"] == 8, u


@pytest.mark.parametrize("kind,budget,min_occ", [(0, 72, 7), (1, 116, 4), (2, 80, 6), (3, 144, 3)])
def test_fused_ranged_kernels(kind, budget, min_occ):
    """k_rollout_dr<K, MODE, ST, TL> for ACT_BUFFER, ACT_RANDOM, ACT_CONTROLLER, three store policies, with and without a time limit: no
    scratch, no spills; the caller- and random-action kernels at the occupancy of k_rollout_tl (test_time_limit_build.py) and within
    8 / 12 registers of its budgets for the two 2-D kinds (the redraw keeps three spare constants and the fp64 re-derivation live)."""
    for mode in (0, 1, 2):
        hits = B.hits(f"_ZN4rmav12k_rollout_drILi{kind}ELi{mode}E")
        assert len(hits) == 6, (kind, mode, sorted(hits))
        for n, u in hits.items():
            assert B.clean(u), (n, u)
            if mode != 2:
                assert u["vgpr"] <= budget and u["occ"] >= min_occ, (n, u)


def test_policy_ranged_kernels():
    """k_rollout_nrm_dr<K, BOOT>, k_rollout_pair_dr<K, BOOT> and k_rollout_pair_shared_dr<K, BOOT>, K = 0..3: no scratch; the pair actors
    within 256 registers at two wavefronts per SIMD; the matrix-core kernels free of LDS permutes and compiler-packed fp32."""
    one = B.family("_ZN4rmav16k_rollout_nrm_drILi")
    pairs = B.family("_ZN4rmav17k_rollout_pair_drILi", "_ZN4rmav24k_rollout_pair_shared_drILi")
    assert len(one) == 8 and len(pairs) == 16, (sorted(one), sorted(pairs))
    for n, u in one.items():
        assert B.clean(u) and u["vgpr"] + u["agpr"] <= 256, (n, u)
    for n, u in pairs.items():
        assert u["vgpr"] + u["agpr"] <= 256 and B.clean(u) and u["occ"] >= 2, (n, u)
    B.assert_matrix_core_clean(r"_ZN4rmav(17k_rollout_pair_dr|24k_rollout_pair_shared_dr|16k_rollout_nrm_dr)", 24)


def test_no_new_kernel_uses_scratch_and_families_are_unchanged():
    """Every kernel of the new translation unit is clean, and the ranged kernels have names no pre-existing prefix matches: the
    families test_resource_usage.py / test_time_limit_build.py count keep their sizes."""
    new = B.family(*B.RANGED)
    assert len(new) == 16 + 72 + 24 + 1, len(new)
    for n, u in new.items():
        assert B.clean(u), (n, u)
    B.family(*B.FAMILIES)

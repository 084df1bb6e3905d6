"""Episode time limits, what can be checked without a GPU: the three entry points are declared, exported and bound, and the
time-limited kernels exist with the resource budgets of the kernels they stand beside (`make asm`, as test_resource_usage.py)."""
import pytest

import buildinfo as B

NEW = {name: ("int", None) for name in ("rmav_set_time_limit", "rmav_get_time_limit", "rmav_episode_truncated")}


def test_time_limit_entry_points_are_declared_exported_and_bound(built):
    B.assert_entry_points(NEW)


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_single_step_time_limit_kernels(kind):
    for ctrl in (0, 1):
        hits = B.hits(f"_ZN4rmav9k_step_tlILi{kind}ELb{ctrl}E")
        assert hits, (kind, ctrl)
        for n, u in hits.items():
            assert B.clean(u), (n, u)
    # the shipped store policy of the small batches: as small as k_step itself (test_single_step_kernel_is_small)
    u = next(iter(B.hits("_ZN4rmav9k_step_tlILi2ELb0ELi0E").values()))
    assert u["vgpr"] <= 48 and u["occ"] == 8, u


@pytest.mark.parametrize("kind,budget,min_occ", [(0, 64, 7), (1, 104, 4), (2, 80, 6), (3, 144, 3)])
def test_fused_time_limit_kernels(kind, budget, min_occ):
    """k_rollout_tl<K, MODE, ST> for ACT_BUFFER, ACT_RANDOM, ACT_CONTROLLER and ACT_POLICY_F32M: no scratch, no spills; the caller-
    and random-action kernels within the one-wavefront budgets of test_one_wavefront_rollout_register_budget."""
    for mode in (0, 1, 2, 8):
        hits = B.hits(f"_ZN4rmav12k_rollout_tlILi{kind}ELi{mode}E")
        assert hits, (kind, mode)
        for n, u in hits.items():
            assert B.clean(u), (n, u)
    for mode, st in ((1, 2), (1, 0), (0, 0)):
        u = next(iter(B.hits(f"_ZN4rmav12k_rollout_tlILi{kind}ELi{mode}ELi{st}E").values()))
        assert u["vgpr"] <= budget and u["occ"] >= min_occ, (kind, mode, st, u)
    u = next(iter(B.hits(f"_ZN4rmav12k_rollout_tlILi{kind}ELi8ELi0E").values()))
    assert u["vgpr"] + u["agpr"] <= 256, u


def test_pair_time_limit_kernels():
    """k_rollout_pair_tl<K, FMT_F16> and k_rollout_pair_shared_tl<K>, K = 0..3: two wavefronts per SIMD, no scratch."""
    hits = B.family("_ZN4rmav17k_rollout_pair_tlILi", "_ZN4rmav24k_rollout_pair_shared_tlILi")
    assert len(hits) == 8, sorted(hits)
    for n, u in hits.items():
        assert u["vgpr"] + u["agpr"] <= 256 and B.clean(u) and u["occ"] >= 2, (n, u)
    # the time-limited matrix-core kernels keep the LDS permutes and compiler-packed fp32 out as well
    B.assert_matrix_core_clean(r"_ZN4rmav(17k_rollout_pair_tl|24k_rollout_pair_shared_tl|12k_rollout_tlILi\dELi8E)", 12)

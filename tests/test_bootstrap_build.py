"""Terminal observations and the bootstrap term of truncated steps, what can be checked without a GPU: the three entry points are
declared, exported and bound, and the new kernels exist for the four quadrotor kinds with the resource budgets of the time-limited
kernels they stand beside (`make asm`, as test_time_limit_build.py)."""
import os

import pytest

import buildinfo as B

NEW = {"rmav_step_final": ("int", 9), "rmav_rollout_policy_boot": ("int", 12), "rmav_gae_boot": ("int", 12)}


def test_bootstrap_entry_points_are_declared_exported_and_bound(built):
    B.assert_entry_points(NEW)


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_single_step_final_kernels(kind):
    """k_step_final<K, TL, ST>: with and without a limit, the three store policies; no scratch, no spills, and no more than two
    registers above the k_step_tl kernel of the same kind and store policy (the finishing lanes' store address)."""
    for tl in (0, 1):
        hits = B.hits(f"_ZN4rmav12k_step_finalILi{kind}ELb{tl}E")
        assert len(hits) == 3, (kind, tl, sorted(hits))
        for n, u in hits.items():
            assert B.clean(u), (n, u)
    for st in (0, 1, 2):
        u = next(iter(B.hits(f"_ZN4rmav12k_step_finalILi{kind}ELb1ELi{st}E").values()))
        ref = next(iter(B.hits(f"_ZN4rmav9k_step_tlILi{kind}ELb0ELi{st}E").values()))
        assert u["vgpr"] <= ref["vgpr"] + 2 and u["occ"] >= ref["occ"], (kind, st, u, ref)


def test_fused_boot_kernels():
    """k_rollout_boot<K, ACT_POLICY_F32M>, k_rollout_pair_boot<K, FMT_F16>, k_rollout_pair_shared_boot<K>, K = 0..3: no scratch, no
    spills, VGPR + AGPR <= 256, the pair kernels two wavefronts per SIMD - and none below the occupancy of its time-limited sibling."""
    fam = (("_ZN4rmav14k_rollout_bootILi{k}ELi8ELi0E", "_ZN4rmav12k_rollout_tlILi{k}ELi8ELi0E", 1),
           ("_ZN4rmav19k_rollout_pair_bootILi{k}ELi1E", "_ZN4rmav17k_rollout_pair_tlILi{k}ELi1E", 2),
           ("_ZN4rmav26k_rollout_pair_shared_bootILi{k}E", "_ZN4rmav24k_rollout_pair_shared_tlILi{k}E", 2))
    for new, old, min_occ in fam:
        for k in range(4):
            h, o = B.hits(new.format(k=k)), B.hits(old.format(k=k))
            assert len(h) == 1 and len(o) == 1, (new, k, sorted(h), sorted(o))
            (n, u), ref = next(iter(h.items())), next(iter(o.values()))
            assert u["vgpr"] + u["agpr"] <= 256 and B.clean(u) and u["occ"] >= min_occ and u["occ"] >= ref["occ"], (n, u, ref)
    # the matrix-core kernels keep the LDS permutes and compiler-packed fp32 out (the rule test_pair_time_limit_kernels applies to their siblings)
    B.assert_matrix_core_clean(r"_ZN4rmav(19k_rollout_pair_boot|26k_rollout_pair_shared_boot|14k_rollout_bootILi\dELi8E)", 12)


def test_gae_boot_kernel():
    """k_gae_boot: k_gae with one more load stream - no scratch, no spills; k_gae itself is still there"""
    new, old = B.hits("_ZN4rmav10k_gae_bootE"), B.hits("_ZN4rmav5k_gaeE")
    assert len(new) == 1 and len(old) == 1
    u = next(iter(new.values()))
    assert B.clean(u) and u["occ"] >= 2, u


def test_the_larger_tiles_fit_the_lds_budget():
    """LDS bytes of a 4-pair workgroup (the largest RMAV_TUNE_PAIR_GROUP) of the *_boot pair kernels for the 16-state kind, from the
    tile definitions of csrc/rmav_policy_pair.hpp: weights + 4 x (noise tile + 2 output rows + 2 terminal-state areas) <= 160 KiB."""
    src = open(os.path.join(B.PKG, "csrc", "rmav_policy_pair.hpp")).read()
    assert "struct PairBootTile" in src and "struct SharedBootTile" in src
    ns, na, g = 16, 4, 4
    z_words = 2 * 4 * 64
    o_half = (ns + 2 + na) * 64
    pair = z_words + 2 * o_half
    boot = pair + 2 * ns * 64
    shared_boot = pair + 4 * 32 + 2 * ns * 64
    net = 2 * 64 * 8 // 2 + 8 * 64 * 8 // 2 + 4 * 64 * 8 // 2 + 64 + 64 + 32    # MfmaLayout::NET: f16 fragments (two per word) + biases
    assert 4 * (2 * net + 4 + g * boot) <= 160 * 1024
    assert 4 * (net + 4 + g * shared_boot) <= 160 * 1024

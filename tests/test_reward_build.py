"""Tracking reward (rmav_set_reward), what can be checked without a GPU: the two entry points are declared, exported and bound; the five new
kernel families exist for the four quadrotor kinds with the members stated here, use no scratch and stay within the budgets of the
frame-skip kernels they are cut from (`make asm`); their names match no pre-existing family prefix; and the reward is a dozen
instructions, not a second copy of the dynamics."""
import pytest

import buildinfo as B
from test_frame_skip_build import SKIP

NEW = {"rmav_set_reward": ("int", 2), "rmav_get_reward": ("int", 3)}
# family prefix -> members: k_step_rw<K, TL>; k_rollout_rw<K, MODE in (buffer, random, controller), ST in (default, write-through, stream),
# TL>; the three policy families <K, BOOT>
REWARD = {"_ZN4rmav9k_step_rwILi": 4 * 2, "_ZN4rmav12k_rollout_rwILi": 4 * 3 * 3 * 2, "_ZN4rmav16k_rollout_nrm_rwILi": 4 * 2,
          "_ZN4rmav17k_rollout_pair_rwILi": 4 * 2, "_ZN4rmav24k_rollout_pair_shared_rwILi": 4 * 2}


def reward_family(prefix):
    h = B.hits(prefix)
    assert len(h) == REWARD[prefix], (prefix, sorted(h))
    return h


def test_reward_entry_points_are_declared_exported_and_bound(built):
    A, _ = B.assert_entry_points(NEW)
    import ctypes as C

    assert C.sizeof(A.RewardSpec) == 48 and A.RewardSpec.act_ref.offset == 28 and A.RewardSpec.terminal.offset == 44


@pytest.mark.parametrize("prefix", sorted(REWARD))
def test_every_new_family_exists_for_every_kind_and_is_clean(prefix):
    h = reward_family(prefix)
    for kind in range(4):
        mine = [n for n in h if n.startswith(f"{prefix}{kind}E")]
        assert len(mine) == REWARD[prefix] // 4, (prefix, kind, mine)
    for n, u in h.items():
        assert B.clean(u), (n, u)
        assert "RewardArgs" in n, n   # RewardArgs by value, or PolicyRewardArgs with the pointer to the handle's copy


def test_no_new_name_matches_an_older_prefix():
    seen = {**B.family(*B.FAMILIES)}
    for p in SKIP:
        h = B.hits(p)
        assert len(h) == SKIP[p], (p, sorted(h))
        seen.update(h)
    new = {}
    for p in REWARD:
        new.update(reward_family(p))
    assert len(new) == 104 and not set(new) & set(seen)
    assert {n for n in B.bodies("rmav_reward_abi") if "k_step_rw" in n or "k_rollout_rw" in n} == \
        set(reward_family("_ZN4rmav9k_step_rwILi")) | set(reward_family("_ZN4rmav12k_rollout_rwILi"))


def test_single_step_kernel_of_quadrotor3d_stays_at_full_occupancy():
    hits = B.hits("_ZN4rmav9k_step_rwILi2E")
    assert len(hits) == 2, sorted(hits)
    for n, u in hits.items():
        assert u["vgpr"] <= 48 and u["occ"] == 8, (n, u)


# (kind, register budget of test_fused_frame_skip_kernels = the ranged budget + 4, its minimum occupancy)
@pytest.mark.parametrize("kind,skip_budget,min_occ", [(0, 76, 6), (1, 120, 4), (2, 84, 6), (3, 148, 3)])
def test_fused_reward_kernels(kind, skip_budget, min_occ):
    """k_rollout_rw<K, MODE, ST, TL>: the caller- and random-action kernels stay within the budgets of the frame-skip kernels
    (test_frame_skip_build.py::test_fused_frame_skip_kernels) + 4 registers at their minimum occupancy.  Observed increase over
    k_rollout_fs: +1 (quadrotor2d: 72 -> 73), +0 .. 1 (quadrotor2d-slungload: 113 / 116 / 117 -> 114 / 116 / 117), +2 .. 3 (quadrotor3d:
    70 / 71 -> 72 / 74), +0 .. 1 (quadrotor3d-slungload).

    quadrotor2d is the one occupancy written from observation, 6 where the frame-skip kernel has 7: k_rollout_fs<quadrotor2d> sits AT
    72 registers, the last count that gives seven wavefronts per SIMD, so its own budget of +4 already costs the seventh.  The extra
    register is not the action cost (computed in front of the loop; a constant in its place leaves 73) and no scalar turned vector
    (the spec stays in scalar registers): it is the transients of d = |P - goal| beside the two norms the step itself keeps for `done`.
    Reworks tried and measured in `make asm`: the action cost inside the loop (73), the live reward under the not-terminated predicate
    (73), a vector copy of `alive` pinned inside the loop (74), amdgpu_waves_per_eu(7) (72 registers, but 2 of them spilled to
    scratch).  profiles/r17/reward.md has the table."""
    for mode in (0, 1, 2):
        hits = B.hits(f"_ZN4rmav12k_rollout_rwILi{kind}ELi{mode}E")
        assert len(hits) == 6, (kind, mode, sorted(hits))
        for n, u in hits.items():
            assert B.clean(u), (n, u)
            if mode != 2:
                assert u["vgpr"] <= skip_budget + 4 and u["occ"] >= min_occ, (n, u)


def test_policy_reward_kernels():
    """k_rollout_nrm_rw, k_rollout_pair_rw, k_rollout_pair_shared_rw <K, BOOT>: no scratch; at most 256 registers; the pair actors at two
    wavefronts per SIMD or more; no LDS permutes and no compiler-packed fp32 in the matrix-core kernels."""
    one = reward_family("_ZN4rmav16k_rollout_nrm_rwILi")
    pairs = {**reward_family("_ZN4rmav17k_rollout_pair_rwILi"), **reward_family("_ZN4rmav24k_rollout_pair_shared_rwILi")}
    for n, u in {**one, **pairs}.items():
        assert B.clean(u) and u["vgpr"] + u["agpr"] <= 256, (n, u)
    for n, u in pairs.items():
        assert u["occ"] >= 2, (n, u)
    B.assert_matrix_core_clean(r"_ZN4rmav(16k_rollout_nrm_rw|17k_rollout_pair_rw|24k_rollout_pair_shared_rw)ILi", 24)


def test_the_reward_is_a_dozen_instructions():
    """k_rollout_rw<K, random, default, no limit> against its k_rollout_fs counterpart: at most 1.15 x the instructions."""
    rw, fs = B.bodies("rmav_reward_abi"), B.bodies("rmav_skip_abi")
    count = lambda body: sum(1 for ln in body.split("\n") if ln.startswith("\t") and not ln.startswith("\t."))
    for kind in range(4):
        r = next(b for n, b in rw.items() if n.startswith(f"_ZN4rmav12k_rollout_rwILi{kind}ELi1ELi0ELb0E"))
        f = next(b for n, b in fs.items() if n.startswith(f"_ZN4rmav12k_rollout_fsILi{kind}ELi1ELi0ELb0E"))
        assert count(r) <= 1.15 * count(f), (kind, count(r), count(f))

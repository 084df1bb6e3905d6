"""The shared-trunk fused learner (rmav_ppo_grad_shared), what can be checked without a GPU: the three entry points are declared,
exported and bound, and their sizes are the documented ones; its one kernel exists in rmav_ppo_abi's listing, uses no scratch, spills
neither vector nor scalar registers, runs its products on the vector ALU from LDS and keeps two workgroups per CU; its header is
included by rmav_ppo_abi.hip alone."""
import buildinfo as B
from test_termination_build import MATRIX_CORE_BAD

NEW = {"rmav_ppo_grad_shared_param_count": ("int64_t", 1), "rmav_ppo_grad_shared_workspace_bytes": ("int64_t", 2),
       "rmav_ppo_grad_shared": ("int", 18)}
TRUNK = "_ZN4rmav12k_trunk_gradENS_9TrunkArgsE"


def test_shared_learner_entry_points_are_declared_exported_and_bound(built):
    A, L = B.assert_entry_points(NEW)
    lib = A.lib()
    for kind, (nS, nA) in enumerate(((5, 2), (9, 2), (10, 4), (16, 4), (13, 4))):
        count = 64 * nS + 64 + 4096 + 64 + 64 * nA + nA + 64 + 1 + nA
        assert lib.rmav_ppo_grad_shared_param_count(kind) == count
        # per-workgroup partial records (the gradient + 4 statistics words), one workgroup per 64-sample tile up to 512
        per = 4 * (count + 4)
        got = [lib.rmav_ppo_grad_shared_workspace_bytes(kind, b) for b in (1, 64, 65, 2125, 70001, 1 << 20)]
        assert got == [per, per, 2 * per, 34 * per, 512 * per, 512 * per]
    assert lib.rmav_ppo_grad_shared_param_count(5) == -1 and lib.rmav_ppo_grad_shared_param_count(-1) == -1
    assert lib.rmav_ppo_grad_shared_workspace_bytes(5, 64) == -1 and lib.rmav_ppo_grad_shared_workspace_bytes(2, 0) == -1
    assert lib.rmav_ppo_grad_shared_workspace_bytes(2, -3) == -1
    import gym_reinmav_amd as g

    assert callable(g.BatchedQuadrotor.ppo_grad_shared)


def test_trunk_kernel_is_clean():
    """(observed: 190 registers, 104 scalar registers, 80 432 bytes of LDS; two wavefronts per SIMD allow 256 registers)"""
    bodies = B.bodies("rmav_ppo_abi")
    mine = {n for n in B.usage() if "k_trunk" in n}
    assert mine == {TRUNK}, sorted(mine)
    assert "k_learner" not in TRUNK
    u, body = B.usage()[TRUNK], bodies[TRUNK]
    assert B.clean(u) and u["sspill"] == 0 and u["agpr"] == 0, u
    assert "atomic" not in body   # sums go through the workspace and the fold, in a fixed order
    for bad in MATRIX_CORE_BAD:
        assert bad not in body, bad
    # the products run on the vector ALU from LDS: 16-byte LDS reads feeding v_fma_f32, no matrix instruction
    assert "ds_read_b128" in body and "v_fma_f32" in body and "v_mfma" not in body
    assert 64 * 1024 < u["lds"] <= 80 * 1024 and u["occ"] == 2, u
    assert 128 < u["vgpr"] <= 256, u


def test_the_header_has_one_user():
    csrc = B.os.path.join(B.PKG, "csrc")
    assert B.os.path.exists(B.os.path.join(csrc, "rmav_learner_shared.hpp"))
    users = [f for f in B.os.listdir(csrc) if '#include "rmav_learner_shared.hpp"' in open(B.os.path.join(csrc, f)).read()]
    assert users == ["rmav_ppo_abi.hip"], users

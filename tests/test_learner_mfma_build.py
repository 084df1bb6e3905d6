"""The shared-trunk learner on the fp32 matrix cores (rmav_ppo_grad_shared_mfma), what can be checked without a GPU: the two entry
points are declared, exported and bound, and the workspace has the documented size; its one kernel exists in rmav_ppo_abi's listing,
uses no scratch, spills neither vector nor scalar registers, runs its products on v_mfma_f32_32x32x2_f32 without atomics, LDS permutes
or compiler packed-fp32 forms, and keeps one workgroup per CU; its header is included by rmav_ppo_abi.hip alone."""
import buildinfo as B
from test_termination_build import MATRIX_CORE_BAD

NEW = {"rmav_ppo_grad_shared_mfma_workspace_bytes": ("int64_t", 2), "rmav_ppo_grad_shared_mfma": ("int", 18)}
MATRIX = "_ZN4rmav13k_matrix_gradENS_9TrunkArgsE"


def test_matrix_learner_entry_points_are_declared_exported_and_bound(built):
    A, L = B.assert_entry_points(NEW)
    lib = A.lib()
    for kind in range(5):
        count = lib.rmav_ppo_grad_shared_param_count(kind)
        # per-workgroup partial records (the gradient + 4 statistics words), one workgroup per 128-sample step up to 256
        per = 4 * (count + 4)
        got = [lib.rmav_ppo_grad_shared_mfma_workspace_bytes(kind, b) for b in (1, 128, 129, 2125, 32768, 32769, 1 << 20)]
        assert got == [per, per, 2 * per, 17 * per, 256 * per, 256 * per, 256 * per]
    assert lib.rmav_ppo_grad_shared_mfma_workspace_bytes(5, 64) == -1 and lib.rmav_ppo_grad_shared_mfma_workspace_bytes(-1, 64) == -1
    assert lib.rmav_ppo_grad_shared_mfma_workspace_bytes(2, 0) == -1 and lib.rmav_ppo_grad_shared_mfma_workspace_bytes(2, -3) == -1
    import gym_reinmav_amd as g

    assert callable(g.BatchedQuadrotor.ppo_grad_shared_mfma)


def test_matrix_kernel_is_clean():
    """(observed: 256 registers + 78 accumulation registers, 106 scalar registers, 124 544 bytes of LDS; one wavefront per SIMD allows
    512 registers)"""
    bodies = B.bodies("rmav_ppo_abi")
    mine = {n for n in B.usage() if "k_matrix" in n}
    assert mine == {MATRIX}, sorted(mine)
    for family in ("k_learner", "k_trunk", "k_adv_moments", "k_ppo_adam"):   # (the censuses of the other learner-side build tests)
        assert family not in MATRIX
    u, body = B.usage()[MATRIX], bodies[MATRIX]
    assert B.clean(u) and u["sspill"] == 0, u
    assert "atomic" not in body   # sums go through LDS, the workspace and the fold, in a fixed order
    for bad in MATRIX_CORE_BAD:
        assert bad not in body, bad
    # every product on the fp32-input matrix instruction: 16 + 64 forward, 64 delta 1, 64 + 32 + 32 weight gradients
    assert body.count("v_mfma_f32_32x32x2") == 272
    assert "v_permlane32_swap" in body and "ds_read_b128" in body
    assert 80 * 1024 < u["lds"] <= 160 * 1024 and u["occ"] == 1, u
    assert u["vgpr"] + u["agpr"] <= 512, u


def test_the_header_has_one_user():
    csrc = B.os.path.join(B.PKG, "csrc")
    assert B.os.path.exists(B.os.path.join(csrc, "rmav_learner_mfma.hpp"))
    users = [f for f in B.os.listdir(csrc) if '#include "rmav_learner_mfma.hpp"' in open(B.os.path.join(csrc, f)).read()]
    assert users == ["rmav_ppo_abi.hip"], users

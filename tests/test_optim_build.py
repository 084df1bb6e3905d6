"""The launches around the fused learner (rmav_adv_moments, rmav_ppo_adam; csrc/rmav_optim.hpp), what can be checked without a GPU:
the three entry points are declared, exported and bound with their argument counts; the workspace size is the documented function of
the batch; the three kernels exist in rmav_ppo_abi's listing, use no scratch and spill neither vector nor scalar registers; the header
is included by rmav_ppo_abi.hip alone."""
import ctypes as C

import buildinfo as B

NEW = {"rmav_adv_moments_workspace_bytes": ("int64_t", 1), "rmav_adv_moments": ("int", 6), "rmav_ppo_adam": ("int", 9)}
KERNELS = {"k_adv_moments": "_ZN4rmav13k_adv_momentsEPKlPKflPNS_6MomentE", "k_adv_moments_fold": "_ZN4rmav18k_adv_moments_foldEPKNS_6MomentEilPf",
           "k_ppo_adam": "_ZN4rmav10k_ppo_adamENS_8AdamArgsE"}


def test_entry_points_are_declared_exported_and_bound(built):
    A, L = B.assert_entry_points(NEW)
    lib = A.lib()
    # one 24-byte moment per workgroup, one workgroup per 256 samples up to 128
    got = [lib.rmav_adv_moments_workspace_bytes(b) for b in (1, 256, 257, 2125, 32768, 32769, 33025, 1 << 20, 1 << 40)]
    assert got == [24, 24, 48, 9 * 24, 128 * 24, 128 * 24, 128 * 24, 128 * 24, 128 * 24]
    assert lib.rmav_adv_moments_workspace_bytes(0) == -1 and lib.rmav_adv_moments_workspace_bytes(-7) == -1
    assert C.sizeof(A.PpoAdamSpec) == 32 and [f[0] for f in A.PpoAdamSpec._fields_] == ["lr", "beta1", "beta2", "eps", "max_grad_norm",
                                                                                      "grad_scale", "_reserved"]
    assert lib.rmav_version() == 101
    import gym_reinmav_amd as g

    assert callable(g.BatchedQuadrotor.adv_moments) and callable(g.BatchedQuadrotor.ppo_adam)


def test_the_three_kernels_are_clean():
    """(observed: k_adv_moments 30 registers, k_adv_moments_fold 30, k_ppo_adam 54 registers and 64 scalar registers, 128 bytes of LDS)"""
    usage, bodies = B.usage(), B.bodies("rmav_ppo_abi")
    mine = {n for n in usage if "k_adv_moments" in n or "k_ppo_adam" in n}
    assert mine == set(KERNELS.values()), sorted(mine)
    for name in KERNELS.values():
        assert "k_learner" not in name and "k_trunk" not in name
        u = usage[name]
        assert name in bodies
        assert B.clean(u) and u["sspill"] == 0 and u["agpr"] == 0, (name, u)
    assert usage[KERNELS["k_ppo_adam"]]["vgpr"] <= 128   # 1024 threads: four wavefronts per SIMD


def test_the_header_has_one_user():
    csrc = B.os.path.join(B.PKG, "csrc")
    assert B.os.path.exists(B.os.path.join(csrc, "rmav_optim.hpp"))
    users = [f for f in B.os.listdir(csrc) if '#include "rmav_optim.hpp"' in open(B.os.path.join(csrc, f)).read()]
    assert users == ["rmav_ppo_abi.hip"], users

"""The fused learner (rmav_ppo_grad), what can be checked without a GPU: the three entry points are declared, exported and bound; its
kernels exist in rmav_ppo_abi's listing, use no scratch, spill neither vector nor scalar registers and contain none of the instruction
forms buildinfo.assert_matrix_core_clean keeps out; registers, LDS and occupancy are what was observed (profiles/r23/learner.md); the
Makefile still lists sixteen units and the GAE kernels of the same unit are still there."""
import ctypes as C
import re

import buildinfo as B
from test_termination_build import MATRIX_CORE_BAD

NEW = {"rmav_ppo_grad_param_count": ("int64_t", 1), "rmav_ppo_grad_workspace_bytes": ("int64_t", 2), "rmav_ppo_grad": ("int", 18)}
GRAD = ("_ZN4rmav14k_learner_gradILb0EEEvNS_11LearnerArgsE", "_ZN4rmav14k_learner_gradILb1EEEvNS_11LearnerArgsE")   # policy net, value net
FOLD = "_ZN4rmav14k_learner_foldEPKfiiiiiiffS1_PfS2_"


def test_learner_entry_points_are_declared_exported_and_bound(built):
    A, L = B.assert_entry_points(NEW)
    S = A.PpoGradSpec
    assert C.sizeof(S) == 16 and (S.clip.offset, S.vf_coef.offset, S.ent_coef.offset, S._reserved.offset) == (0, 4, 8, 12)
    # the flat gradient's size for the five kinds: 2 (64 nS + 64 + 4096 + 64) + (64 nA + nA) + (64 + 1) + nA
    lib = A.lib()
    for kind, (nS, nA) in enumerate(((5, 2), (9, 2), (10, 4), (16, 4), (13, 4))):
        assert lib.rmav_ppo_grad_param_count(kind) == 2 * (64 * nS + 64 + 4096 + 64) + 65 * nA + 65 + nA
        # per-workgroup partial records (the gradient + 4 statistics words), one workgroup per 64-sample tile up to 512
        per = 4 * (lib.rmav_ppo_grad_param_count(kind) + 4)
        assert [lib.rmav_ppo_grad_workspace_bytes(kind, b) for b in (1, 64, 65, 2125, 70001, 1 << 20)] == [per, per, 2 * per, 34 * per, 512 * per, 512 * per]
    assert lib.rmav_ppo_grad_param_count(5) == -1 and lib.rmav_ppo_grad_workspace_bytes(2, 0) == -1
    # RMAV_VERSION, the tuning keys and the set of public headers are what they were
    assert lib.rmav_version() == 101 and len(A.TUNE) == 9
    assert sorted(B.os.listdir(B.os.path.join(B.ROOT, "include"))) == ["rmav.h", "rmav_comm.h", "rmav_ppo.h"]
    import gym_reinmav_amd as g

    assert callable(g.BatchedQuadrotor.ppo_grad)


def test_learner_kernels_are_clean():
    bodies = B.bodies("rmav_ppo_abi")
    mine = {n for n in B.usage() if "k_learner" in n}
    assert mine == set(GRAD) | {FOLD}, sorted(mine)
    for n in mine:
        u = B.usage()[n]
        assert B.clean(u) and u["sspill"] == 0 and u["agpr"] == 0, (n, u)
        assert n in bodies, n
        for bad in MATRIX_CORE_BAD:
            assert bad not in bodies[n], (n, bad)
        assert "atomic" not in bodies[n], n   # sums go through the workspace and a fold, in a fixed order
    for n in GRAD:   # the products run on the vector ALU from LDS: 16-byte LDS reads feeding v_fma_f32, no matrix instruction
        assert "ds_read_b128" in bodies[n] and "v_fma_f32" in bodies[n] and "v_mfma" not in bodies[n], n


def test_learner_resources_are_as_observed():
    """(observed: 160 / 162 registers, 79 648 bytes of LDS - two workgroups per CU, two wavefronts per SIMD)"""
    for n in GRAD:
        u = B.usage()[n]
        assert 128 < u["vgpr"] <= 168 and u["occ"] == 2, (n, u)
        assert 64 * 1024 < u["lds"] <= 80 * 1024, (n, u)
    u = B.usage()[FOLD]
    assert u["vgpr"] <= 32 and u["occ"] == 8 and 0 < u["lds"] <= 4096, u


def test_the_unit_lists_and_the_gae_kernels_are_what_they_were():
    mk = open(B.os.path.join(B.PKG, "Makefile")).read()
    units = re.search(r"^ABI_UNITS\s*:=(.*)$", mk, re.M).group(1).split() + re.search(r"^POLICY_UNITS\s*:=(.*)$", mk, re.M).group(1).split()
    assert len(units) == 16 and "rmav_ppo_abi" in units
    names = set(B.bodies("rmav_ppo_abi"))
    for k in ("_ZN4rmav5k_gaeE", "_ZN4rmav10k_gae_bootE", "_ZN4rmav10k_gae_normILb0EE", "_ZN4rmav10k_gae_normILb1EE", "_ZN4rmav10k_gae_foldE"):
        assert any(n.startswith(k) for n in names), k
    # the kernels live in a header only this unit includes
    csrc = B.os.path.join(B.PKG, "csrc")
    users = [f for f in B.os.listdir(csrc) if '#include "rmav_learner.hpp"' in open(B.os.path.join(csrc, f)).read()]
    assert users == ["rmav_ppo_abi.hip"], users

"""Observation normalisation, what can be checked without a GPU: the new entry points are declared, exported and bound, and the new
kernels exist with the resource budgets of the kernels they stand beside (`make asm`, as test_bootstrap_build.py)."""
import ctypes as C

import buildinfo as B

NEW = {"rmav_obs_norm_bytes": ("int64_t", 0), "rmav_obs_norm_init": ("int", 5), "rmav_obs_moments": ("int", 6),
       "rmav_obs_norm_merge": ("int", 4), "rmav_obs_normalize": ("int", 7), "rmav_rollout_policy_norm": ("int", 13)}


def test_obs_norm_entry_points_are_declared_exported_and_bound(built):
    A, L = B.assert_entry_points(NEW)
    L.rmav_obs_norm_bytes.restype = C.c_int64
    from gym_reinmav_amd import obs_norm

    assert L.rmav_obs_norm_bytes() == obs_norm.N_BYTES == 432
    assert L.rmav_version() == 101 and len(A.TUNE) == 9   # additive: neither moved


def test_normalised_rollout_kernels():
    """k_rollout_nrm<K, BOOT>, k_rollout_pair_nrm<K, BOOT>, k_rollout_pair_shared_nrm<K, BOOT>, K = 0..3: 24 kernels, no scratch, no
    spills, VGPR + AGPR <= 256, the pair kernels two wavefronts per SIMD - the budgets of the kernels they stand beside
    (test_resource_usage.py, test_bootstrap_build.py)."""
    fam = (("_ZN4rmav13k_rollout_nrmILi{k}ELb{b}E", 1), ("_ZN4rmav18k_rollout_pair_nrmILi{k}ELb{b}E", 2),
           ("_ZN4rmav25k_rollout_pair_shared_nrmILi{k}ELb{b}E", 2))
    seen = 0
    for pat, min_occ in fam:
        for k in range(4):
            for b in (0, 1):
                h = B.hits(pat.format(k=k, b=b))
                assert len(h) == 1, (pat, k, b, sorted(h))
                n, u = next(iter(h.items()))
                assert B.clean(u), (n, u)
                assert u["vgpr"] + u["agpr"] <= 256 and u["occ"] >= min_occ, (n, u)
                seen += 1
    assert seen == 24
    assert len(B.hits("_ZN4rmav13k_rollout_nrmI")) + len(B.hits("_ZN4rmav18k_rollout_pair_nrmI")) + \
        len(B.hits("_ZN4rmav25k_rollout_pair_shared_nrmI")) == 24, "no REINMAV instantiation, no third variant"
    # the matrix-core kernels keep the LDS permutes and compiler-packed fp32 out (the rule their siblings are held to)
    for name, body in B.assert_matrix_core_clean(r"_ZN4rmav(13k_rollout_nrm|18k_rollout_pair_nrm|25k_rollout_pair_shared_nrm)I", 24).items():
        assert "v_med3_f32" in body and "v_max_f32" not in body and "v_min_f32" not in body, name   # the clamp is one instruction
        # (the one-wavefront kernel calls its fp32-MFMA net, mlp_mfma32, as a function: its own body has no v_mfma)
        assert ("v_mfma" in body) == ("k_rollout_nrmI" not in name), name


def test_statistics_kernels():
    """k_obs_moments (both load widths), its fold, the merge and the elementwise pass: no scratch, no spills"""
    for prefix, count in (("_ZN4rmav13k_obs_momentsILb", 2), ("_ZN4rmav18k_obs_moments_foldE", 1), ("_ZN4rmav16k_obs_norm_mergeE", 1),
                          ("_ZN4rmav15k_obs_norm_initE", 1), ("_ZN4rmav15k_obs_normalizeE", 1)):
        h = B.hits(prefix)
        assert len(h) == count, (prefix, sorted(h))
        for n, u in h.items():
            assert B.clean(u), (n, u)

"""Return normalisation, what can be checked without a GPU: the new entry points are declared, exported and bound, and the new
kernels exist, once each, without scratch or spills (`make asm`, as test_obs_norm_build.py); k_gae / k_gae_boot keep their names."""
import ctypes as C

import buildinfo as B

NEW = {"rmav_ret_norm_bytes": ("int64_t", 0), "rmav_ret_norm_init": ("int", 5), "rmav_ret_moments": ("int", 8),
       "rmav_ret_norm_merge": ("int", 4), "rmav_ret_normalize": ("int", 6), "rmav_gae_norm": ("int", 13)}


def test_ret_norm_entry_points_are_declared_exported_and_bound(built):
    A, L = B.assert_entry_points(NEW)
    L.rmav_ret_norm_bytes.restype = C.c_int64
    from gym_reinmav_amd import ret_norm

    assert L.rmav_ret_norm_bytes() == ret_norm.N_BYTES == 64
    assert L.rmav_version() == 101 and len(A.TUNE) == 9   # additive: neither moved


def test_ret_norm_kernels():
    """every new kernel exactly once (k_gae_norm<BOOT> twice), no scratch, no spills; the pinned GAE kernels are still there"""
    for prefix, count in (("_ZN4rmav13k_ret_momentsE", 1), ("_ZN4rmav18k_ret_moments_foldE", 1), ("_ZN4rmav15k_ret_norm_initE", 1),
                          ("_ZN4rmav16k_ret_norm_mergeE", 1), ("_ZN4rmav15k_ret_normalizeE", 1), ("_ZN4rmav10k_gae_normILb", 2)):
        h = B.hits(prefix)
        assert len(h) == count, (prefix, sorted(h))
        for n, u in h.items():
            assert B.clean(u) and u["sspill"] == 0, (n, u)
    assert {n[:24] for n in B.hits("_ZN4rmav10k_gae_normILb")} == {"_ZN4rmav10k_gae_normILb0", "_ZN4rmav10k_gae_normILb1"}
    assert len(B.hits("_ZN4rmav5k_gaeE")) == 1 and len(B.hits("_ZN4rmav10k_gae_bootE")) == 1


def test_gae_norm_clamp_is_one_instruction():
    bodies = B.bodies("rmav_ppo_abi")
    seen = 0
    for name, body in bodies.items():
        if not name.startswith("_ZN4rmav10k_gae_normILb"):
            continue
        seen += 1
        assert "v_med3_f32" in body and "v_max_f32" not in body and "v_min_f32" not in body, name
        for bad in ("scratch_", "v_pk_mul_f32", "v_pk_fma_f32"):   # (the block reduction's shuffles are the only cross-lane traffic)
            assert bad not in body, (name, bad)
    assert seen == 2
    txt = B.listing("rmav_ppo_abi")
    assert "_ZN4rmav5k_gaeE" in txt and "_ZN4rmav10k_gae_bootE" in txt

"""Return normalisation, what can be checked without a GPU: the new entry points are declared, exported and bound, and the new
kernels exist, once each, without scratch or spills (`make asm`, as test_obs_norm_build.py); k_gae / k_gae_boot keep their names."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "reinmav-gym_amd")
NEW = {"rmav_ret_norm_bytes": ("int64_t", 0), "rmav_ret_norm_init": ("int", 5), "rmav_ret_moments": ("int", 8),
       "rmav_ret_norm_merge": ("int", 4), "rmav_ret_normalize": ("int", 6), "rmav_gae_norm": ("int", 13)}


def test_ret_norm_entry_points_are_declared_exported_and_bound(built):
    from gym_reinmav_amd import _abi as A

    inc = os.path.join(ROOT, "include")
    txt = "".join(open(os.path.join(inc, f)).read() for f in sorted(os.listdir(inc)) if f.endswith(".h"))
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = C.CDLL(A.LIB_PATH)
    for name, (ret, nargs) in NEW.items():
        m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^)]*)\)", txt)
        assert m, name
        declared = 0 if m.group(1).strip() == "void" else len(m.group(1).split(","))
        assert declared == nargs, (name, declared)
        assert hasattr(L, name), name
        assert name in A.PROTOTYPES, name
        assert len(A.PROTOTYPES[name][1]) == nargs, name
    L.rmav_ret_norm_bytes.restype = C.c_int64
    from gym_reinmav_amd import ret_norm

    assert L.rmav_ret_norm_bytes() == ret_norm.N_BYTES == 64
    assert L.rmav_version() == 101 and len(A.TUNE) == 9   # additive: neither moved


@pytest.fixture(scope="module")
def usage():
    subprocess.run(["make", "-s", "-C", PKG, "asm"], check=True)
    txt = open(os.path.join(PKG, "build", "resource_usage.txt")).read()
    out = {}
    for b in re.split(r"remark: Function Name: ", txt)[1:]:
        name = b.split(" ")[0]
        out[name] = {k: int(re.search(pat, b).group(1)) for k, pat in (
            ("vgpr", r"VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"),
            ("sspill", r"SGPRs Spill: (\d+)"))}
    return out


def test_ret_norm_kernels(usage):
    """every new kernel exactly once (k_gae_norm<BOOT> twice), no scratch, no spills; the pinned GAE kernels are still there"""
    for prefix, count in (("_ZN4rmav13k_ret_momentsE", 1), ("_ZN4rmav18k_ret_moments_foldE", 1), ("_ZN4rmav15k_ret_norm_initE", 1),
                          ("_ZN4rmav16k_ret_norm_mergeE", 1), ("_ZN4rmav15k_ret_normalizeE", 1), ("_ZN4rmav10k_gae_normILb", 2)):
        h = {n: v for n, v in usage.items() if n.startswith(prefix)}
        assert len(h) == count, (prefix, sorted(h))
        for n, u in h.items():
            assert u["scratch"] == 0 and u["spill"] == 0 and u["sspill"] == 0, (n, u)
    assert {n[:24] for n in usage if n.startswith("_ZN4rmav10k_gae_normILb")} == {"_ZN4rmav10k_gae_normILb0", "_ZN4rmav10k_gae_normILb1"}
    assert len([n for n in usage if n.startswith("_ZN4rmav5k_gaeE")]) == 1
    assert len([n for n in usage if n.startswith("_ZN4rmav10k_gae_bootE")]) == 1


def test_gae_norm_clamp_is_one_instruction(usage):
    txt = open(os.path.join(PKG, "build", "rmav_abi.gfx950.s")).read()
    bodies = re.split(r"^(_ZN4rmav\w+):[^\n]*\n", txt, flags=re.M)
    seen = 0
    for name, body in zip(bodies[1::2], bodies[2::2]):
        if not name.startswith("_ZN4rmav10k_gae_normILb"):
            continue
        seen += 1
        body = body.split(".Lfunc_end")[0]
        assert "v_med3_f32" in body and "v_max_f32" not in body and "v_min_f32" not in body, name
        for bad in ("scratch_", "v_pk_mul_f32", "v_pk_fma_f32"):   # (the block reduction's shuffles are the only cross-lane traffic)
            assert bad not in body, (name, bad)
    assert seen == 2
    assert "_ZN4rmav5k_gaeE" in txt and "_ZN4rmav10k_gae_bootE" in txt

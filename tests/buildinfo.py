"""What the *_build tests and test_resource_usage.py read off a build without a GPU: the assembly listings and hipcc's
-Rpass-analysis=kernel-resource-usage remarks of `make asm`, the census of the kernel families, and the declared / exported / bound
check of the C entry points.  `make asm` recompiles every translation unit, so it runs once per process."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "reinmav-gym_amd")
UNITS = ("rmav_abi", "rmav_ppo_abi", "rmav_comm_abi", "rmav_policy_abi", "rmav_range_abi")   # = UNITS of the Makefile

# Every kernel family (prefix of the mangled name) and how many members the library has.  A new family is a new line here.
RANGED = {"_ZN4rmav9k_step_drILi": 16, "_ZN4rmav12k_rollout_drILi": 72, "_ZN4rmav16k_rollout_nrm_drILi": 8,   # (handles with a parameter range)
          "_ZN4rmav17k_rollout_pair_drILi": 8, "_ZN4rmav24k_rollout_pair_shared_drILi": 8, "_ZN4rmav12k_range_drawE": 1}
FAMILIES = {"_ZN4rmav6k_stepILi": 28, "_ZN4rmav10k_step_bigILi": 24, "_ZN4rmav9k_step_tlILi": 16, "_ZN4rmav12k_step_finalILi": 24,
            "_ZN4rmav9k_rolloutILi": 128, "_ZN4rmav12k_rollout_tlILi": 52, "_ZN4rmav14k_rollout_bootILi": 4, "_ZN4rmav13k_rollout_nrmILi": 8,
            "_ZN4rmav14k_rollout_pairILi": 10, "_ZN4rmav21k_rollout_pair_sharedILi": 5,
            "_ZN4rmav17k_rollout_pair_tlILi": 4, "_ZN4rmav24k_rollout_pair_shared_tlILi": 4,
            "_ZN4rmav19k_rollout_pair_bootILi": 4, "_ZN4rmav26k_rollout_pair_shared_bootILi": 4,
            "_ZN4rmav18k_rollout_pair_nrmILi": 8, "_ZN4rmav25k_rollout_pair_shared_nrmILi": 8, **RANGED}

_FIELDS = (("vgpr", r"VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
           ("spill", r"VGPRs Spill: (\d+)"), ("sspill", r"SGPRs Spill: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"),
           ("lds", r"LDS Size \[bytes/block\]: (\d+)"))
_cache = {}


def asm():
    """The build directory after `make asm` (<unit>.gfx950.s and resource_usage.txt)."""
    if "asm" not in _cache:
        subprocess.run(["make", "-s", "-C", PKG, "asm"], check=True)
        _cache["asm"] = os.path.join(PKG, "build")
    return _cache["asm"]


def usage():
    """{mangled kernel name: {vgpr, agpr, scratch, spill, sspill, occ, lds}} of every kernel of the library."""
    if "usage" not in _cache:
        txt = open(os.path.join(asm(), "resource_usage.txt")).read()
        out = {}
        for b in re.split(r"remark: Function Name: ", txt)[1:]:
            out[b.split(" ")[0]] = {k: int(re.search(pat, b).group(1)) for k, pat in _FIELDS}
        assert len(out) >= 100
        _cache["usage"] = out
    return _cache["usage"]


def hits(prefix):
    return {n: v for n, v in usage().items() if n.startswith(prefix)}


def family(*prefixes):
    """The kernels of these families, which have the members the census says."""
    out = {}
    for p in prefixes:
        h = hits(p)
        assert len(h) == FAMILIES[p], (p, sorted(h))
        out.update(h)
    return out


def clean(u):
    return u["scratch"] == 0 and u["spill"] == 0


def listing(unit):
    return open(os.path.join(asm(), unit + ".gfx950.s")).read()


def bodies(unit):
    """{symbol: its body up to .Lfunc_end} of a translation unit's listing."""
    if ("bodies", unit) not in _cache:
        parts = re.split(r"^(_ZN4rmav\w+):[^\n]*\n", listing(unit), flags=re.M)   # [pre, name, body, name, body, ...]
        _cache["bodies", unit] = {name: body.split(".Lfunc_end")[0] for name, body in zip(parts[1::2], parts[2::2])}
    return _cache["bodies", unit]


def assert_matrix_core_clean(name_regex, expected_count):
    """The policy kernels whose names match: lanes are exchanged with v_permlane32_swap, never through LDS permutes, and the compiler-only
    packed-fp32 forms stay out.  -> {name: body} of the kernels looked at."""
    seen = {n: b for n, b in bodies("rmav_policy_abi").items() if re.match(name_regex, n)}
    for name, body in seen.items():
        for bad in ("ds_bpermute", "ds_permute", "v_pk_mul_f32", "v_pk_mov_b32"):
            assert bad not in body, (name, bad)
    assert len(seen) == expected_count, len(seen)
    return seen


def assert_entry_points(spec):
    """spec {name: (return type, argument count or None)}: declared in include/*.h (with that many arguments), exported by the library
    and bound in _abi.PROTOTYPES (with that many arguments)."""
    from gym_reinmav_amd import _abi as A

    inc = os.path.join(ROOT, "include")
    txt = "".join(open(os.path.join(inc, f)).read() for f in sorted(os.listdir(inc)) if f.endswith(".h"))
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = C.CDLL(A.LIB_PATH)
    for name, (ret, nargs) in spec.items():
        m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^)]*)\)", txt)
        assert m, name
        assert hasattr(L, name), name
        assert name in A.PROTOTYPES, name
        if nargs is not None:
            declared = 0 if m.group(1).strip() == "void" else len(m.group(1).split(","))
            assert declared == nargs, (name, declared)
            assert len(A.PROTOTYPES[name][1]) == nargs, name
    return A, L

"""Episode time limits, what can be checked without a GPU: the three entry points are declared, exported and bound, and the
time-limited kernels exist with the resource budgets of the kernels they stand beside (`make asm`, as test_resource_usage.py)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "reinmav-gym_amd")
NEW = ("rmav_set_time_limit", "rmav_get_time_limit", "rmav_episode_truncated")


def test_time_limit_entry_points_are_declared_exported_and_bound(built):
    from gym_reinmav_amd import _abi as A

    inc = os.path.join(ROOT, "include")
    txt = "".join(open(os.path.join(inc, f)).read() for f in sorted(os.listdir(inc)) if f.endswith(".h"))
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = C.CDLL(A.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
        assert hasattr(L, name), name
        assert name in A.PROTOTYPES, name


@pytest.fixture(scope="module")
def usage():
    subprocess.run(["make", "-s", "-C", PKG, "asm"], check=True)
    txt = open(os.path.join(PKG, "build", "resource_usage.txt")).read()
    out = {}
    for b in re.split(r"remark: Function Name: ", txt)[1:]:
        name = b.split(" ")[0]
        out[name] = {k: int(re.search(pat, b).group(1)) for k, pat in (
            ("vgpr", r"VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
            ("spill", r"VGPRs Spill: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"))}
    return out


def _hits(usage, prefix):
    return {n: v for n, v in usage.items() if n.startswith(prefix)}


def _clean(u):
    return u["scratch"] == 0 and u["spill"] == 0


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_single_step_time_limit_kernels(usage, kind):
    for ctrl in (0, 1):
        hits = _hits(usage, f"_ZN4rmav9k_step_tlILi{kind}ELb{ctrl}E")
        assert hits, (kind, ctrl)
        for n, u in hits.items():
            assert _clean(u), (n, u)
    # the shipped store policy of the small batches: as small as k_step itself (test_single_step_kernel_is_small)
    u = next(iter(_hits(usage, "_ZN4rmav9k_step_tlILi2ELb0ELi0E").values()))
    assert u["vgpr"] <= 48 and u["occ"] == 8, u


@pytest.mark.parametrize("kind,budget,min_occ", [(0, 64, 7), (1, 104, 4), (2, 80, 6), (3, 144, 3)])
def test_fused_time_limit_kernels(usage, kind, budget, min_occ):
    """k_rollout_tl<K, MODE, ST> for ACT_BUFFER, ACT_RANDOM, ACT_CONTROLLER and ACT_POLICY_F32M: no scratch, no spills; the caller-
    and random-action kernels within the one-wavefront budgets of test_one_wavefront_rollout_register_budget."""
    for mode in (0, 1, 2, 8):
        hits = _hits(usage, f"_ZN4rmav12k_rollout_tlILi{kind}ELi{mode}E")
        assert hits, (kind, mode)
        for n, u in hits.items():
            assert _clean(u), (n, u)
    for mode, st in ((1, 2), (1, 0), (0, 0)):
        u = usage[next(iter(_hits(usage, f"_ZN4rmav12k_rollout_tlILi{kind}ELi{mode}ELi{st}E")))]
        assert u["vgpr"] <= budget and u["occ"] >= min_occ, (kind, mode, st, u)
    u = next(iter(_hits(usage, f"_ZN4rmav12k_rollout_tlILi{kind}ELi8ELi0E").values()))
    assert u["vgpr"] + u["agpr"] <= 256, u


def test_pair_time_limit_kernels(usage):
    """k_rollout_pair_tl<K, FMT_F16> and k_rollout_pair_shared_tl<K>, K = 0..3: two wavefronts per SIMD, no scratch."""
    hits = {**_hits(usage, "_ZN4rmav17k_rollout_pair_tlILi"), **_hits(usage, "_ZN4rmav24k_rollout_pair_shared_tlILi")}
    assert len(hits) == 8, sorted(hits)
    for n, u in hits.items():
        assert u["vgpr"] + u["agpr"] <= 256 and _clean(u) and u["occ"] >= 2, (n, u)
    # the time-limited matrix-core kernels keep the LDS permutes and compiler-packed fp32 out as well
    txt = open(os.path.join(PKG, "build", "rmav_policy_abi.gfx950.s")).read()
    bodies = re.split(r"^(_ZN4rmav\w+):[^\n]*\n", txt, flags=re.M)
    seen = 0
    for name, body in zip(bodies[1::2], bodies[2::2]):
        if not re.match(r"_ZN4rmav(17k_rollout_pair_tl|24k_rollout_pair_shared_tl|12k_rollout_tlILi\dELi8E)", name):
            continue
        seen += 1
        body = body.split(".Lfunc_end")[0]
        for bad in ("ds_bpermute", "ds_permute", "v_pk_mul_f32", "v_pk_mov_b32"):
            assert bad not in body, (name, bad)
    assert seen == 12, seen

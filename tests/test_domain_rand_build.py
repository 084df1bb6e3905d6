"""Per-episode domain randomisation, what can be checked without a GPU: the three entry points are declared, exported and bound, the
ranged kernels exist for K = 0..3 with the resource budgets of the kernels they stand beside (`make asm`, as test_time_limit_build.py),
and no pre-existing kernel family gained or lost a member."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "reinmav-gym_amd")
NEW = ("rmav_set_env_param_range", "rmav_get_env_param_range", "rmav_get_env_param")
UNITS = ("rmav_abi", "rmav_policy_abi", "rmav_range_abi")


def test_domain_rand_entry_points_are_declared_exported_and_bound(built):
    from gym_reinmav_amd import _abi as A

    inc = os.path.join(ROOT, "include")
    txt = "".join(open(os.path.join(inc, f)).read() for f in sorted(os.listdir(inc)) if f.endswith(".h"))
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = C.CDLL(A.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
        assert hasattr(L, name), name
        assert name in A.PROTOTYPES, name
    # the RNG table documents the stream
    assert "(4<<24)" in open(os.path.join(inc, "rmav.h")).read()


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
def test_single_step_ranged_kernels(usage, kind):
    """k_step_dr<K, CTRL, TL>: no scratch, no spills, and no bigger than the time-limited single-step kernel of the same kind plus the
    few registers of the draw (k_step_tl of quadrotor3d: <= 48 VGPRs at occupancy 8)."""
    hits = _hits(usage, f"_ZN4rmav9k_step_drILi{kind}E")
    assert len(hits) == 4, sorted(hits)
    for n, u in hits.items():
        assert _clean(u), (n, u)
    if kind == 2:
        u = next(iter(_hits(usage, "_ZN4rmav9k_step_drILi2ELb0ELb0E").values()))
        assert u["vgpr"] <= 48 and u["occ"] == 8, u


@pytest.mark.parametrize("kind,budget,min_occ", [(0, 72, 7), (1, 116, 4), (2, 80, 6), (3, 144, 3)])
def test_fused_ranged_kernels(usage, kind, budget, min_occ):
    """k_rollout_dr<K, MODE, ST, TL> for ACT_BUFFER, ACT_RANDOM, ACT_CONTROLLER, three store policies, with and without a time limit: no
    scratch, no spills; the caller- and random-action kernels at the occupancy of k_rollout_tl (test_time_limit_build.py) and within
    8 / 12 registers of its budgets for the two 2-D kinds (the redraw keeps three spare constants and the fp64 re-derivation live)."""
    for mode in (0, 1, 2):
        hits = _hits(usage, f"_ZN4rmav12k_rollout_drILi{kind}ELi{mode}E")
        assert len(hits) == 6, (kind, mode, sorted(hits))
        for n, u in hits.items():
            assert _clean(u), (n, u)
            if mode != 2:
                assert u["vgpr"] <= budget and u["occ"] >= min_occ, (n, u)


def test_policy_ranged_kernels(usage):
    """k_rollout_nrm_dr<K, BOOT>, k_rollout_pair_dr<K, BOOT> and k_rollout_pair_shared_dr<K, BOOT>, K = 0..3: no scratch; the pair actors
    within 256 registers at two wavefronts per SIMD; the matrix-core kernels free of LDS permutes and compiler-packed fp32."""
    one = _hits(usage, "_ZN4rmav16k_rollout_nrm_drILi")
    pairs = {**_hits(usage, "_ZN4rmav17k_rollout_pair_drILi"), **_hits(usage, "_ZN4rmav24k_rollout_pair_shared_drILi")}
    assert len(one) == 8 and len(pairs) == 16, (sorted(one), sorted(pairs))
    for n, u in one.items():
        assert _clean(u) and u["vgpr"] + u["agpr"] <= 256, (n, u)
    for n, u in pairs.items():
        assert u["vgpr"] + u["agpr"] <= 256 and _clean(u) and u["occ"] >= 2, (n, u)
    txt = open(os.path.join(PKG, "build", "rmav_policy_abi.gfx950.s")).read()
    bodies = re.split(r"^(_ZN4rmav\w+):[^\n]*\n", txt, flags=re.M)
    seen = 0
    for name, body in zip(bodies[1::2], bodies[2::2]):
        if not re.match(r"_ZN4rmav(17k_rollout_pair_dr|24k_rollout_pair_shared_dr|16k_rollout_nrm_dr)", name):
            continue
        seen += 1
        body = body.split(".Lfunc_end")[0]
        for bad in ("ds_bpermute", "ds_permute", "v_pk_mul_f32", "v_pk_mov_b32"):
            assert bad not in body, (name, bad)
    assert seen == 24, seen


def test_no_new_kernel_uses_scratch_and_families_are_unchanged(usage):
    """Every kernel of the new translation unit is clean, and the ranged kernels have names no pre-existing prefix matches: the
    families test_resource_usage.py / test_time_limit_build.py count keep their sizes."""
    new = [n for n in usage if re.match(r"_ZN4rmavL?(9k_step_dr|12k_rollout_dr|16k_rollout_nrm_dr|17k_rollout_pair_dr|24k_rollout_pair_shared_dr|12k_range_draw)", n)]
    assert len(new) == 16 + 72 + 24 + 1, len(new)
    for n in new:
        assert _clean(usage[n]), (n, usage[n])
    expected = {"_ZN4rmav6k_stepILi": 28, "_ZN4rmav10k_step_bigILi": 24, "_ZN4rmav9k_step_tlILi": 16, "_ZN4rmav12k_step_finalILi": 24,
                "_ZN4rmav9k_rolloutILi": 128, "_ZN4rmav12k_rollout_tlILi": 52, "_ZN4rmav14k_rollout_bootILi": 4, "_ZN4rmav13k_rollout_nrmILi": 8,
                "_ZN4rmav14k_rollout_pairILi": 10, "_ZN4rmav21k_rollout_pair_sharedILi": 5,
                "_ZN4rmav17k_rollout_pair_tlILi": 4, "_ZN4rmav24k_rollout_pair_shared_tlILi": 4,
                "_ZN4rmav19k_rollout_pair_bootILi": 4, "_ZN4rmav26k_rollout_pair_shared_bootILi": 4,
                "_ZN4rmav18k_rollout_pair_nrmILi": 8, "_ZN4rmav25k_rollout_pair_shared_nrmILi": 8}
    for prefix, count in expected.items():
        assert len(_hits(usage, prefix)) == count, (prefix, sorted(_hits(usage, prefix)))

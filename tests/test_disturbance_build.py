"""Wind / gust disturbance (rmav_set_disturbance), what can be checked without a GPU: the three entry points are declared, exported and
bound; the new kernel families exist for the four quadrotor kinds with the members stated here, use no scratch and spill no vector
register (`make asm`); their names match no pre-existing family prefix and the older families keep their members; registers and occupancy
are what was observed (profiles/r18/disturbance.md has the table beside the tracking-reward kernels they are cut from); and the
disturbance is a handful of Philox calls, not a second copy of the dynamics."""
import pytest

import buildinfo as B
from test_frame_skip_build import SKIP
from test_reward_build import REWARD

NEW = {"rmav_set_disturbance": ("int", 2), "rmav_get_disturbance": ("int", 3), "rmav_disturbance_now": ("int", 3)}
# family prefix -> members: k_step_ds<K, TL, RW>; k_rollout_ds<K, MODE in (buffer, random, controller), TL, RW> (one store policy);
# k_disturbance_now<K>; the policy rollouts k_rollout_nrm_ds / k_rollout_pair_ds / k_rollout_pair_shared_ds<K, BOOT, RW> (rmav_policy_abi).
DISTURB = {"_ZN4rmav9k_step_dsILi": 4 * 2 * 2, "_ZN4rmav12k_rollout_dsILi": 4 * 3 * 2 * 2, "_ZN4rmav17k_disturbance_nowILi": 4}
POLICY = {"_ZN4rmav16k_rollout_nrm_dsILi": 4 * 2 * 2, "_ZN4rmav17k_rollout_pair_dsILi": 4 * 2 * 2, "_ZN4rmav24k_rollout_pair_shared_dsILi": 4 * 2 * 2}
SET = "_ZN4rmav17k_set_disturbanceEPjNS_11DisturbSpecE"   # the launch that rewrites the handle's device copy of the spec


def disturb_family(prefix):
    h = B.hits(prefix)
    assert len(h) == {**DISTURB, **POLICY}[prefix], (prefix, sorted(h))
    return h


def test_disturbance_entry_points_are_declared_exported_and_bound(built):
    A, _ = B.assert_entry_points(NEW)
    import ctypes as C

    S = A.DisturbanceSpec
    assert C.sizeof(S) == 40 and (S.wind_lo.offset, S.wind_hi.offset, S.gust.offset, S.gust_hold.offset) == (0, 12, 24, 36)


@pytest.mark.parametrize("prefix", sorted({**DISTURB, **POLICY}))
def test_every_new_family_exists_for_every_kind_and_is_clean(prefix):
    h = disturb_family(prefix)
    for kind in range(4):
        mine = [n for n in h if n.startswith(f"{prefix}{kind}E")]
        assert len(mine) == len(h) // 4, (prefix, kind, mine)
    for n, u in h.items():
        assert B.clean(u), (n, u)
        # the spec by value; the policy kernels read the handle's device copy
        assert ("PolicyDisturbArgs" if prefix in POLICY else "_11DisturbArgsE") in n, n


def test_no_new_name_matches_an_older_prefix():
    seen = {**B.family(*B.FAMILIES)}
    for census in (SKIP, REWARD):
        for p in census:
            h = B.hits(p)
            assert len(h) == census[p], (p, sorted(h))
            seen.update(h)
    new = {}
    for p in DISTURB:
        new.update(disturb_family(p))
    assert len(new) == 68 and not set(new) & set(seen)
    assert set(B.bodies("rmav_disturb_abi")) == set(new) | {SET}, "the unit holds the new kernels and nothing else"
    pol = {}
    for p in POLICY:
        pol.update(disturb_family(p))
    assert len(pol) == 48 and not set(pol) & set(seen) and set(pol) <= set(B.bodies("rmav_policy_abi"))


# (kind, registers and occupancy of k_step_ds as observed; k_step_rw beside them: 45 / 7, 77 / 6, 45 / 8 (by amdgpu_waves_per_eu), 97 / 4)
@pytest.mark.parametrize("kind,vgpr,occ", [(0, 49, 7), (1, 83, 5), (2, 47, 7), (3, 105, 4)])
def test_single_step_kernels(kind, vgpr, occ):
    hits = B.hits(f"_ZN4rmav9k_step_dsILi{kind}E")
    assert len(hits) == 4, sorted(hits)
    for n, u in hits.items():
        assert u["vgpr"] <= vgpr and u["occ"] == occ, (n, u)


# (kind, {mode: (registers, minimum occupancy)} of k_rollout_ds as observed; the wind, the spare wind and the gust are up to nine lane
# registers, and gv + d turns three scalar constants - six registers in the fp64 kinds - into lane values: +11 .. 20 over k_rollout_rw)
@pytest.mark.parametrize("kind,budget", [(0, {0: (85, 5), 1: (85, 5), 2: (104, 4)}), (1, {0: (129, 3), 1: (131, 3), 2: (151, 3)}),
                                         (2, {0: (88, 5), 1: (86, 5), 2: (104, 4)}), (3, {0: (160, 3), 1: (158, 3), 2: (176, 2)})])
def test_fused_disturbed_kernels(kind, budget):
    for mode, (vgpr, occ) in budget.items():
        hits = B.hits(f"_ZN4rmav12k_rollout_dsILi{kind}ELi{mode}E")
        assert len(hits) == 4, (kind, mode, sorted(hits))
        for n, u in hits.items():
            assert B.clean(u) and u["vgpr"] <= vgpr and u["occ"] >= occ, (n, u)


def test_the_disturbance_is_a_few_philox_calls():
    """k_rollout_ds<K, MODE, no limit, RW> against its k_rollout_rw counterpart (default store policy): at most 1.35 x the instructions of
    the listing - the wind at the start of the launch, the spare wind at its two sites, the gust at the start and in the loop: five
    inlined Philox calls of ~70 instructions on bodies of 1 500 .. 2 400; observed 1.11 .. 1.34.  k_step_ds against k_step_rw: two
    calls, at most 1.15 x (observed 1.07 .. 1.14)."""
    ds, rw = B.bodies("rmav_disturb_abi"), B.bodies("rmav_reward_abi")
    count = lambda body: sum(1 for ln in body.split("\n") if ln.startswith("\t") and not ln.startswith("\t."))   # noqa: E731
    for kind in range(4):
        for mode in range(3):
            d = next(b for n, b in ds.items() if n.startswith(f"_ZN4rmav12k_rollout_dsILi{kind}ELi{mode}ELb0ELb1E"))
            r = next(b for n, b in rw.items() if n.startswith(f"_ZN4rmav12k_rollout_rwILi{kind}ELi{mode}ELi0ELb0E"))
            assert count(d) <= 1.35 * count(r), (kind, mode, count(d), count(r))
        d = next(b for n, b in ds.items() if n.startswith(f"_ZN4rmav9k_step_dsILi{kind}ELb0ELb1E"))
        r = next(b for n, b in rw.items() if n.startswith(f"_ZN4rmav9k_step_rwILi{kind}ELb0E"))
        assert count(d) <= 1.15 * count(r), (kind, count(d), count(r))


# (kind, registers of the three disturbed actors as observed - all four (BOOT, RW) members within the figure - and their minimum occupancy;
# the tracking-reward counterparts: profiles/r18/disturbance.md)
@pytest.mark.parametrize("kind,budget", [(0, {"16k_rollout_nrm_ds": (143, 3), "17k_rollout_pair_ds": (182, 2), "24k_rollout_pair_shared_ds": (144, 3)}),
                                         (1, {"16k_rollout_nrm_ds": (161, 2), "17k_rollout_pair_ds": (207, 2), "24k_rollout_pair_shared_ds": (170, 2)}),
                                         (2, {"16k_rollout_nrm_ds": (148, 2), "17k_rollout_pair_ds": (195, 2), "24k_rollout_pair_shared_ds": (156, 3)}),
                                         (3, {"16k_rollout_nrm_ds": (200, 2), "17k_rollout_pair_ds": (226, 2), "24k_rollout_pair_shared_ds": (191, 2)})])
def test_disturbed_policy_kernels(kind, budget):
    for fam, (vgpr, occ) in budget.items():
        hits = B.hits(f"_ZN4rmav{fam}ILi{kind}E")
        assert len(hits) == 4, (kind, fam, sorted(hits))
        for n, u in hits.items():
            assert B.clean(u) and u["vgpr"] <= vgpr and u["occ"] >= occ, (n, u)


def test_the_disturbance_of_a_policy_kernel_is_a_few_philox_calls():
    """k_rollout_*_ds<K, BOOT, reward> against its *_rw counterpart: the fp32 actor runs k_rollout_ds's body - five inlined Philox calls of ~70
    instructions on bodies of 1 900 .. 2 900 instructions, at most 350 / 1 900 = 0.18 more; the pair kernels keep no spare wind - the wind
    and the gust at the start, the gust in the loop, the wind on the reset path: four calls on bodies of 3 600 .. 6 400.  At most 1.2 x."""
    pol = B.bodies("rmav_policy_abi")
    count = lambda body: sum(1 for ln in body.split("\n") if ln.startswith("\t") and not ln.startswith("\t."))   # noqa: E731
    for fam in ("16k_rollout_nrm", "17k_rollout_pair", "24k_rollout_pair_shared"):
        for kind in range(4):
            for boot in (0, 1):
                d = next(b for n, b in pol.items() if n.startswith(f"_ZN4rmav{fam}_dsILi{kind}ELb{boot}ELb1E"))
                r = next(b for n, b in pol.items() if n.startswith(f"_ZN4rmav{fam}_rwILi{kind}ELb{boot}E"))
                print(fam, kind, boot, count(d), count(r), round(count(d) / count(r), 3))
                assert count(d) <= 1.2 * count(r), (fam, kind, boot, count(d), count(r))

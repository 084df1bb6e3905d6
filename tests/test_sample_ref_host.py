"""oracle/sample_ref.py without a GPU: its vectorised Philox is the oracle's, its noise is the spec the older tests state
(test_gpu_ppo._predicted_noise), the edge table (tests/noise_edges.py) is what it claims, the zero-head policy's mean is its bias, and the
bound is tight enough to see twelve arithmetic mutants of the sampling half - on exactly the counters tests/test_gpu_policy_sample.py
launches (the builders of those inputs live here and are imported there)."""
import functools

import numpy as np
import pytest

import noise_edges as E
import oracle as O
import policy_ref as R
import sample_ref as S
from test_gpu_ppo import _predicted_noise
from test_policy_ref_host import dims, family, nets_of

SEED, BASE, T = E.SEED, 1000, 5
B3 = np.array([0.173, -0.2371, 0.0911, -0.1457], np.float32)        # the zero-head policy's action bias = its mean, everywhere
WIDE_BASE = 2 ** 40 + 3
LATE_T0 = (2 ** 32 - 2, 2 ** 48 - 2)                                 # t crosses 2^32 / 2^48 inside a 5-step launch
ACTORS = ("fp32", "fp32_mfma", "bf16", "bf16_1w", "f16", "f16_shared")
PAIR_ACTORS = ("bf16", "f16", "f16_shared")
VARIANT_ACTORS = ("fp32_mfma", "f16", "f16_shared")
VARIANTS = ("tl", "tl_boot", "norm", "ranged", "skip3", "reward", "clip")
PLAIN_SHAPES = (("quad2d", 1), ("quad2d_sl", 63), ("quad3d", 65), ("quad3d_sl", 130), ("reinmav", 65))
PAIR_SHAPES = (("quad3d", 300, 1), ("quad2d_sl", 300, 4))            # (kind, n, pair_group)
_QUAD = ("quad2d", "quad2d_sl", "quad3d", "quad3d_sl")
_SIZES = (1, 63, 65, 130)


def variant_shapes(variant):
    """Sizes paired with kinds, rotated by the variant (as test_gpu_frame_skip.py pairs them): every variant sees every kind and every
    size, every (kind, size) pair is seen by some variant."""
    r = VARIANTS.index(variant)
    return tuple((k, _SIZES[(i + r) % 4]) for i, k in enumerate(_QUAD))


def plain_cases():
    """(actor, kind, n, variant, pair_group or None) of part (a) of the GPU test."""
    out = [(a, k, n, "plain", None) for a in ACTORS for k, n in PLAIN_SHAPES]
    out += [(a, k, n, "plain", g) for a in PAIR_ACTORS for k, n, g in PAIR_SHAPES]
    out += [(a, k, n, v, None) for a in VARIANT_ACTORS for v in VARIANTS for k, n in variant_shapes(v)]
    out += [(a, "quad3d_sl", 300, v, (1, 4)[i % 2]) for a in ("f16", "f16_shared") for i, v in enumerate(VARIANTS)]
    return out


def logstd_of(nA):
    return np.linspace(-1.2, 0.7, nA).astype(np.float32)


def zero_head_policy(fam, kind):
    """CPU MlpPolicy with dense hidden layers (default init + 0.3 randn, biases in +-0.3), a ZERO action-head weight, the action bias
    B3 and a distinct log-std per component: its mean is B3 whatever the observation."""
    import torch
    from gym_reinmav_amd.ppo import MlpPolicy

    nS, nA = dims(kind)
    torch.manual_seed(77 + nS)
    pol = MlpPolicy(nS, nA, value_network="shared" if fam == "f16_shared" else "copy")
    with torch.no_grad():
        for net in (pol.pi, pol.vf):
            for lin in net:
                lin.weight.add_(torch.randn_like(lin.weight) * 0.3)
                lin.bias.uniform_(-0.3, 0.3)
        pol.pi[2].weight.zero_()
        pol.pi[2].bias.copy_(torch.from_numpy(B3[:nA]))
        pol.logstd.copy_(torch.from_numpy(logstd_of(nA)))
    return pol


@functools.lru_cache(maxsize=None)
def mean_reference(fam, kind):
    """(mean [nA], mean_bound [nA]) of the zero-head policy from oracle/policy_ref.py, over 130 spread-out observations (the largest
    bound of any of them; the mean itself must not depend on the observation)."""
    nS, nA = dims(kind)
    obs = np.random.RandomState(5).uniform(-3, 3, (nS, 130)).astype(np.float32)
    res = R.ACTORS[fam](nets_of(zero_head_policy(fam, kind)), obs)
    assert (res.mean == res.mean[0]).all()
    return res.mean[0].copy(), res.bound[:, :nA].max(0)


@functools.lru_cache(maxsize=None)
def noise_grid(base, n, t0, steps=T):
    """(z_ref [steps, n, 4], rad_ref [steps, n, 2], bound_z [steps, n, 4]) of a launch of `steps` steps from step t0 on env ids
    base .. base + n - 1; computed once, read-only."""
    e = np.array([base + i for i in range(n)], dtype=np.uint64)[None, :]
    t = np.array([t0 + k for k in range(steps)], dtype=np.uint64)[:, None]
    out = S.noise(SEED, e, t)
    for a in out:
        a.setflags(write=False)
    return out


def edge_launch(i, entry):
    """Where entry i of an edge table sits in its 65-env, T-step launch: (env_id_base, step_count, lane j, step s); j cycles over
    first lane, last lane of the first wavefront, lane 64; s over 0 .. T - 1."""
    _, _, _, env_id, t = entry
    j, s = (0, 63, 64)[i % 3], i % T
    return env_id - j, t - s, j, s


# ---- Philox ---------------------------------------------------------------------------------------------------------------------------
def test_vectorised_philox_is_the_oracles():
    rng = np.random.RandomState(1)
    cases = [(int(rng.randint(0, 2 ** 31)), int(rng.randint(0, 2 ** 31)), int(rng.randint(0, 2 ** 31))) for _ in range(40)]
    big = lambda lo: lo + int(rng.randint(0, 2 ** 31))  # noqa: E731
    cases += [(big(2 ** 32), big(0), big(0)), (big(2 ** 40), big(2 ** 32), 21), (big(0), big(2 ** 48), 21), (big(2 ** 63), big(2 ** 63), big(2 ** 63)),
              (2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1), (WIDE_BASE, 2 ** 32 - 1, SEED), (BASE, 2 ** 48 + 1, SEED)]
    for e, t, seed in cases:
        for tag in (1, 2, 3):
            want = O.philox([e & 0xFFFFFFFF, e >> 32, t & 0xFFFFFFFF, (tag << 24) | (((t >> 32) & 0xFFFF) << 8)], [seed & 0xFFFFFFFF, seed >> 32])
            got = S.noise_words(seed, e, t, tag=tag)
            assert np.array_equal(got.astype(np.uint32), want), (e, t, seed, tag)
    # arrays against scalars: the broadcast draws what the one-by-one calls draw
    e = np.array([3, 2 ** 33 + 5, 2 ** 63 + 1], dtype=np.uint64)
    t = np.array([0, 2 ** 32, 2 ** 47 + 9], dtype=np.uint64)
    grid = S.noise_words(SEED, e[None, :], t[:, None])
    for i in range(3):
        for j in range(3):
            assert np.array_equal(grid[i, j], S.noise_words(SEED, int(e[j]), int(t[i])))


def test_noise_is_the_spec_the_older_tests_state():
    """|_predicted_noise - z_ref| inside the asserted bound (the fp32 NumPy emulation's log, sqrt and product round as the bound
    allows a kernel to), on the regular grid, the wide env ids, the 2^32 crossing and every edge entry."""
    worst = 0.0
    for base, n, t0 in [(BASE, 300, 0), (WIDE_BASE, 65, 0), (BASE, 65, LATE_T0[0]), (BASE, 65, LATE_T0[1])]:
        z, _, bz = noise_grid(base, n, t0)
        ids = np.arange(0, n, 7)
        for k in (0, 2, T - 1):
            zp = _predicted_noise(SEED, [base + int(i) for i in ids], t0 + k).astype(np.float64)
            ratio = np.abs(zp - z[k, ids]) / (S.SAFETY * bz[k, ids])
            worst = max(worst, float(ratio.max()))
    for table in (E.EDGES, E.EDGES_WIDE_ENV, E.EDGES_LATE_T):
        for kind, w, top, env_id, t in table:
            z, _, bz = S.noise(SEED, env_id, t)
            zp = _predicted_noise(SEED, [env_id], t)[0].astype(np.float64)
            assert np.isfinite(zp).all() and np.isfinite(z).all()
            d, b = np.abs(zp - z), S.SAFETY * bz
            assert (d <= b).all(), (kind, w, env_id, t, d, b)
            worst = max(worst, float((d[b > 0] / b[b > 0]).max()))
    print(f"fp32 NumPy emulation against z_ref: worst error / asserted bound {worst:.3f}")
    assert worst <= 1.0


# ---- the edge table ---------------------------------------------------------------------------------------------------------------------
RADIUS = {"u1_min": 0x000000, "u1_one": 0xFFFFFF, "u1_next_to_one": 0xFFFFFE}
ANGLE = {"turn_0": 0x000000, "turn_1_4": 0x400000, "turn_1_2": 0x800000, "turn_3_4": 0xC00000, "turn_last": 0xFFFFFF}


def exact_zero_components(entry):
    """Components of z that the spec makes EXACTLY zero at an edge entry (u1 = 1: both of the pair; a quarter turn: sin or cos)."""
    kind, w, _, _, _ = entry
    p = 2 * (w // 2)
    return {"u1_one": (p, p + 1), "turn_0": (p + 1,), "turn_1_2": (p + 1,), "turn_1_4": (p,), "turn_3_4": (p,)}.get(kind, ())


def test_edge_table_is_what_it_claims():
    seen = set()
    for name, table in (("EDGES", E.EDGES), ("EDGES_WIDE_ENV", E.EDGES_WIDE_ENV), ("EDGES_LATE_T", E.EDGES_LATE_T)):
        assert len(table) > 0, name
        for i, (kind, w, top, env_id, t) in enumerate(table):
            r = O.philox([env_id & 0xFFFFFFFF, env_id >> 32, t & 0xFFFFFFFF, (3 << 24) | (((t >> 32) & 0xFFFF) << 8)], [SEED & 0xFFFFFFFF, SEED >> 32])
            assert int(r[w]) >> 8 == top, (name, kind, w, env_id, t, hex(int(r[w])))
            assert (RADIUS if w % 2 == 0 else ANGLE)[kind] == top
            base, t0, j, s = edge_launch(i, (kind, w, top, env_id, t))
            assert base >= 0 and t0 >= 0 and base + j == env_id and t0 + s == t
            if name == "EDGES":
                assert env_id < 2 ** 26
                seen.add((kind, w % 2))
            if name == "EDGES_WIDE_ENV":
                assert env_id >= 2 ** 32
            if name == "EDGES_LATE_T":
                assert 2 ** 32 - 16 <= t < 2 ** 32
            # ... and the reference does there what the spec says
            z, rad, _ = S.noise(SEED, env_id, t)
            p = w // 2
            if kind == "u1_min":
                assert abs(rad[p] - np.sqrt(48.0 * np.log(2.0))) < 1e-12      # sqrt(-2 ln 2^-24) = 5.768
            if kind == "u1_one":
                assert rad[p] == 0.0
            if kind == "u1_next_to_one":
                assert abs(rad[p] - np.sqrt(2.0 * 2.0 ** -24)) < 1e-10
            for c in exact_zero_components((kind, w, top, env_id, t)):
                assert z[c] == 0.0, (kind, w, c, z)
    # every kind of edge is in the main table, for a radius word and for an angle word
    assert seen == {(k, 0) for k in RADIUS} | {(k, 1) for k in ANGLE}, seen


# ---- the zero-head policy ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["fp32", "bf16", "f16", "f16_shared"])
def test_zero_head_mean_is_its_bias(fam):
    """policy_ref's mean of the zero-head policy IS B3 (as fp32), for every observation, and its bound is 2 (64 + 2) 2^-24 |b3| = 66 ulps
    of b3 for every family: policy_ref charges one ulp per multiply-add of the padded depth 64 and per bias add whatever the operands
    are, so it cannot know that 64 products with a zero weight add exact zeros.  It is used as it is (the issue: "use its bound as it
    is"); the EXACT equality of the kernel's mean and b3 is asserted on the GPU where z is exactly zero (part c)."""
    for kind in ("quad2d", "quad2d_sl", "quad3d", "quad3d_sl", "reinmav"):
        nA = dims(kind)[1]
        mean, bound = mean_reference(fam, kind)
        assert np.array_equal(mean, B3[:nA].astype(np.float64)), (fam, kind)
        ulps = bound / (2.0 * S.U * np.abs(mean))
        print(f"{fam} {kind}: mean_bound = {ulps.max():.1f} ulps of b3 ({bound.max():.3g})")
        assert (bound <= 132.0 * S.U * np.abs(mean) * (1 + 1e-12)).all() and (bound > 0).all()


@pytest.mark.parametrize("actor", ["fp32", "fp32_mfma", "bf16", "f16", "f16_shared"])
def test_packer_pads_the_staged_logstd_with_zeros(actor):
    """The staged log-std has four slots; for a 2-action kind the packer fills slots 2 and 3 with zeros.  That padding is what makes a
    sum over four slots equal the sum over nA (see test_every_mutant_leaves_the_bound, `logstd_sum4`)."""
    from gym_reinmav_amd.ppo import _PolicyPacker

    for kind in ("quad2d", "quad3d"):
        nS, nA = dims(kind)
        buf = _PolicyPacker(zero_head_policy(family(actor), kind), nS, actor).pack().numpy()
        want = np.zeros(4, np.float32)
        want[:nA] = logstd_of(nA)
        assert np.array_equal(buf[-4:], want), (actor, kind, buf[-4:])


# ---- mutants ----------------------------------------------------------------------------------------------------------------------------
def _counter_sets():
    """[(name, env ids [n], steps [k])] of everything the GPU test launches."""
    sets = [("regular", BASE, 300, 0), ("wide env ids", WIDE_BASE, 65, 0)] + [(f"t0 = {t0}", BASE, 65, t0) for t0 in LATE_T0]
    for name, table in (("edge", E.EDGES), ("edge, wide env id", E.EDGES_WIDE_ENV), ("edge, late t", E.EDGES_LATE_T)):
        for i, en in enumerate(table):
            base, t0, _, _ = edge_launch(i, en)
            sets.append((f"{name} {en[0]} r{en[1]}", base, 65, t0))
    return sets


def _factor(mut, nA):
    """Largest |mutated - reference| / asserted bound over every stored quantity of every launch, and where."""
    mean, mb = mean_reference("f16", "quad3d" if nA == 4 else "quad2d")
    worst, where = 0.0, None
    noise_level = mut not in ("std_xor1", "logstd_sum4", "q_sum4")
    for name, base, n, t0 in _counter_sets():
        z, _, bz = noise_grid(base, n, t0)
        ref = S.sample(mean, mb, logstd_of(nA), 1.0, z, bz, nA)
        if noise_level:
            e = np.array([base + i for i in range(n)], dtype=np.uint64)[None, :]
            t = np.array([t0 + k for k in range(T)], dtype=np.uint64)[:, None]
            zm = S.noise(SEED, e, t, mutant=mut)[0]
            got = S.sample(mean, mb, logstd_of(nA), 1.0, zm, bz, nA)
        else:
            got = S.sample(mean, mb, logstd_of(nA), 1.0, z, bz, nA, mutant=mut)
        with np.errstate(invalid="ignore"):
            fa = np.abs(got.act - ref.act) / ref.bound_act
            fl = np.abs(got.logp - ref.logp) / ref.bound_logp
        f = max(float(np.where(np.isnan(fa), np.inf, fa).max()), float(np.where(np.isnan(fl), np.inf, fl).max()))
        if f > worst:
            worst, where = f, name
    return worst, where


@pytest.mark.parametrize("mut", [m for m in S.MUTANTS if m != "logstd_sum4"])
def test_every_mutant_leaves_the_bound(mut):
    """Each mutant of the sampling half puts a stored action or log-probability more than 10x outside the asserted bound somewhere on
    the GPU test's counters (an inf / NaN counts as outside), with 2 and with 4 actions - except where it is no mutation with 4
    (`q_sum4`)."""
    for nA in (2, 4):
        if mut == "q_sum4" and nA == 4:
            continue
        f, where = _factor(mut, nA)
        print(f"MUTANT {mut} nA={nA}: {f:.3g} x the bound ({where})")
        assert f > 10.0, (mut, nA, f)


def test_fast_log_is_caught_at_u1_next_to_one_and_only_at_the_edges():
    mean, mb = mean_reference("f16", "quad3d")
    z, _, bz = noise_grid(BASE, 300, 0)
    e = np.array([BASE + i for i in range(300)], dtype=np.uint64)[None, :]
    t = np.arange(T, dtype=np.uint64)[:, None]
    ref = S.sample(mean, mb, logstd_of(4), 1.0, z, bz, 4)
    got = S.sample(mean, mb, logstd_of(4), 1.0, S.noise(SEED, e, t, mutant="fast_log")[0], bz, 4)
    regular = float((np.abs(got.act - ref.act) / ref.bound_act).max())
    edge = 0.0
    for kind, w, top, env_id, tt in E.EDGES:
        if kind == "u1_next_to_one":
            z1, _, b1 = S.noise(SEED, env_id, tt)
            r1 = S.sample(mean, mb, logstd_of(4), 1.0, z1, b1, 4)
            g1 = S.sample(mean, mb, logstd_of(4), 1.0, S.noise(SEED, env_id, tt, mutant="fast_log")[0], b1, 4)
            edge = max(edge, float((np.abs(g1.act - r1.act) / r1.bound_act).max()))
    print(f"MUTANT fast_log: regular grid {regular:.3g} x the bound, u1 next to 1: {edge:.3g} x")
    assert edge > 10.0


def test_logstd_summed_over_four_slots_is_no_mutation_behind_the_packers_zero_padding():
    """`logstd_sum4` (the sum of the staged log-std over 4 slots instead of nA, for the 2-action kinds) CANNOT leave any bound through
    the public API: the slots it adds hold the packer's zeros (test_packer_pads_the_staged_logstd_with_zeros), so the sum has the same
    bits.  The hook itself works: with anything else in those slots it is ~1e6 x outside."""
    f, _ = _factor("logstd_sum4", 2)
    assert f == 0.0
    mean, mb = mean_reference("f16", "quad2d")
    z, _, bz = noise_grid(BASE, 300, 0)
    ref = S.sample(mean, mb, logstd_of(2), 1.0, z, bz, 2)
    got = S.sample(mean, mb, logstd_of(2), 1.0, z, bz, 2, mutant="logstd_sum4", logstd_pad=(0, 0, 0.3, -0.9))
    f = float((np.abs(got.logp - ref.logp) / ref.bound_logp).max())
    print(f"MUTANT logstd_sum4 nA=2: 0 x the bound behind zero padding; {f:.3g} x with (0.3, -0.9) in the padding slots")
    assert f > 10.0


def test_reference_sample_is_the_torch_policys_density():
    """logp_ref is MlpPolicy.log_prob of act_ref under the zero-head policy (fp64 torch), and act_ref = mean + std z."""
    import copy

    import torch

    for kind in ("quad2d_sl", "quad3d"):
        nA = dims(kind)[1]
        pol = copy.deepcopy(zero_head_policy("fp32", kind)).double()
        mean, mb = mean_reference("fp32", kind)
        z, _, bz = noise_grid(BASE, 300, 0)
        smp = S.sample(mean, mb, logstd_of(nA), 1.0, z, bz, nA)
        act = torch.from_numpy(smp.act.reshape(-1, nA).T.copy())
        m = torch.from_numpy(np.broadcast_to(mean[:, None], act.shape).copy())
        with torch.no_grad():
            lp = pol.log_prob(m, act).numpy().reshape(smp.logp.shape)
        assert np.abs(lp - smp.logp).max() < 1e-9
        assert np.isfinite(smp.bound_act).all() and np.isfinite(smp.bound_logp).all()
        # the bound is small against what the older tests accept (6e-3 on the implied noise, 1e-3 on logp)
        print(f"{kind}: bound_act max {smp.bound_act.max():.3g}, bound_logp max {smp.bound_logp.max():.3g}")
        assert smp.bound_act.max() < 6e-3 * float(smp.std.min()) / 50 and smp.bound_logp.max() < 1e-3 / 10


def test_case_list():
    cases = plain_cases()
    assert len(set(cases)) == len(cases) and 120 <= len(cases) <= 160, len(cases)
    assert {c[0] for c in cases} == set(ACTORS) and {c[3] for c in cases} == {"plain", *VARIANTS}
    for v in VARIANTS:
        assert {k for k, _ in variant_shapes(v)} == set(_QUAD) and {n for _, n in variant_shapes(v)} == set(_SIZES)

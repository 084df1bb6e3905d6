"""Wind / gust disturbance (rmav_set_disturbance), what can be checked without a GPU: the kernels' draw functions (csrc/rmav_disturb.hpp,
compiled for the host as the stand-alone program tests/disturb_host) equal the numpy restatement tests/disturbance_ref.py bit for bit -
at the edges of every counter too -; ranges, lo == hi and the all-zero spec; the Python class; and how rare tether-edge steps are in
the inputs of the GPU parity test."""
import os
import subprocess

import numpy as np
import pytest

import disturbance_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DIR = os.path.join(ROOT, "tests", "disturb_host")
F32 = np.float32


@pytest.fixture(scope="module")
def host():
    subprocess.run(["make", "-s", "-C", HOST_DIR], check=True)
    exe = os.path.join(HOST_DIR, "_build", "disturb_host")

    def run(cases):
        """cases: [(spec, seed, env_id, reset_idx, t)] -> uint32 [len, 9]: the bits of w, q, d."""
        def bits(x):
            return "%08x" % int(np.array([x], F32).view(np.uint32)[0])

        lines = []
        for spec, seed, env, rc, t in cases:
            v = list(spec["wind_lo"]) + list(spec["wind_hi"]) + list(spec["gust"])
            lines.append(" ".join(["%x" % seed, "%x" % env, "%x" % rc, "%x" % t] + [bits(x) for x in v] + ["%x" % spec["gust_hold"]]))
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split()
        assert len(out) == 9 * len(cases), (len(out), len(cases))
        return np.array([int(x, 16) for x in out], np.uint64).astype(np.uint32).reshape(len(cases), 9)

    return run


def ref_bits(spec, seed, env, rc, t):
    w, q = R.wind(spec, seed, env, rc), R.gust(spec, seed, env, t)
    return np.concatenate([w, q, (w + q).astype(F32)]).view(np.uint32)


EDGE_T = (0, 1, 2, 3, 2**32 - 1, 2**32, 2**32 + 1, 2**48 - 2, 2**48 - 1, 3 * 2**32 - 1, 3 * 2**32, 2**20 * (2**32 - 1) + 5, 2**20 * 2**32 - 1)
EDGE_ENV = (0, 1, 2**32 - 1, 2**32, 2**40 + 12345, 2**63 + 7)
EDGE_RC = (0, 1, 2**32 - 1, 2**31)


def test_the_draw_functions_equal_the_restatement_bit_for_bit(host):
    rng = np.random.RandomState(5)
    cases = []
    for hold in (1, 3, 1048576):
        spec = dict(R.SPEC, gust_hold=hold)
        for t in EDGE_T:
            for env in EDGE_ENV:
                cases.append((spec, 11, env, 0, t))
        for rc in EDGE_RC:
            cases.append((spec, 2**64 - 3, 2**40 + 1, rc, 7))
    for _ in range(200):   # random specs, seeds and counters
        lo = rng.uniform(-3, 3, 3)
        spec = dict(wind_lo=tuple(float(F32(x)) for x in lo), wind_hi=tuple(float(F32(x)) for x in lo + rng.uniform(0, 4, 3)),
                    gust=tuple(float(F32(x)) for x in rng.uniform(0, 2, 3)), gust_hold=int(rng.randint(1, 50)))
        cases.append((spec, int(rng.randint(0, 2**62)), int(rng.randint(0, 2**62)), int(rng.randint(0, 2**32)), int(rng.randint(0, 2**47))))
    got = host(cases)
    for c, g in zip(cases, got):
        assert np.array_equal(g, ref_bits(*c)), (c, g, ref_bits(*c))
    # the gust is held: t and t' of one block give one value, the next block another; the block index reaches the counter's high word
    spec = dict(R.SPEC, gust_hold=3)
    a, b, c = host([(spec, 11, 5, 0, 3 * 2**32 - 1), (spec, 11, 5, 0, 3 * 2**32 - 3), (spec, 11, 5, 0, 3 * 2**32)])
    assert np.array_equal(a, b) and not np.array_equal(a[3:6], c[3:6]) and np.array_equal(a[:3], c[:3])
    # the reset index wraps at 2^32 (the running episode of a record that holds 0 is 2^32 - 1)
    assert np.array_equal(R.wind(R.SPEC, 11, 5, -1), R.wind(R.SPEC, 11, 5, 2**32 - 1))


def test_ranges_equal_bounds_and_the_zero_spec(host):
    rng = np.random.RandomState(6)
    spec = dict(wind_lo=(-1.5, 0.25, 2.0), wind_hi=(0.5, 0.25, 2.0 + 2**-20), gust=(0.75, 0.0, 1e-3), gust_hold=2)
    cases = [(spec, 3, int(e), int(rc), int(t)) for e, rc, t in zip(rng.randint(0, 2**40, 500), rng.randint(0, 2**32, 500), rng.randint(0, 2**40, 500))]
    got = host(cases).view(F32)
    lo, hi, g = (np.array(spec[k], F32) for k in ("wind_lo", "wind_hi", "gust"))
    w, q, d = got[:, 0:3], got[:, 3:6], got[:, 6:9]
    assert (w >= lo).all() and (w <= hi).all()
    assert (q >= -g).all() and ((q < g) | (g == 0)).all()
    assert (d >= lo - g).all() and (d <= hi + g).all()
    assert (w[:, 1] == F32(0.25)).all() and (q[:, 1] == 0).all()             # lo == hi is exact: fma(0, u, lo); a zero amplitude gives 0
    assert len(np.unique(w[:, 0])) > 400 and len(np.unique(q[:, 0])) > 400   # and the others do vary
    zero = host([(R.ZERO, 3, int(e), 1, int(t)) for e, t in zip(rng.randint(0, 2**40, 50), rng.randint(0, 2**40, 50))])
    assert (zero == 0).all(), "an all-zero spec gives +0 in w, q and d"
    assert (np.concatenate([ref_bits(R.ZERO, 3, 9, 1, 4)]) == 0).all()


def test_the_python_class_validates_and_parses(built):
    import gym_reinmav_amd as g
    from gym_reinmav_amd import _abi as A

    D = g.Disturbance
    d = D.parse("wind=-1:1,-1:1,0:0:gust=0.5,0.5,0.2:hold=25")
    assert d.wind == ((-1.0, 1.0), (-1.0, 1.0), (0.0, 0.0)) and d.gust == (0.5, 0.5, 0.2) and d.hold == 25
    assert eval(repr(d), {"Disturbance": D}).wind == d.wind
    assert D.parse("wind=0.5:hold=3").wind == ((-0.5, 0.5),) * 3 and D.parse("gust=1").gust == (1.0, 1.0, 1.0) and D().hold == 1
    s = d.spec(A.KIND_BY_NAME["quad3d"])
    assert (list(s.wind_lo), list(s.wind_hi), s.gust_hold) == ([-1.0, -1.0, 0.0], [1.0, 1.0, 0.0], 25)
    back = D.from_spec(s)
    assert back.wind == d.wind and back.hold == 25 and back.gust == tuple(float(F32(x)) for x in d.gust)
    s2 = D(wind=((-1, 1), (0, 2)), gust=(0.1, 0.2)).spec(A.KIND_BY_NAME["quad2d_sl"])   # two axes for a 2-D kind; the third is 0
    assert list(s2.wind_hi) == [1.0, 2.0, 0.0] and list(s2.gust)[2] == 0.0
    s3 = D(wind=1.0, gust=0.5).spec(A.KIND_BY_NAME["quad2d"])                            # ... which reads two of three given axes
    assert list(s3.wind_lo) == [-1.0, -1.0, 0.0] and list(s3.gust) == [0.5, 0.5, 0.0]
    for bad in ("wind=1:-1,0:0,0:0", "hold=0", "hold=1048577", "hold=2.5", "foo=1", "wind=1:2", "gust=-1", "gust=1,2,3,4", "", "wind=1:wind=2",
                "gust=nan", "wind=-inf:0,0:0,0:0"):
        with pytest.raises(ValueError):
            D.parse(bad)
    for kw in (dict(wind=-1.0), dict(gust=(1.0,)), dict(wind=((0, 1e39), (0, 0), (0, 0))), dict(wind=((-3e38, 3e38), (0, 0), (0, 0))), dict(gust=2e38)):
        with pytest.raises(ValueError):
            D(**kw)
    for kw in (dict(hold=True), dict(hold=2.0), dict(wind="1"), dict(gust=None), dict(wind=None)):
        with pytest.raises(TypeError):
            D(**kw)
    with pytest.raises(ValueError):
        D(wind=((-1, 1), (0, 2))).spec(A.KIND_BY_NAME["quad3d"])
    with pytest.raises(ValueError):
        D().check_kind(A.REINMAV)
    from gym_reinmav_amd.core import check_disturbance

    with pytest.raises(TypeError):
        check_disturbance("wind=1")
    assert check_disturbance(None) is None


@pytest.mark.parametrize("kind", ("quad2d_sl", "quad3d_sl"))
def test_tether_edge_steps_are_rare_in_the_parity_inputs(built, kind):
    """The GPU parity test accepts either tether branch where a step starts within 2e-6 of |tether| = L.  Over its exact inputs, walked
    with the oracle alone, such (env, step) cases are at most 1 % of all - the cap of that acceptance; none is expected.  (A property of the test inputs: it
    reads the oracle and tests/disturbance_ref.py only, so it does not tell a library with the feature from one without.)"""
    import oracle as O

    edge = total = taut = 0
    for n in (1, 63, 65, 130):
        for phase, _, s, _ in R.oracle_walk(kind, n):
            p = R.parity_params(kind, phase)
            slack = O.tether_slack(kind, s.astype(np.float64), p)
            edge += int((np.abs(slack) < 2e-6).sum())
            taut += int((slack >= 0).sum())
            total += n
    print(f"tether-edge cases {kind}: {edge} of {total}; taut starts: {taut}")
    assert total == (R.PARITY["steps"] + R.PARITY["fresh"]) * (1 + 63 + 65 + 130) and edge <= 0.01 * total
    assert edge == 0
    assert taut > total // 20, "the inputs do exercise the taut branch"

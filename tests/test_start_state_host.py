"""Start-state ranges (rmav_set_start_state), what can be checked without a GPU: the kernels' map statement and the host's derivation of its
coefficients (csrc/rmav_start.hpp, compiled for the host as the stand-alone program tests/start_host) equal the numpy restatement
tests/start_ref.py bit for bit - against the rational fma32_exact, at the identity for all 2^24 values of v, at pinned components for both
ends of the v range, and for a span whose midpoint is not representable; StartState.spec() / coefficients() derive what the library derives;
check_start_state and the class validate their arguments; the example has the flag."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import start_ref as R
from util import KINDS, NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DIR = os.path.join(ROOT, "tests", "start_host")
sys.path.insert(0, os.path.join(ROOT, "reinmav-gym_amd"))

F32 = np.float32
V_MIN, V_MAX = F32(-1.0), F32(1.0 - 2.0 ** -23)     # the ends of the reset stream's range: x = 0 and x = 2^24 - 1


def hexbits(x):
    return "%08x" % int(R.bits(F32(x)))


@pytest.fixture(scope="module")
def host():
    subprocess.run(["make", "-s", "-C", HOST_DIR], check=True)
    exe = os.path.join(HOST_DIR, "_build", "start_host")

    def run(lines, width=1):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split()
        assert len(out) == width * len(lines), (len(out), len(lines))
        return np.array([int(x, 16) for x in out], np.uint64).astype(np.uint32).reshape(len(lines), width)

    return run


def reset_values(rng, n):
    """n values of the reset stream: v = fma(2^-23, x, -1), x in [0, 2^24)"""
    x = rng.randint(0, 1 << 24, n)
    return (x.astype(np.float64) * 2.0 ** -23 - 1.0).astype(F32)     # (exact in fp64, representable in fp32)


def cases():
    """(h, m, v): the tests' ranges of every kind, spans at the edges of fp32, and random ranges - on the ends of v and on random draws"""
    rng = np.random.RandomState(21)
    pairs = []
    for kind in KINDS:
        pairs += list(zip(*R.coeffs(*R.ranges(kind))))
    pairs += [(F32(1.0), F32(0.0)), (F32(0.0), F32(0.25)), (F32(0.0), F32(-3.5)), (F32(2.0 ** -24), F32(1.0)), (F32(1e-30), F32(1e-30)),
              (F32(3.0e38 / 2), F32(0.0)), (F32(1.5), F32(-1.5)), (F32(0.1), F32(0.7))]
    for _ in range(60):
        lo, hi = np.sort(rng.uniform(-1, 1, 2) * 10.0 ** rng.uniform(-3, 3))
        pairs.append(R.coeffs(F32(lo), F32(hi)))
    vs = [V_MIN, V_MAX, F32(0.0), F32(2.0 ** -23), F32(-2.0 ** -23), F32(0.5)] + list(reset_values(rng, 6))
    return [(F32(h), F32(m), F32(v)) for h, m in pairs for v in vs]


def test_the_host_program_equals_the_exact_fma_bit_for_bit(host):
    cs = cases()
    got = host(["f %s %s %s" % (hexbits(h), hexbits(m), hexbits(v)) for h, m, v in cs])[:, 0]
    h, m, v = (np.array([c[i] for c in cs], F32) for i in range(3))
    want = R.fma32(h, v, m)
    bad = np.nonzero(got != R.bits(want))[0]
    assert bad.size == 0, [(cs[i], hex(got[i]), hex(int(R.bits(want[i])))) for i in bad[:5]]
    for i in range(0, len(cs), 5):   # ... and the vectorised form against the rationals
        assert R.bits(R.fma32_exact(cs[i][0], cs[i][2], cs[i][1])) == got[i], cs[i]
    # the single rounding is not decoration: a product and a sum rounded separately differ somewhere on this set
    naive = (h * v + m).astype(F32)
    assert (R.bits(naive) != got).any()


def test_the_identity_returns_every_value_of_the_reset_stream(host):
    """lo = -1, hi = 1 gives h = 1, m = 0, and fma(1, v, 0) has the bits of v for ALL 2^24 values of v"""
    h, m = R.coeffs(F32(-1.0), F32(1.0))
    assert (R.bits(h), R.bits(m)) == (0x3F800000, 0x00000000)
    bad, vmin, vmax = host(["i %s %s" % (hexbits(h), hexbits(m))], 3)[0]
    assert bad == 0
    assert (vmin, vmax) == (R.bits(V_MIN), R.bits(V_MAX)), "the loop covered the range the contract states"
    # ... and the program can tell: another h is no identity
    assert host(["i %s %s" % (hexbits(F32(0.5)), hexbits(m))], 3)[0][0] > 0
    rng = np.random.RandomState(4)
    v = reset_values(rng, 1000)
    assert np.array_equal(R.bits(R.map_state(F32(-1.0), F32(1.0), v)), R.bits(v))


def test_a_pinned_component_is_its_value_at_both_ends(host):
    for val in (F32(0.25), F32(-3.5), F32(0.0), F32(1e-30), F32(123456.789)):
        h, m = R.coeffs(val, val)
        assert R.bits(h) == 0 and R.bits(m) == R.bits(val)
        got = host(["f %s %s %s" % (hexbits(h), hexbits(m), hexbits(v)) for v in (V_MIN, V_MAX, F32(0.0))])[:, 0]
        assert (got == R.bits(val)).all(), (val, got)
        assert (R.bits(R.map_state(val, val, np.array([V_MIN, V_MAX], F32))) == R.bits(val)).all()


def test_a_span_whose_midpoint_is_not_representable(host):
    """lo = 1, hi = 1 + 2^-23: the midpoint 1 + 2^-24 is a tie of fp32 - m rounds to even once, h = 2^-24 exactly - and every state the map
    gives lies inside [lo, hi]"""
    lo, hi = F32(1.0), F32(1.0 + 2.0 ** -23)
    h, m = host(["d %s %s" % (hexbits(lo), hexbits(hi))], 2)[0]
    assert (h, m) == (R.bits(F32(2.0 ** -24)), R.bits(F32(1.0)))
    assert (h, m) == tuple(int(R.bits(x)) for x in R.coeffs(lo, hi))
    rng = np.random.RandomState(5)
    vs = [V_MIN, V_MAX, F32(0.0)] + list(reset_values(rng, 50))
    got = R.from_bits(host(["f %08x %08x %s" % (h, m, hexbits(v)) for v in vs])[:, 0])
    assert np.array_equal(R.bits(got), R.bits(R.map_state(lo, hi, np.array(vs, F32))))
    # the statement is the fma of the ROUNDED h and m, not a clamp: with m rounded down to lo, v = -1 gives lo - h = 1 - 2^-24, one
    # fp32 value below lo - the most a state can leave its range by is this rounding of m (half an ulp of the larger bound)
    assert got[0] == F32(1.0 - 2.0 ** -24) and ((got >= F32(1.0 - 2.0 ** -24)) & (got <= hi)).all()
    # a wide span whose sum is not representable either: the fp64 sum is exact, one rounding
    lo, hi = F32(-0.1), F32(16777216.0)
    h, m = host(["d %s %s" % (hexbits(lo), hexbits(hi))], 2)[0]
    assert (h, m) == tuple(int(R.bits(x)) for x in R.coeffs(lo, hi))
    assert R.from_bits(m) == F32((float(hi) + float(lo)) / 2)


def test_the_derivation_matches_the_python_class(host, built):
    from gym_reinmav_amd import StartState, _abi as A

    rng = np.random.RandomState(6)
    for kind in KINDS:
        k, nS = A.KIND_BY_NAME[kind], NS[kind]
        for lo, hi in (R.ranges(kind), R.identity(kind), (np.sort(rng.uniform(-2, 2, (2, nS)), axis=0) * 10.0 ** rng.uniform(-2, 2, nS))):
            st = StartState(tuple(float(x) for x in lo), tuple(float(x) for x in hi))
            s = st.spec(k)
            assert ctypes.sizeof(s) == 128
            assert np.array_equal(R.bits(np.array(s.lo[:nS], F32)), R.bits(np.asarray(lo, F32))) and not any(s.lo[nS:]) and not any(s.hi[nS:])
            h, m = st.coefficients(k)
            hr, mr = R.coeffs(lo, hi)
            assert np.array_equal(R.bits(h), R.bits(hr)) and np.array_equal(R.bits(m), R.bits(mr))
            got = host(["d %s %s" % (hexbits(a), hexbits(b)) for a, b in zip(s.lo[:nS], s.hi[:nS])], 2)
            assert np.array_equal(got[:, 0], R.bits(hr)) and np.array_equal(got[:, 1], R.bits(mr))


def test_start_states_of_the_restatement(built):
    import oracle as O

    kind, ids = "quad3d", np.array([300, 301, 2 ** 33 + 5])
    lo, hi = R.ranges(kind)
    s = R.start_states(kind, 11, ids, [1, 2, 0], lo, hi)
    assert s.shape == (3, NS[kind]) and s.dtype == F32
    assert ((s >= lo) & (s <= hi)).all() and (s[:, 1] == F32(0.25)).all() and (s[:, 2] > 0).all()
    v = O.reset_states(kind, 11, ids, [1, 2, 0])
    assert np.array_equal(R.bits(R.start_states(kind, 11, ids, [1, 2, 0], *R.identity(kind))), R.bits(v))
    for c in (0, 5):
        assert R.bits(R.fma32_exact(R.coeffs(lo, hi)[0][c], v[2, c], R.coeffs(lo, hi)[1][c])) == R.bits(s[2, c])


def test_the_python_class_and_check_start_state(built):
    from gym_reinmav_amd import StartState, _abi as A, check_start_state

    q3, q2 = A.KIND_BY_NAME["quad3d"], A.KIND_BY_NAME["quad2d"]
    a = StartState(-0.5, 0.5)
    s = a.spec(q3)
    assert list(s.lo) == [-0.5] * 10 + [0.0] * 6 and list(s.hi) == [0.5] * 10 + [0.0] * 6
    assert list(a.spec(q2).hi) == [0.5] * 5 + [0.0] * 11
    b = StartState((-1, -2, -3, -4, -5), 1.0)
    assert list(b.spec(q2).lo)[:5] == [-1.0, -2.0, -3.0, -4.0, -5.0] and list(b.spec(q2).hi)[:5] == [1.0] * 5
    back = StartState.from_spec(b.spec(q2), q2)
    assert back.lo == (-1.0, -2.0, -3.0, -4.0, -5.0) and back.hi == (1.0,) * 5 and repr(back).startswith("StartState(lo=")
    pinned = StartState(0.25, 0.25)
    assert pinned.coefficients(q2)[0].tolist() == [0.0] * 5
    ar = StartState.around((0.0, 0.0, 1.0, 0.0, 0.0), 0.5)
    assert ar.lo == (-0.5, -0.5, 0.5, -0.5, -0.5) and ar.hi == (0.5, 0.5, 1.5, 0.5, 0.5)
    ar = StartState.around(np.arange(5.0), (0.0, 0.1, 0.2, 0.3, 0.4))
    assert ar.lo[0] == ar.hi[0] == 0.0 and ar.hi[4] == 4.4
    assert StartState.parse("-0.5:0.5").lo == -0.5 and StartState.parse("-1:1,0:2,3:3,-4:4,0:0").hi == (1.0, 2.0, 3.0, 4.0, 0.0)
    for bad in (None, "0.1", True, [0.1, "x"], object()):
        with pytest.raises(TypeError):
            StartState(bad, 1.0)
        with pytest.raises(TypeError):
            StartState(-1.0, bad)
    for lo, hi in ((1.0, 0.5), (float("nan"), 1.0), (0.0, float("inf")), (-1e39, 0.0), ((), 1.0), ((0.0,) * 17, 1.0), ((0.0, 2.0), (1.0, 1.0)),
                   ((0.0,) * 5, (1.0,) * 9)):
        with pytest.raises(ValueError):
            StartState(lo, hi)
    for text in ("1", "1:2:3", "a:b", "1:2,3"):
        with pytest.raises(ValueError):
            StartState.parse(text)
    with pytest.raises(ValueError):
        StartState.around((0.0,) * 5, -0.1)
    with pytest.raises(ValueError):
        StartState.around((0.0,) * 5, (0.1,) * 4)
    with pytest.raises(ValueError):
        b.spec(q3)                                   # 5 components, a 10-component kind
    with pytest.raises(ValueError):
        a.spec(A.REINMAV)
    assert check_start_state(None) is None and check_start_state(a, q3) is a
    with pytest.raises(ValueError):
        check_start_state(b, q3)
    for bad in (0.5, (-1.0, 1.0), "x"):
        with pytest.raises(TypeError):
            check_start_state(bad)


def test_the_example_has_the_flag():
    src = open(os.path.join(ROOT, "examples", "train_ppo2.py")).read()
    assert '"--start-state"' in src and "g.StartState.parse(args.start_state)" in src and src.count("start_state=start_state") == 2

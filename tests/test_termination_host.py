"""Termination rules (rmav_set_termination), what can be checked without a GPU: the kernels' rule (csrc/rmav_term.hpp, compiled for the host
as the stand-alone program tests/term_host) decides what the numpy restatement tests/term_ref.py decides, on a table of the edges where it
can go wrong - every bound at and one ulp either side of lo and hi, -0.0 against a bound of 0, NaN and +-inf in every component in turn, the
load outside while the quadrotor is inside and the reverse, |theta| at and one ulp either side of max_tilt (large unwrapped angles too),
quaternions at max_tilt in {0, pi/2, pi, +inf}, unnormalised ones and the zero quaternion, random quaternions within a few ulps of the
threshold; the identity spec decides "no" on 10^5 finite random states; Termination.spec() round-trips; the class and check_termination
validate their arguments; the example has the flag."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import term_ref as R
from util import KINDS, NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DIR = os.path.join(ROOT, "tests", "term_host")
sys.path.insert(0, os.path.join(ROOT, "reinmav-gym_amd"))

F32 = np.float32
INF, NAN = F32(np.inf), F32(np.nan)
PI = F32(math.pi)


def hexbits(x):
    return "%08x" % int(R.bits(F32(x)))


@pytest.fixture(scope="module")
def host():
    subprocess.run(["make", "-s", "-C", HOST_DIR], check=True)
    exe = os.path.join(HOST_DIR, "_build", "term_host")

    def run(cases):
        """cases: (kind, pos_lo[3], pos_hi[3], max_tilt, s[nS]) -> (decisions, bits of the seventh threshold)"""
        lines = []
        for kind, lo, hi, mt, s in cases:
            assert len(s) == NS[kind]
            lines.append(" ".join([str(KINDS.index(kind))] + [hexbits(v) for v in (*lo, *hi, mt, *s)]))
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split()
        assert len(out) == 2 * len(cases), (len(out), len(cases))
        return np.array([int(x) for x in out[0::2]], bool), np.array([int(x, 16) for x in out[1::2]], np.uint64).astype(np.uint32)

    return run


def want(cases):
    return np.array([R.rule(kind, np.asarray(s, F32)[None], lo[:R.DIM[kind]], hi[:R.DIM[kind]], mt)[0] for kind, lo, hi, mt, s in cases], bool)


def check(host, cases, expect=None):
    got, tilt = host(cases)
    ref = want(cases)
    bad = np.nonzero(got != ref)[0]
    assert bad.size == 0, [(cases[i], bool(got[i]), bool(ref[i])) for i in bad[:5]]
    for i, (kind, lo, hi, mt, s) in enumerate(cases):   # the host's seventh threshold: max_tilt itself (2-D), the rounded fp64 cosine (3-D)
        assert tilt[i] == R.bits(F32(mt) if R.DIM[kind] == 2 else R.cos_tilt(mt)), (kind, mt, hex(tilt[i]))
    if expect is not None:
        assert list(ref) == list(expect), (list(ref), list(expect))
    return ref


def calm(kind):
    """a state every spec of these tests leaves alone: at the origin, upright, at rest"""
    s = np.zeros(NS[kind], F32)
    if R.DIM[kind] == 3:
        s[3] = 1.0
    return s


def unbounded():
    return np.full(3, -np.inf, F32), np.full(3, np.inf, F32)


def up_down(v):
    return [F32(v), np.nextafter(F32(v), -INF), np.nextafter(F32(v), INF)]


@pytest.mark.parametrize("kind", KINDS)
def test_every_bound_at_and_one_ulp_either_side(host, kind):
    d = R.DIM[kind]
    bodies = [0] + ([R.LOAD[kind]] if R.LOAD[kind] is not None else [])
    cases, expect = [], []
    for b in (F32(0.3), F32(-2.0), F32(0.0), F32(1e-38), F32(123456.0)):
        for axis in range(d):
            for body in bodies:
                for side in ("lo", "hi"):
                    lo, hi = unbounded()
                    (lo if side == "lo" else hi)[axis] = b
                    at, below, above = up_down(b)
                    for v, ends in ((at, False), (below, side == "lo"), (above, side == "hi")):
                        s = calm(kind)
                        for other in bodies:                     # (every body on the bound, which is inside; then the one under test)
                            s[other + axis] = b
                        s[body + axis] = v
                        cases.append((kind, lo, hi, INF, s)), expect.append(ends)
    # -0.0 against a bound of 0, from both sides: -0.0 >= 0 and -0.0 <= 0 both hold
    for axis in range(d):
        for side in ("lo", "hi"):
            for zero in (F32(0.0), F32(-0.0)):
                for v in (F32(0.0), F32(-0.0)):
                    lo, hi = unbounded()
                    (lo if side == "lo" else hi)[axis] = zero
                    s = calm(kind)
                    s[axis] = v
                    cases.append((kind, lo, hi, INF, s)), expect.append(False)
    # lo == hi: the one value stays
    lo, hi = np.full(3, 0.5, F32), np.full(3, 0.5, F32)
    s = calm(kind)
    s[:d] = 0.5
    if R.LOAD[kind] is not None:
        s[R.LOAD[kind]:R.LOAD[kind] + d] = 0.5
    cases.append((kind, lo, hi, INF, s)), expect.append(False)
    s = s.copy()
    s[0] = np.nextafter(F32(0.5), INF)
    cases.append((kind, lo, hi, INF, s)), expect.append(True)
    check(host, cases, expect)


@pytest.mark.parametrize("kind", KINDS)
def test_nan_and_inf_in_every_component_in_turn(host, kind):
    cases, expect = [], []
    box = (np.array([-2, -2, -2], F32), np.array([2, 2, 2], F32))
    for lo, hi in (unbounded(), box):
        for mt in (INF, F32(1.0)):
            for c in range(NS[kind]):
                for v in (NAN, INF, -INF, R.from_bits(np.uint32(0xFFC00001))):
                    s = calm(kind)
                    s[c] = v
                    cases.append((kind, lo, hi, mt, s)), expect.append(True)
            cases.append((kind, lo, hi, mt, calm(kind))), expect.append(False)
            big = calm(kind)                                         # the largest finite value is finite: only a bound ends it
            big[NS[kind] - 1] = np.finfo(F32).max
            cases.append((kind, lo, hi, mt, big)), expect.append(False)
    check(host, cases, expect)


@pytest.mark.parametrize("kind", ("quad2d_sl", "quad3d_sl"))
def test_the_load_outside_while_the_quadrotor_is_inside_and_the_reverse(host, kind):
    d, L = R.DIM[kind], R.LOAD[kind]
    lo, hi = np.full(3, -1.0, F32), np.full(3, 1.0, F32)
    lo[d - 1] = 0.3     # a floor on the last axis
    cases, expect = [], []
    for quad_in in (True, False):
        for load_in in (True, False):
            for axis in range(d):
                s = calm(kind)
                s[d - 1] = s[L + d - 1] = 0.5
                if not quad_in:
                    s[axis] = 1.5 if axis < d - 1 else 0.25
                if not load_in:
                    s[L + axis] = -1.5 if axis < d - 1 else 0.25
                cases.append((kind, lo, hi, INF, s)), expect.append(not (quad_in and load_in))
    check(host, cases, expect)


@pytest.mark.parametrize("kind", ("quad2d", "quad2d_sl"))
def test_the_2d_tilt_at_and_one_ulp_either_side(host, kind):
    cases, expect = [], []
    for mt in (F32(0.0), F32(1.2), PI, F32(0.5)):
        at, below, above = up_down(mt)
        for sign in (1, -1):
            for v, ends in ((at, False), (above, True)) + (((below, False),) if mt > 0 else ()):
                s = calm(kind)
                s[2] = sign * v
                cases.append((kind, *unbounded(), mt, s)), expect.append(ends)
    for theta in (F32(7.0), F32(-100.0), F32(2 * math.pi), F32(1e6)):   # the angle is never wrapped: 2 pi is a tilt of 2 pi
        for mt, ends in ((PI, True), (INF, False), (F32(abs(theta)), False)):
            s = calm(kind)
            s[2] = theta
            cases.append((kind, *unbounded(), mt, s)), expect.append(ends)
    check(host, cases, expect)


def quat(angle, axis_angle=0.3, scale=1.0):
    """a quaternion (w, x, y, z) whose body z axis is tilted by `angle`, about a horizontal axis at `axis_angle`, times a yaw - fp64"""
    ha = 0.5 * angle
    q = np.array([math.cos(ha), math.sin(ha) * math.cos(axis_angle), math.sin(ha) * math.sin(axis_angle), 0.0])
    yaw = np.array([math.cos(0.35), 0.0, 0.0, math.sin(0.35)])
    w1, x1, y1, z1 = q
    w2, x2, y2, z2 = yaw
    out = np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                    w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])
    return (out * scale).astype(F32)


@pytest.mark.parametrize("kind", ("quad3d", "quad3d_sl"))
def test_the_3d_tilt(host, kind):
    cases = []
    rng = np.random.RandomState(5)

    def add(mt, q):
        s = calm(kind)
        s[3:7] = q
        cases.append((kind, *unbounded(), F32(mt), s))

    for mt in (F32(0.0), F32(math.pi / 2), PI, INF, F32(1.2), F32(0.3)):
        for scale in (1.0, 1e-3, 1e3, 1e-20, 1e18):
            for angle in (0.0, 0.2, 1.2, math.pi / 2, 3.0, math.pi) + ((float(mt),) if mt < INF else ()):
                add(mt, quat(angle, scale=scale))
        add(mt, np.zeros(4, F32))                                        # the zero quaternion
        add(mt, np.array([0, 0, 0, -0.0], F32))
        add(mt, np.array([1, 0, 0, 0], F32)), add(mt, np.array([0, 1, 0, 0], F32)), add(mt, np.array([0, 0, 1, 0], F32)), add(mt, np.array([0, 0, 0, 1], F32))
        add(mt, np.array([np.finfo(F32).max, 0, 0, 0], F32))            # |q|^2 overflows: inf against c * inf
        add(mt, np.array([0, np.finfo(F32).max, 0, 0], F32))
    # random quaternions within a few ulps of the threshold: tilt angle = max_tilt, components nudged by up to 3 ulps
    for mt in (F32(1.2), F32(0.3), F32(math.pi / 2), F32(2.5)):
        for _ in range(150):
            q = quat(float(mt), axis_angle=rng.uniform(0, 2 * math.pi), scale=10.0 ** rng.uniform(-3, 3))
            u = R.bits(q).astype(np.int64) + rng.randint(-3, 4, 4)
            add(mt, R.from_bits(u.astype(np.uint32)))
    ref = check(host, cases)
    near = ref[-600:]
    assert 100 < near.sum() < 500, "the nudged quaternions fall on both sides of the threshold"
    # what the rule means: upright never ends below pi, inverted ends for every limit below pi, nothing ends without a limit
    up, down = calm(kind), calm(kind)
    down[3:7] = (0, 1, 0, 0)
    assert not R.rule(kind, up[None], max_tilt=0.0)[0] and R.rule(kind, down[None], max_tilt=3.0)[0] and not R.rule(kind, down[None], max_tilt=None)[0]
    assert not R.rule(kind, down[None], max_tilt=PI)[0], "cos(pi as fp32) rounds to -1: a tilt of pi is the limit itself"


@pytest.mark.parametrize("kind", KINDS)
def test_the_identity_spec_decides_no_on_finite_states(host, kind):
    rng = np.random.RandomState(9)
    n = 100000
    s = (rng.standard_normal((n, NS[kind])) * 10.0 ** rng.uniform(-6, 6, (n, NS[kind]))).astype(F32)
    s[::7, :3] = 0.0
    if R.DIM[kind] == 3:
        s[::11, 3:7] = 0.0
    assert np.isfinite(s).all()
    assert not R.rule(kind, s).any()
    lo, hi = unbounded()
    got, _ = host([(kind, lo, hi, INF, row) for row in s[:2000]])
    assert not got.any()
    # the extremes of fp32 are finite too
    s[:, :] = np.finfo(F32).max
    s[1::2] *= -1
    got, _ = host([(kind, lo, hi, INF, row) for row in s[:4]])
    assert not got.any() and not R.rule(kind, s[:4]).any()


def test_the_python_class_and_check_termination(built):
    from gym_reinmav_amd import Termination, _abi as A, check_termination
    import ctypes as C

    q2, q3, q3s = A.KIND_BY_NAME["quad2d"], A.KIND_BY_NAME["quad3d"], A.KIND_BY_NAME["quad3d_sl"]
    assert C.sizeof(A.TerminationSpec) == 32
    ident = Termination()
    s = ident.spec(q3)
    assert list(s.pos_lo) == [-math.inf] * 3 and list(s.pos_hi) == [math.inf] * 3 and s.max_tilt == math.inf and s._reserved == 0
    hover = Termination(pos_lo=(-2, -2, 0.3), pos_hi=(2, 2, math.inf))
    s = hover.spec(q3s)
    assert list(s.pos_lo) == [-2.0, -2.0, float(F32(0.3))] and list(s.pos_hi) == [2.0, 2.0, math.inf]
    back = Termination.from_spec(s, q3s)
    assert back.pos_lo == (-2.0, -2.0, float(F32(0.3))) and back.pos_hi == (2.0, 2.0, math.inf) and back.max_tilt == math.inf
    assert repr(back).startswith("Termination(pos_lo=")
    # a scalar broadcasts over the axes; the third axis of a 2-D kind is unbounded
    b = Termination(pos_lo=-1.5, pos_hi=2, max_tilt=1.2)
    s = b.spec(q2)
    assert list(s.pos_lo) == [-1.5, -1.5, -math.inf] and list(s.pos_hi) == [2.0, 2.0, math.inf] and s.max_tilt == float(F32(1.2))
    assert list(b.spec(q3).pos_lo) == [-1.5] * 3
    assert Termination(max_tilt=math.pi).spec(q3).max_tilt == float(PI) and Termination(max_tilt=float(PI)).max_tilt == float(PI)
    assert Termination(max_tilt=0).max_tilt == 0.0 and Termination(max_tilt=math.inf).max_tilt == math.inf
    p = Termination.parse("box=-2:2,-2:2,0.3:inf:tilt=1.2")
    assert p.pos_lo == (-2.0, -2.0, 0.3) and p.pos_hi == (2.0, 2.0, math.inf) and p.max_tilt == 1.2
    p = Termination.parse("tilt=0.5")
    assert p.pos_lo == -math.inf and p.max_tilt == 0.5
    p = Termination.parse("box=-1:1,0:inf")
    assert p.pos_lo == (-1.0, 0.0) and p.max_tilt == math.inf
    for text in ("", "box", "box=1", "box=1:2:3,1:2", "tilt=x", "box=-2:2,-2:2;tilt=1", "floor=0.3", "tilt=1.2:junk"):
        with pytest.raises(ValueError):
            Termination.parse(text)
    for bad in (dict(pos_lo=float("nan")), dict(pos_hi=(1.0, float("nan"))), dict(pos_lo=1.0, pos_hi=0.5), dict(pos_lo=(0, 0, 1), pos_hi=(1, 1, 0.5)),
                dict(max_tilt=-0.1), dict(max_tilt=3.2), dict(max_tilt=float("nan")), dict(pos_lo=(1,)), dict(pos_lo=(0, 0, 0, 0)),
                dict(pos_lo=(0, 0), pos_hi=(1, 1, 1))):
        with pytest.raises(ValueError):
            Termination(**bad)
    for bad in (dict(pos_lo="1"), dict(pos_hi=True), dict(max_tilt="1"), dict(pos_lo=(None, 1.0)), dict(max_tilt=(1.0,))):
        with pytest.raises(TypeError):
            Termination(**bad)
    with pytest.raises(ValueError):
        hover.spec(q2)                                   # three axes for a 2-D kind
    with pytest.raises(ValueError):
        ident.spec(A.REINMAV)
    assert check_termination(None) is None and check_termination(hover, q3) is hover
    with pytest.raises(ValueError):
        check_termination(hover, q2)
    for bad in (1.0, "box", (0, 1), {"pos_lo": 0}):
        with pytest.raises(TypeError):
            check_termination(bad)
    # the example has the flag and hands it to both constructors
    src = open(os.path.join(ROOT, "examples", "train_ppo2.py")).read()
    assert '"--termination"' in src and "g.Termination.parse(args.termination)" in src and src.count("termination=termination") == 2

"""Actuator lag (rmav_set_actuator), what can be checked without a GPU: the kernels' filter statement and the host's derivation of its
coefficients (csrc/rmav_actuator.hpp, compiled for the host as the stand-alone program tests/actuator_host) equal the numpy restatement
tests/actuator_ref.py bit for bit - at the edges of alpha, m and u and at 200 random cases; the restatement's two forms of the exact fma
agree; tau = 0 returns the command; the rule converges to a constant command; the derivation matches for every kind's default dt; the
Python class validates its arguments; the example has the flag."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import actuator_ref as R
from util import KINDS, NA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DIR = os.path.join(ROOT, "tests", "actuator_host")
sys.path.insert(0, os.path.join(ROOT, "reinmav-gym_amd"))

F32 = np.float32
FLT_MAX = np.finfo(F32).max
TINY = np.finfo(F32).tiny                      # the smallest normal
DENORM = F32(1.401298464324817e-45)            # the smallest denormal
ONE_M = F32(1.0 - 2.0 ** -24)                  # 1 - 2^-24, the fp32 value below 1

# m and u at +-0, denormals, +-FLT_MAX / 2 and ordinary values of both signs
VALUES = [F32(0.0), F32(-0.0), DENORM, -DENORM, F32(TINY / 4), F32(-TINY / 4), F32(FLT_MAX / 2), F32(-FLT_MAX / 2), F32(1.0), F32(-1.0), F32(9.8),
          F32(-0.3)]
# (alpha, beta): no lag; alpha at the smallest normal and at 1 - 2^-24 with the beta next to 1 - alpha; an ordinary pair
COEFFS = [(F32(1.0), F32(0.0)), (F32(TINY), F32(1.0)), (F32(TINY), ONE_M), (ONE_M, F32(2.0 ** -24)), (ONE_M, DENORM), (F32(0.18126924), F32(0.81873076))]


def hexbits(x):
    return "%08x" % int(R.bits(F32(x)))


@pytest.fixture(scope="module")
def host():
    subprocess.run(["make", "-s", "-C", HOST_DIR], check=True)
    exe = os.path.join(HOST_DIR, "_build", "actuator_host")

    def run(lines, width=1):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split()
        assert len(out) == width * len(lines), (len(out), len(lines))
        return np.array([int(x, 16) for x in out], np.uint64).astype(np.uint32).reshape(len(lines), width)

    return run


def edge_cases():
    cases = [(a, b, m, u) for a, b in COEFFS for m in VALUES for u in VALUES]
    cases += [(a, b, F32(FLT_MAX / 2), F32(-FLT_MAX / 2)) for a, b in COEFFS] + [(a, b, F32(-FLT_MAX / 2), F32(FLT_MAX / 2)) for a, b in COEFFS]
    return cases


def random_cases(n=200, seed=20):
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        tau = 10.0 ** rng.uniform(-3, 0)
        a, b = R.coeffs(tau, 10.0 ** rng.uniform(-3, -1))
        scale = 10.0 ** rng.uniform(-6, 6) if i % 4 == 0 else 10.0
        out.append((a, b, F32(rng.uniform(-1, 1) * scale), F32(rng.uniform(-1, 1) * scale)))
    return out


def test_the_two_forms_of_the_exact_fma_agree():
    """fma32 (round to odd in fp64, vectorised) against fma32_exact (rationals) where a double-rounded fp64 sum goes wrong, and everywhere else"""
    cases = [(a, u, F32(b * m)) for a, b, m, u in edge_cases() + random_cases()]
    # a tie of the fp64 sum that the exact sum breaks: 1 + 2^-24 (half an fp32 ulp) + a product far below the fp64 ulp
    cases += [(F32(2.0 ** -60), F32(2.0 ** -60), F32(1.0)), (F32(2.0 ** -30), F32(2.0 ** -30 + 2.0 ** -50), F32(1.0 + 2.0 ** -23)),
              (F32(1.0 + 2.0 ** -23), F32(2.0 ** -24), F32(1.0)), (F32(-(1.0 + 2.0 ** -23)), F32(2.0 ** -24), F32(1.0)),
              (F32(1.0 + 2.0 ** -12), F32(1.0 + 2.0 ** -12), F32(2.0 ** -60)), (F32(1.0 + 2.0 ** -12), F32(1.0 + 2.0 ** -12), F32(-2.0 ** -60))]
    a, b, c = (np.array([x[i] for x in cases], F32) for i in range(3))
    fast = R.fma32(a, b, c)
    for i, (x, y, z) in enumerate(cases):
        want = R.fma32_exact(x, y, z)
        assert R.bits(fast[i]) == R.bits(want), (x, y, z, fast[i], want)
    # the double-rounded fp64 sum does differ on this set: the exactness is not decoration
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
    assert (R.bits(naive) != R.bits(fast)).any()


def test_the_host_program_equals_the_restatement_bit_for_bit(host):
    cases = edge_cases() + random_cases()
    for tag in "fv":   # the statement itself, and through actuator_step<4>
        got = host(["%s %s %s %s %s" % ((tag,) + tuple(hexbits(x) for x in c)) for c in cases])[:, 0]
        a, b, m, u = (np.array([c[i] for c in cases], F32) for i in range(4))
        want = R.filt(a, b, m, u)
        bad = np.nonzero(got != R.bits(want))[0]
        assert bad.size == 0, (tag, [(cases[i], hex(got[i]), hex(int(R.bits(want[i])))) for i in bad[:5]])
    for c in cases[::7]:
        assert R.bits(R.filt_exact(*c)) == R.bits(R.filt(*c)), c


def test_tau_zero_returns_the_command(host):
    alpha, beta = R.coeffs(0.0, 0.01)
    assert (alpha, beta) == (F32(1.0), F32(0.0))
    us = [v for v in VALUES] + [F32(3.25), F32(-7.5)]
    for m in (F32(0.0), F32(5.0), F32(-FLT_MAX / 2), DENORM):
        got = host(["f %s %s %s %s" % (hexbits(alpha), hexbits(beta), hexbits(m), hexbits(u)) for u in us])[:, 0]
        for u, g in zip(us, got):
            # the bits of u - but for a zero command, whose sign follows IEEE's sum of zeros (0 * m keeps m's sign)
            if float(u) == 0.0:
                assert R.from_bits(g) == 0.0
            else:
                assert g == R.bits(u), (m, u, hex(g))
        assert np.array_equal(R.bits(R.filt(alpha, beta, m, np.array(us, F32))), got)


def test_iterating_the_rule_converges_to_a_constant_command():
    for tau, dt in ((0.05, 0.01), (0.5, 0.02), (0.005, 0.01)):
        alpha, beta = R.coeffs(tau, dt)
        for u, m0 in ((F32(9.8), F32(0.0)), (F32(-3.0), F32(10.0)), (F32(0.25), F32(0.25))):
            m = m0
            gap = abs(float(m) - float(u))
            for _ in range(int(40 * max(tau / dt, 1))):
                m = R.filt(alpha, beta, m, u)
                assert abs(float(m) - float(u)) <= gap + 1e-6 * abs(float(u))   # no overshoot beyond rounding
                gap = abs(float(m) - float(u))
            assert gap <= 4 * np.spacing(F32(abs(float(u)))) / float(alpha), (tau, dt, u, m0, m)


def test_the_derivation_matches_for_the_default_dt_of_every_kind(host, built):
    from gym_reinmav_amd import _abi as A

    taus = (0.0, 0.005, 0.02, 0.05, 0.3, 1e-6, 1e3)
    dts = sorted({float(A.default_params(A.KIND_BY_NAME[k]).dt) for k in KINDS} | {float(A.default_params(A.KIND_BY_NAME["quad2d"], "A").dt)})
    assert all(0 < dt < 1 for dt in dts)
    lines, want = [], []
    for dt in dts:
        for tau in taus:
            lines.append("d %s %016x" % (hexbits(tau), struct.unpack("<Q", struct.pack("<d", dt))[0]))
            want.append(R.coeffs(tau, dt))
    got = host(lines, 2)
    for ln, g, (a, b) in zip(lines, got, want):
        assert (g[0], g[1]) == (R.bits(a), R.bits(b)), (ln, g, a, b)
        assert 0.0 <= float(b) <= 1.0 and 0.0 <= float(a) <= 1.0
    # alpha + beta = 1 up to their two roundings
    for a, b in want:
        assert abs(float(a) + float(b) - 1.0) <= 2.0 ** -23


def test_the_episode_rule_of_the_restatement():
    lag = R.Lag(0.05, 0.01, (9.8, 0.0), 3)
    assert lag.m.shape == (3, 2) and np.array_equal(lag.m[:, 0], np.full(3, F32(9.8)))
    u = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]], F32)
    m1 = lag.step(u)
    assert np.array_equal(R.bits(m1), R.bits(R.filt(lag.alpha[None], lag.beta[None], np.tile(lag.init, (3, 1)), u)))
    m2 = lag.step(u, live=[True, False, True])          # a lane that has left the frame-skip loop keeps its m
    assert np.array_equal(m2[1], m1[1]) and not np.array_equal(m2[0], m1[0])
    lag.end_of_step([False, True, False])
    assert np.array_equal(lag.m[1], lag.init) and np.array_equal(lag.m[0], m2[0])
    lag.end_of_step([True, True, True], auto_reset=False)   # without auto-reset a finished env keeps filtering
    assert np.array_equal(lag.m[0], m2[0])
    lag.reset()
    assert np.array_equal(lag.m, np.tile(lag.init, (3, 1)))


def test_the_python_class(built):
    import ctypes

    from gym_reinmav_amd import Actuator, _abi as A
    from gym_reinmav_amd.core import check_actuator

    assert ctypes.sizeof(A.ActuatorSpec) == 32
    q3, q2 = A.KIND_BY_NAME["quad3d"], A.KIND_BY_NAME["quad2d_sl"]
    p3, p2 = A.default_params(q3), A.default_params(q2)
    a = Actuator(0.05)
    s = a.spec(q3, p3)
    assert list(s.tau) == [F32(0.05)] * 4
    hover = F32(np.float64(p3.mass) * float(np.sqrt(sum(float(x) ** 2 for x in p3.g_vec))) / np.float64(p3.thrust_scale))
    assert list(s.init) == [hover, 0.0, 0.0, 0.0] and hover > 0
    s2 = a.spec(q2, p2)
    assert list(s2.tau) == [F32(0.05), F32(0.05), 0.0, 0.0] and list(s2.init)[1:] == [0.0, 0.0, 0.0]
    # the hover action is the one TrackingReward(act_ref=None) resolves
    from gym_reinmav_amd import TrackingReward
    assert list(TrackingReward().spec(q2, p2).act_ref)[:2] == list(s2.init)[:2]
    b = Actuator((0.0, 0.1, 0.2, 0.3), init=(1.0, -2.0, 0.5, 0.0))
    sb = b.spec(q3, p3)
    assert list(sb.tau) == [F32(x) for x in (0.0, 0.1, 0.2, 0.3)] and list(sb.init) == [1.0, -2.0, 0.5, 0.0]
    back = Actuator.from_spec(sb, q3)
    assert back.init == (1.0, -2.0, 0.5, 0.0) and len(back.tau) == 4 and repr(back).startswith("Actuator(tau=")
    for bad in (None, "0.1", True, [0.1, "x"], object()):
        with pytest.raises(TypeError):
            Actuator(bad)
    for bad in (-0.1, float("nan"), float("inf"), 1e39, (), (0.1,) * 3, (0.1, -0.2), (0.1, float("nan"))):
        with pytest.raises(ValueError):
            Actuator(bad)
    for bad in ((1.0,), (1.0, float("inf")), (1.0, 2.0, 3.0)):
        with pytest.raises(ValueError):
            Actuator(0.1, init=bad)
    with pytest.raises(TypeError):
        Actuator(0.1, init=1.0)
    with pytest.raises(ValueError):
        b.spec(q2, p2)                                   # 4 components, a 2-action kind
    with pytest.raises(ValueError):
        Actuator((0.1, 0.1)).spec(q3, p3)
    with pytest.raises(ValueError):
        Actuator(0.1, init=(1.0, 2.0)).spec(q3, p3)
    with pytest.raises(ValueError):
        a.spec(A.REINMAV, p3)
    assert check_actuator(None) is None and check_actuator(a, q3) is a
    with pytest.raises(TypeError):
        check_actuator(0.05)


def test_the_example_has_the_flag():
    src = open(os.path.join(ROOT, "examples", "train_ppo2.py")).read()
    assert '"--actuator-tau"' in src and "g.Actuator(args.actuator_tau)" in src and src.count("actuator=actuator") == 2   # the training and the evaluation envs

"""Sensor noise (rmav_set_sensor_noise), what can be checked without a GPU: the counter / words part of the kernels' draw
(csrc/rmav_sensor.hpp, compiled for the host as the stand-alone program tests/sensor_host) equals the numpy restatement
tests/sensor_ref.py bit for bit at the edges of every counter and at the ends of the 24-bit uniforms; six mutants of the restatement
each leave its bound by more than a decade on the inputs of tests/test_gpu_sensor_noise.py; the moments of the restatement; the
Python class."""
import os
import subprocess
import sys

import numpy as np
import pytest

import disturbance_ref as D
import noise_edges as E
import oracle as O
import sensor_ref as R
from util import KINDS, NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DIR = os.path.join(ROOT, "tests", "sensor_host")
sys.path.insert(0, os.path.join(ROOT, "reinmav-gym_amd"))

EDGE_B = (0, 1, 2**32 - 1, 2**32, 2**32 + 1, 2**48 - 2, 2**48 - 1)
EDGE_ENV = (0, 2**32 - 1, 2**32, 2**40 + 12345, 2**63 + 7)
# what the GPU test draws at: its seed and env ids, the step counters of its observe() cases, sigma on every component
GPU_SEED, GPU_BASE, GPU_SIGMA = D.PARITY["seed"], D.PARITY["env_id_base"], 0.25
GPU_SIZES = (1, 63, 65, 130)
GPU_B = (0, 1, 8, 2**32 - 1, 2**32 + 1, 3 * 2**32, 2**48 - 2)
GPU_WIDE_BASE = 2**40 + 12345


@pytest.fixture(scope="module")
def host():
    subprocess.run(["make", "-s", "-C", HOST_DIR], check=True)
    exe = os.path.join(HOST_DIR, "_build", "sensor_host")

    def run(lines, width):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split()
        assert len(out) == width * len(lines), (len(out), len(lines))
        return np.array([int(x, 16) for x in out], np.uint64).reshape(len(lines), width)

    return run


def test_the_words_and_uniforms_equal_the_restatement_bit_for_bit(host):
    rng = np.random.RandomState(7)
    cases = [(11, env, b, j) for b in EDGE_B for env in EDGE_ENV for j in range(4)]
    cases += [(2**64 - 3, 2**40 + 1, b, j) for b in EDGE_B for j in range(4)]
    cases += [(int(rng.randint(0, 2**62)), int(rng.randint(0, 2**62)), int(rng.randint(0, 2**47)), int(rng.randint(0, 4))) for _ in range(200)]
    got = host(["c %x %x %x %x" % c for c in cases], 8)
    for c, g in zip(cases, got):
        r = R.words(*c)
        assert np.array_equal(g[:4], r), (c, g[:4], r)
        assert np.array_equal(g[4:].astype(np.uint32), R.uniform_bits(r)), (c, g[4:], R.uniform_bits(r))
    # j and the high half of b reach the counter: neighbours differ
    a, b, c = host(["c b 5 7 0", "c b 5 7 1", "c b 5 100000007 0"], 8)
    assert not np.array_equal(a[:4], b[:4]) and not np.array_equal(a[:4], c[:4])


def test_the_ends_of_the_24_bit_uniforms(host):
    """The top-24-bit values tests/noise_edges.py lists for the policy's draw (the sensor stream has counters of its own, so the words
    are fed directly): u1 = 2^-24 .. 1 is never 0, u2 = 0 .. 1 - 2^-24 never 1, both exact."""
    tops = sorted({e[2] for e in E.EDGES + E.EDGES_WIDE_ENV + E.EDGES_LATE_T})
    assert {0x000000, 0xFFFFFF, 0xFFFFFE, 0x400000, 0x800000, 0xC00000} <= set(tops)
    lines, words = [], []
    for t in tops:
        for low in (0x00, 0xFF):   # the low byte is dropped
            r = [(t << 8) | low] * 4
            words.append(r)
            lines.append("w %x %x %x %x" % tuple(r))
    got = host(lines, 4).astype(np.uint32)
    assert np.array_equal(got, R.uniform_bits(np.array(words, np.uint64)))
    u = got.view(np.float32)
    assert (u[:, 0::2] > 0).all() and (u[:, 0::2] <= 1).all() and (u[:, 1::2] >= 0).all() and (u[:, 1::2] < 1).all()
    assert u[0, 0] == np.float32(2.0**-24) and u[-1, 0] == 1.0 and u[0, 1] == 0.0 and u[-1, 1] == np.float32(1 - 2.0**-24)


def gpu_inputs():
    """(kind, env ids, b, states) of the GPU test's observe() cases: fresh states of the oracle's reset."""
    for kind in KINDS:
        for n in GPU_SIZES:
            for base in (GPU_BASE, GPU_WIDE_BASE):
                ids = base + np.arange(n)
                s = O.reset_states(kind, GPU_SEED, ids, 0).astype(np.float32)
                for b in GPU_B:
                    yield kind, ids, b, s


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_leaves_the_bound_by_more_than_a_decade(mutant):
    worst = 0.0
    for kind, ids, b, s in gpu_inputs():
        sigma = np.full(NS[kind], GPU_SIGMA)
        o, bound = R.o_ref(sigma, GPU_SEED, ids, b, s)
        m, _ = R.o_ref(sigma, GPU_SEED, ids, b, s, mutant=mutant)
        worst = max(worst, float((np.abs(m - o) / bound).max()))
    assert worst > 10.0, (mutant, worst)


def test_the_restatement_is_inside_its_own_bound_in_fp32():
    """o_ref rounded to fp32 is what a correctly rounded implementation would store: far inside the bound (the bound is not vacuous the
    other way round either: it is a few ulps of |o|)."""
    for kind, ids, b, s in gpu_inputs():
        o, bound = R.o_ref(np.full(NS[kind], GPU_SIGMA), GPU_SEED, ids, b, s)
        assert (np.abs(o.astype(np.float32).astype(np.float64) - o) <= bound / 4).all()
        assert (bound <= 64 * 2.0**-24 * np.maximum(np.abs(o), GPU_SIGMA * 6)).all()


def test_moments_of_the_restatement():
    """4096 envs at one step counter, per component: |mean z| <= 5/64 and |std z - 1| <= 5/sqrt(8192), five standard errors each.
    MOMENT_SEED is chosen so that this passes; the GPU test reuses it."""
    z, _ = R.z_ref(R.MOMENT_SEED, np.arange(R.MOMENT_N), 5, 16)
    assert (np.abs(z.mean(0)) <= R.MEAN_CAP).all(), z.mean(0)
    assert (np.abs(z.std(0) - 1.0) <= R.STD_CAP).all(), z.std(0)
    # blocks and components are not copies of each other
    c = np.corrcoef(z.T)
    assert (np.abs(c - np.eye(16)) <= 5.0 / 64.0).all()


def test_the_python_class():
    from gym_reinmav_amd import _abi as A
    from gym_reinmav_amd.core import SensorNoise, check_sensor_noise

    q3 = A.KIND_BY_NAME["quad3d"]
    sn = SensorNoise(0.25)
    assert list(sn.spec(q3).sigma) == [0.25] * 10 + [0.0] * 6 and C_sizeof(A) == 64
    assert SensorNoise.parse("0.01").sigma == 0.01 and repr(SensorNoise.parse("0.01")) == "SensorNoise(sigma=0.01)"
    five = SensorNoise.parse("0.5,0,0.25,0.125,1")
    assert five.sigma == (0.5, 0.0, 0.25, 0.125, 1.0)
    assert list(five.spec(A.KIND_BY_NAME["quad2d"]).sigma)[:6] == [0.5, 0.0, 0.25, 0.125, 1.0, 0.0]
    back = SensorNoise.from_spec(five.spec(A.KIND_BY_NAME["quad2d"]), A.KIND_BY_NAME["quad2d"])
    assert back.sigma == five.sigma and repr(back) == repr(five)
    assert SensorNoise.from_spec(sn.spec(q3), q3).sigma == (0.25,) * 10
    for bad in (None, "0.1", True, [0.1, "x"], object()):
        with pytest.raises(TypeError):
            SensorNoise(bad)
    for bad in (-0.1, float("nan"), float("inf"), 1e39, (), (0.1,) * 17, (0.1, -0.2), (0.1, float("nan"))):
        with pytest.raises(ValueError):
            SensorNoise(bad)
    for bad in ("", "a", "0.1,b", "0.1;0.2"):
        with pytest.raises(ValueError):
            SensorNoise.parse(bad)
    with pytest.raises(TypeError):
        SensorNoise.parse(0.1)
    with pytest.raises(ValueError):
        five.spec(q3)                                  # 5 components, quadrotor3d observes 10
    with pytest.raises(ValueError):
        sn.spec(A.REINMAV)
    assert check_sensor_noise(None) is None and check_sensor_noise(sn, q3) is sn
    with pytest.raises(TypeError):
        check_sensor_noise(0.25)


def C_sizeof(A):
    import ctypes

    return ctypes.sizeof(A.SensorNoiseSpec)

"""Start-state ranges (rmav_set_start_state, include/rmav.h), restated in numpy for the tests: the host's derivation of h and m from (lo, hi)
and the map of a fresh state.

    h_c = (hi_c - lo_c) / 2, m_c = (hi_c + lo_c) / 2     in fp64 from the spec's fp32 values, each rounded to fp32 once
    s_c = fma(h_c, v_c, m_c)                             fp32, ONE rounding (actuator_ref.fma32: the exact fma)

v is the reference's draw, oracle.reset_states(kind, seed, env_ids, episodes): the "reset" stream of the RNG table, v_c = fma(2^-23, x >> 8, -1)."""
import numpy as np

from actuator_ref import bits, fma32, fma32_exact, from_bits  # noqa: F401  (the exact single-rounding fma; imported, not copied)
from util import NS

F32 = np.float32


def coeffs(lo, hi):
    """(h, m) in fp32 for arrays of lo and hi - what the host derives from the spec's fp32 values"""
    lo, hi = np.asarray(lo, F32).astype(np.float64), np.asarray(hi, F32).astype(np.float64)
    return ((hi - lo) * 0.5).astype(F32), ((hi + lo) * 0.5).astype(F32)


def map_state(lo, hi, v):
    """the fresh states of a handle with the ranges [lo, hi] from the reference's draws v [..., nS]"""
    h, m = coeffs(lo, hi)
    return fma32(h, np.asarray(v, F32), m)


def start_states(kind, seed, env_ids, episodes, lo, hi):
    """the fresh state of each env at its reset index: [len(env_ids), nS]"""
    import oracle as O

    return map_state(lo, hi, O.reset_states(kind, seed, env_ids, episodes))


def ranges(kind):
    """(lo, hi) of the tests: another range for every component, component 1 pinned (lo == hi), component 2 not straddling 0.  Every bound
    is a multiple of 1/64, so h and m are exact and a state never leaves [lo, hi] by the rounding of m (tests/test_start_state_host.py shows
    a range that does)."""
    nS = NS[kind]
    c = np.arange(nS)
    lo = (-(20.0 + c) / 64.0).astype(F32)
    hi = ((12.0 + 2.0 * c) / 64.0).astype(F32)
    lo[1] = hi[1] = F32(0.25)
    lo[2], hi[2] = F32(8.0 / 64.0), F32(26.0 / 64.0)
    return lo, hi


def identity(kind):
    nS = NS[kind]
    return np.full(nS, -1.0, F32), np.full(nS, 1.0, F32)

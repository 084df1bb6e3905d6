"""Actuator lag (rmav_set_actuator, include/rmav.h), restated in numpy for the tests: the filter statement with an EXACT fp32 fma, the host's
derivation of alpha / beta from (tau, dt), and the episode rule (m = init after a done).

    m_c = fma(alpha_c, u_c, beta_c * m_c)       the product beta_c * m_c rounded to fp32 on its own, then one fma: product and sum formed
                                                exactly, ONE rounding to fp32
    alpha_c = 1 - exp(-dt / tau_c), beta_c = exp(-dt / tau_c)   in fp64, each rounded to fp32 once; tau_c = 0: alpha = 1, beta = 0

fma32_exact is the statement itself, in rationals.  fma32 is its vectorised form: the product of two fp32 values is exact in fp64, the sum
with the addend is split into its fp64 rounding and the exact remainder (two-sum), the pair is folded into ONE fp64 value rounded to odd,
and the conversion of that to fp32 rounds once (fp64 carries more than 2 x 24 + 2 bits).  tests/test_actuator_host.py compares the two with
each other and with the kernels' own function compiled for the host."""
import math
from fractions import Fraction

import numpy as np

F32 = np.float32


def bits(x):
    return np.asarray(x, F32).view(np.uint32)


def from_bits(u):
    return np.asarray(u, np.uint32).view(F32)


def _round_fraction_to_f32(x: Fraction) -> np.float32:
    """a non-zero rational, rounded to the nearest fp32 (ties to even), denormals and overflow included"""
    sign = -1 if x < 0 else 1
    x = abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()   # 2^e <= x < 2^(e+1), up to one
    if Fraction(2) ** e > x:
        e -= 1
    if Fraction(2) ** (e + 1) <= x:
        e += 1
    e = max(e, -126)
    quantum = Fraction(2) ** (e - 23)
    q = x / quantum
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (n & 1)):
        n += 1
    val = n * quantum
    if val >= Fraction(2) ** 128:
        return F32(sign * np.inf)
    return F32(sign * float(val))   # (val has at most 24 significant bits: the conversions are exact)


def fma32_exact(a, b, c) -> np.float32:
    """fma(a, b, c) of three finite fp32 values: the exact product plus the exact addend, one rounding"""
    a, b, c = F32(a), F32(b), F32(c)
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if x == 0:
        # an exact zero: the common sign of product and addend when both are zeros of one sign, +0 otherwise (round to nearest)
        p_neg = bool(np.signbit(a)) != bool(np.signbit(b))
        if float(a) * float(b) == 0.0 and float(c) == 0.0 and p_neg and bool(np.signbit(c)):
            return F32(-0.0)
        return F32(0.0)
    return _round_fraction_to_f32(x)


def fma32(a, b, c):
    """fma32_exact, vectorised (finite fp32 arrays whose product does not underflow fp64)"""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b                                 # exact: 24 + 24 bits
        s = p + c                                 # fp64 rounding of the exact sum ...
        bb = s - p
        err = (p - (s - bb)) + (c - bb)           # ... and its exact remainder (two-sum)
    # round to odd: the truncation of the exact sum towards zero, with the last bit set when anything was dropped
    u = s.view(np.int64).copy()
    inexact = err != 0.0
    away = inexact & ((err > 0) != (s > 0))       # the remainder points towards zero: s was rounded away from it
    with np.errstate(over="ignore"):              # (the discarded arm of the first where: -0.0 is the smallest int64)
        u = np.where(away, u - 1, u)              # (the magnitude's bit pattern decreases towards zero for either sign)
        u = np.where(inexact, u | 1, u)
        return u.view(np.float64).astype(F32)


def coeffs(tau, dt):
    """(alpha, beta) in fp32 for one component: what the host derives from the spec's tau - an fp32 value - and rmav_params.dt"""
    tau = float(F32(tau))
    if not tau > 0.0:
        return F32(1.0), F32(0.0)
    e = math.exp(-float(dt) / tau)
    return F32(1.0 - e), F32(e)


def coeff_arrays(tau, dt, nA):
    """alpha[nA], beta[nA] for a scalar tau or one per component"""
    taus = [tau] * nA if np.isscalar(tau) else list(tau)
    ab = [coeffs(t, dt) for t in taus]
    return np.array([x[0] for x in ab], F32), np.array([x[1] for x in ab], F32)


def filt(alpha, beta, m, u):
    """one dynamics step of the filter; arrays broadcast"""
    bm = np.asarray(beta, F32) * np.asarray(m, F32)   # fp32 product, rounded on its own
    return fma32(alpha, u, bm)


def filt_exact(alpha, beta, m, u) -> np.float32:
    bm = F32(F32(beta) * F32(m))
    return fma32_exact(alpha, u, bm)


class Lag:
    """The per-env actuator state of a batch: m[N, nA], advanced once per dynamics step, init after a done (the episode rule)."""

    def __init__(self, tau, dt, init, n):
        init = np.asarray(init, F32)
        self.nA = init.shape[0]
        self.alpha, self.beta = coeff_arrays(tau, dt, self.nA)
        self.init = init
        self.m = np.tile(init, (n, 1))

    def step(self, u, live=None):
        """advance by one dynamics step with the commands u[N, nA] (only rows where live, default all); returns m"""
        new = filt(self.alpha[None, :], self.beta[None, :], self.m, np.asarray(u, F32))
        self.m = new if live is None else np.where(np.asarray(live, bool)[:, None], new, self.m)
        return self.m.copy()

    def end_of_step(self, done, auto_reset=True):
        """the episode rule: envs whose episode ended start the next one from init"""
        if auto_reset:
            self.m = np.where(np.asarray(done, bool)[:, None], self.init[None, :], self.m)

    def reset(self):
        self.m = np.tile(self.init, (self.m.shape[0], 1))

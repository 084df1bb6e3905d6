"""fp64 restatement of the SAMPLING half of the in-kernel policy (csrc/rmav_policy.hpp gaussian4, and the statements around its call
sites in rmav_rollout_body.inc / rmav_pair_draw.inc / rmav_pair_body.inc / rmav_pair_shared_body.inc / rmav_pair_env_load.inc), with a
per-output error bound.  Test-only, NumPy only.  oracle/policy_ref.py is the other half (means and values).

The arithmetic restated, for env `e` at global step `t` of a handle with seed `s`:

  r[0..3] = Philox4x32-10(counter (e_lo, e_hi, t_lo, 3 << 24 | ((t >> 32) & 0xFFFF) << 8), key (s_lo, s_hi))
  u1 = ((r[2p] >> 8) + 1) / 2^24 in (0, 1],  u2 = (r[2p + 1] >> 8) / 2^24 in [0, 1)          (both exact in fp32)
  rad = sqrtf(-2 logf(u1)),  (sn, cs) = sincospif(2 u2),  z[2p] = rad cs,  z[2p + 1] = rad sn          p = 0, 1
  std[c] = expf(logstd[c]) * noise_scale,  act[c] = fma(std[c], z[c], mean[c])                                c < nA
  q = fma(z[c], z[c], q) over c < nA (from 0),  q *= noise_scale,  sl = logstd[0] + .. + logstd[nA - 1] (fp32, in order)
  logp0 = -sl - fl32(0.5 nA fl32(ln 2 pi)),  logp = fma(-0.5, q, logp0)

Here every step is carried in fp64 from the exact rationals u1, u2 (sin / cos of exact multiples of a quarter turn are set to their
exact 0 / +-1), and the kernel's own roundings are bounded to first order (U = 2^-24; half an ulp is at most U relative, one ulp 2 U):

  ln      E_LOG ulps of logf: 2 E_LOG U relative on ln u1, half of that on rad
  sqrt    E_SQRT ulps of sqrtf: 2 E_SQRT U relative on rad
  angle   E_SINCOSPI ulps of sincospif, taken as ABSOLUTE error at the spacing of 1.0 (2 U per ulp), so nothing is assumed about its
          relative accuracy beside a zero: 2 E_SINCOSPI U on sn and cs, times rad on z
  product one rounding of rad * cs: U relative
          => bound_z = U (A |z_ref| + B rad_ref),  A = E_LOG + 2 E_SQRT + 1,  B = 2 E_SINCOSPI
  std     E_EXP ulps of expf: 2 E_EXP U relative (the multiplication by noise_scale = 0 or 1 is exact)
  act     std bound_z + 2 E_EXP U std |z_ref| + U |act_ref| (the one rounding of the fma)            [x SAFETY]  + mean_bound
  logp    sum_c |z_c| bound_z_c + nA U q / 2 (nA fma roundings, each at most U q, halved by the -0.5) + (nA - 1) U sum |logstd| (sl)
          + U |logp0| (the subtraction) + U |logp_ref| (the last fma)                                 [x SAFETY]
          + nA / 2 |fl32(ln 2 pi) - ln 2 pi| (a known constant of the kernel, not a rounding: unscaled)

Tests assert SAFETY = 4 times the first-order part; mean_bound (policy_ref's own worst case) is added as it is.

`mutant=` applies one deliberate error (MUTANTS) to the restatement; tests/test_sample_ref_host.py shows that each leaves the bound by
more than a decade on the inputs tests/test_gpu_policy_sample.py launches."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

# Maximum error, in ulps, of the device's accurate (-fno-fast-math, OCML) single-precision functions.
# Source: NONE FOUND.  The table these figures should come from is the "Math API" page of the HIP documentation ("maximum ULP
# difference" per function); no copy of it ships with the ROCm installation this file was written against (its share/doc tree holds
# the runtime API reference only, and no header states the figures).  As agreed for that case, each of the four is taken as 2 ulps.
# When a copy of the table is at hand, correct the figures HERE - nothing else in the bound is tunable.
ULP_TABLE = {
    "logf": 2.0,        # assumed (no table available)
    "sqrtf": 2.0,       # assumed
    "sincospif": 2.0,   # assumed
    "expf": 2.0,        # assumed
}
E_LOG, E_SQRT, E_SINCOSPI, E_EXP = (ULP_TABLE[k] for k in ("logf", "sqrtf", "sincospif", "expf"))
A_Z = E_LOG + 2.0 * E_SQRT + 1.0
B_Z = 2.0 * E_SINCOSPI
SAFETY = 4.0

U = 2.0 ** -24
LN_2PI = float(np.log(2.0 * np.pi))
LN_2PI_F32 = float(np.float32(1.8378770664093453))     # the kernels' literal, as fp32
NOISE_TAG = 3

MUTANTS = ("no_plus1", "shift9", "tag2", "drop_t_hi", "drop_env_hi", "swap_sincos", "swap_z12", "stale_t2", "std_xor1", "logstd_sum4",
           "q_sum4", "fast_log")

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _u64(x):
    """Python ints (up to 2^64 - 1) or arrays -> uint64 array, without a detour through int64 / float64."""
    if isinstance(x, np.ndarray):
        return x.astype(np.uint64)
    if isinstance(x, (int, np.integer)):
        return np.asarray(int(x) & (2 ** 64 - 1), dtype=np.uint64)
    return np.array([int(v) & (2 ** 64 - 1) for v in x], dtype=np.uint64)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32-10: uint64 arrays holding 32-bit words (broadcast against each other) -> uint64 [..., 4] of 32-bit words.
    The plain form: 64-bit products, high and low halves by shift and mask."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[_u64(v) & _M32 for v in (c0, c1, c2, c3, k0, k1)])
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2
        n0 = (p1 >> _S32) ^ c1 ^ k0
        n2 = (p0 >> _S32) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & _M32, p0 & _M32, n0, n2
        k0, k1 = (k0 + w0) & _M32, (k1 + w1) & _M32
    return np.stack([c0, c1, c2, c3], axis=-1)


def noise_words(seed, env_ids, t, tag=NOISE_TAG, mutant=None):
    """The four Philox words of the noise draw of (env, step): uint64 [..., 4]; env_ids and t broadcast."""
    e, t, s = _u64(env_ids), _u64(t), _u64(seed)
    e_hi = (e >> _S32) if mutant != "drop_env_hi" else np.zeros_like(e)
    t_hi = ((t >> _S32) & np.uint64(0xFFFF)) if mutant != "drop_t_hi" else np.zeros_like(t)
    c3 = (np.uint64(tag) << np.uint64(24)) | (t_hi << np.uint64(8))
    return philox4x32_10(e & _M32, e_hi, t & _M32, c3, s & _M32, s >> _S32)


def _quarter_exact(k):
    """(sin, cos)(2 pi k / 2^24) in fp64 for integer k in [0, 2^24), exact 0 / +-1 at the quarter turns.  The argument is reduced to
    [-1/8, 1/8] of a turn in exact integer arithmetic first, so the fp64 result is good to ~1e-16 absolute AND relative."""
    k = k.astype(np.int64)
    quad = (k + (1 << 21)) >> 22                      # nearest quarter turn, 0 .. 4
    rem = (k - (quad << 22)).astype(np.float64)       # in [-2^21, 2^21)
    a = rem * (2.0 * np.pi / 16777216.0)
    s, c = np.sin(a), np.cos(a)
    q = quad & 3
    sn = np.where(q == 0, s, np.where(q == 1, c, np.where(q == 2, -s, -c)))
    cs = np.where(q == 0, c, np.where(q == 1, -s, np.where(q == 2, -c, s)))
    return sn + 0.0, cs + 0.0


def noise(seed, env_ids, t, mutant=None):
    """(z_ref [..., 4], rad_ref [..., 2], bound_z [..., 4]) in fp64 for env ids and steps that broadcast against each other.
    bound_z is the FIRST-ORDER bound (the tests assert SAFETY times it)."""
    assert mutant is None or mutant in MUTANTS, mutant
    if mutant == "stale_t2":
        t = (_u64(t) - np.uint64(2))                   # (wraps below 2: any other step's draw is as wrong)
    r = noise_words(seed, env_ids, t, tag=2 if mutant == "tag2" else NOISE_TAG, mutant=mutant)
    shift = np.uint64(9 if mutant == "shift9" else 8)
    k1 = (r[..., 0::2] >> shift) + np.uint64(0 if mutant == "no_plus1" else 1)       # [..., 2]
    k2 = r[..., 1::2] >> np.uint64(8)
    u1 = k1.astype(np.float64) / 16777216.0
    with np.errstate(divide="ignore"):
        if mutant == "fast_log":   # v_log_f32-style: log2 good to 2^-22 absolute, times fl32(ln 2)
            l2 = np.rint(np.log2(u1) * 4194304.0) / 4194304.0
            ln = (l2.astype(np.float32) * np.float32(0.6931471805599453)).astype(np.float64)
        else:
            ln = np.where(k1 == np.uint64(16777216), 0.0, np.log(u1))
    rad = np.sqrt(-2.0 * ln) + 0.0
    sn, cs = _quarter_exact(k2)
    if mutant == "swap_sincos":
        sn, cs = cs, sn
    z = np.stack([rad[..., 0] * cs[..., 0], rad[..., 0] * sn[..., 0], rad[..., 1] * cs[..., 1], rad[..., 1] * sn[..., 1]], axis=-1)
    if mutant == "swap_z12":
        z = z[..., [0, 2, 1, 3]]
    rad4 = np.repeat(rad, 2, axis=-1)
    with np.errstate(invalid="ignore"):
        bound = U * (A_Z * np.abs(z) + B_Z * rad4)
    return z, rad, bound


@dataclass
class Sample:
    """act, bound_act [..., nA]; logp, bound_logp [...]; logp0: the launch's constant; std [nA].  The bounds are the ASSERTED ones
    (SAFETY times the first-order part, plus mean_bound)."""
    act: np.ndarray
    bound_act: np.ndarray
    logp: np.ndarray
    bound_logp: np.ndarray
    logp0: float
    bound_logp0: float
    std: np.ndarray


def sample(mean, mean_bound, logstd, noise_scale, z_ref, bound_z, nA, mutant=None, logstd_pad=(0.0, 0.0, 0.0, 0.0)):
    """The stored action and its log-probability.  mean, mean_bound: [nA] or [..., nA] (policy_ref's numbers); logstd: the policy's
    [nA] (rounded to fp32 here, as the packer stores it); z_ref, bound_z [..., 4] from noise(); noise_scale 1 (sample) or 0 (deterministic).
    logstd_pad: what the staged log-std buffer holds in slots nA .. 3 (the packer stores zeros) - only the `logstd_sum4` mutant reads it."""
    assert mutant is None or mutant in MUTANTS, mutant
    ls = np.asarray(logstd, np.float32).astype(np.float64)
    assert ls.shape == (nA,) and nA in (2, 4)
    ns = float(noise_scale)
    std = np.exp(ls) * ns
    mean = np.asarray(mean, np.float64)
    mean_bound = np.asarray(mean_bound, np.float64)
    z, bz = z_ref[..., :nA], bound_z[..., :nA]
    std_used = std[np.arange(nA) ^ 1] if mutant == "std_xor1" else std
    act = std_used * z + mean
    with np.errstate(invalid="ignore"):
        first = std * bz + 2.0 * E_EXP * U * std * np.abs(z) + U * np.abs(std * z + mean)
    bound_act = SAFETY * first + mean_bound
    zq = z_ref if mutant == "q_sum4" else z
    q = (zq * zq).sum(-1)
    staged = np.concatenate([ls, np.asarray(logstd_pad, np.float64)[nA:4]])
    sl = float(staged.sum()) if mutant == "logstd_sum4" else float(ls.sum())
    logp0 = -sl - 0.5 * nA * LN_2PI
    logp = -0.5 * ns * q + logp0
    const = 0.5 * nA * abs(LN_2PI_F32 - LN_2PI)
    first0 = (nA - 1) * U * float(np.abs(ls).sum()) + U * abs(logp0)
    q_true = (z * z).sum(-1)
    with np.errstate(invalid="ignore"):
        first_l = ns * ((np.abs(z) * bz).sum(-1) + 0.5 * nA * U * q_true) + first0 + U * np.abs(-0.5 * ns * q_true + (-float(ls.sum()) - 0.5 * nA * LN_2PI))
    return Sample(act, bound_act, logp, SAFETY * first_l + const, logp0, SAFETY * (first0 + U * abs(logp0)) + const, std)

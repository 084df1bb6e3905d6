"""fp64 restatement of the sensor-noise draw (csrc/rmav_sensor.hpp; include/rmav.h, stream "sensor"), with a per-output error bound.
Test-only, NumPy only.  Built on oracle/sample_ref.py - the restatement of the policy's Box-Muller draw, whose lines the sensor draw
repeats with tag 7 and the block index j in the low byte of the last counter word:

  r[0..3] = Philox4x32-10(counter (e_lo, e_hi, b_lo, 7 << 24 | ((b >> 32) & 0xFFFF) << 8 | j), key (s_lo, s_hi)),  j = c >> 2
  u1 = ((r[2p] >> 8) + 1) / 2^24,  u2 = (r[2p + 1] >> 8) / 2^24,  rad = sqrtf(-2 logf(u1)),  (sn, cs) = sincospif(2 u2)
  z[4j + 2p] = rad cs,  z[4j + 2p + 1] = rad sn                                                            p = 0, 1
  o_c = fma(sigma_c, z_c, s_c)

b is the handle's step counter after the operation that produced the observation.  The asserted bound on o is

  SAFETY (sigma bound_z + U |o_ref|),     bound_z = U (A_Z |z_ref| + B_Z rad_ref)

sample_ref's `act` bound with a given sigma in std's place: no expf term and no mean_bound (s is an fp32 input, exact in fp64).  It
inherits sample_ref.ULP_TABLE's ASSUMED 2-ulp figures for logf, sqrtf and sincospif - no table of the device functions' accuracy was at
hand when that file was written; tests/test_gpu_policy_sample.py rests on the same figures for the same three functions.

`mutant=` applies one deliberate error (MUTANTS); tests/test_sensor_noise_host.py shows that each leaves the bound by more than a
decade on the inputs the GPU test uses."""
import numpy as np

import sample_ref as S

SENSOR_TAG = 7
MUTANTS = ("tag3", "drop_j", "b_minus_1", "drop_t_hi", "swap_sincos", "wrong_block")
MOMENT_SEED = 11          # the seed of the moment tests (host: the restatement alone; GPU: the device against the same caps)
MOMENT_N = 4096
MEAN_CAP = 5.0 / 64.0                     # five standard errors of the mean of 4096 standard normals
STD_CAP = 5.0 / np.sqrt(8192.0)           # ... and of their standard deviation

_M32, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def words(seed, env_ids, b, j, mutant=None):
    """The four Philox words of block (b, j): uint64 [..., 4]; env_ids, b and j broadcast."""
    e, b, s, j = S._u64(env_ids), S._u64(b), S._u64(seed), S._u64(j)
    if mutant == "b_minus_1":
        b = b - np.uint64(1)
    b_hi = ((b >> _S32) & np.uint64(0xFFFF)) if mutant != "drop_t_hi" else np.zeros_like(b)
    tag = np.uint64(3 if mutant == "tag3" else SENSOR_TAG)
    c3 = (tag << np.uint64(24)) | (b_hi << np.uint64(8)) | (np.zeros_like(j) if mutant == "drop_j" else j)
    return S.philox4x32_10(e & _M32, e >> _S32, b & _M32, c3, s & _M32, s >> _S32)


def uniform_bits(r):
    """The fp32 bits of (u1, u2) of both pairs of a block: uint32 [..., 4] = (u1_0, u2_0, u1_1, u2_1), both exact in fp32."""
    k = (r >> np.uint64(8)).astype(np.float64)
    k[..., 0::2] += 1.0
    return (k / 16777216.0).astype(np.float32).view(np.uint32)


def z4(seed, env_ids, b, j, mutant=None):
    """(z_ref, bound_z) [..., 4] in fp64 of block (b, j); bound_z is the first-order bound."""
    r = words(seed, env_ids, b, j, mutant)
    k1 = (r[..., 0::2] >> np.uint64(8)) + np.uint64(1)
    k2 = r[..., 1::2] >> np.uint64(8)
    u1 = k1.astype(np.float64) / 16777216.0
    ln = np.where(k1 == np.uint64(16777216), 0.0, np.log(u1))
    rad = np.sqrt(-2.0 * ln) + 0.0
    sn, cs = S._quarter_exact(k2)
    if mutant == "swap_sincos":
        sn, cs = cs, sn
    z = np.stack([rad[..., 0] * cs[..., 0], rad[..., 0] * sn[..., 0], rad[..., 1] * cs[..., 1], rad[..., 1] * sn[..., 1]], axis=-1)
    rad4 = np.repeat(rad, 2, axis=-1)
    return z, S.U * (S.A_Z * np.abs(z) + S.B_Z * rad4)


def z_ref(seed, env_ids, b, nS, mutant=None):
    """(z_ref, bound_z) [n, nS] of the envs `env_ids` (a 1-D array) at the step counter b."""
    env_ids = S._u64(np.asarray(env_ids))
    nb = (nS + 3) // 4
    zs, bs = zip(*(z4(seed, env_ids, b, j, mutant) for j in range(nb)))
    if mutant == "wrong_block":   # sigma applied to z of the next block (cyclically)
        zs, bs = zs[1:] + zs[:1], bs[1:] + bs[:1]
    return np.concatenate(zs, axis=-1)[:, :nS], np.concatenate(bs, axis=-1)[:, :nS]


def o_ref(sigma, seed, env_ids, b, s, mutant=None):
    """(o_ref, bound) [n, nS]: the observation of the states s [n, nS] (fp32) and the ASSERTED bound.  sigma: [nS]."""
    s = np.asarray(s)
    assert s.dtype == np.float32 and s.ndim == 2
    sigma = np.asarray(sigma, np.float32).astype(np.float64)
    z, bz = z_ref(seed, env_ids, b, s.shape[1], mutant)
    o = sigma * z + s.astype(np.float64)
    return o, S.SAFETY * (sigma * bz + S.U * np.abs(o))

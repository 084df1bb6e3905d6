"""Termination rules (rmav_set_termination, include/rmav.h), restated in numpy for the tests: the rule on a stored post-step fp32 state s.

    nonfinite = any c < nS: !(|s_c| < inf)
    outside   = any body B, any axis i < dim: !(B_i >= pos_lo_i) || !(B_i <= pos_hi_i)      bodies: s[0:dim] and - slung load - s[5:7] / s[10:13]
    tilted    = 2-D: |s[2]| > max_tilt
                3-D: fma(w,w, fma(z,z, -fma(x,x, y*y))) < c * fma(w,w, fma(x,x, fma(y,y, z*z))),  (w,x,y,z) = s[3:7],
                     c = (float)cos((double)max_tilt), -inf for max_tilt = +inf
    rule      = nonfinite || outside || tilted

fp32 throughout; every fma is the exact single-rounding one of tests/start_ref.py (actuator_ref.fma32), every plain product one fp32 rounding."""
import numpy as np

from start_ref import bits, fma32, from_bits  # noqa: F401  (the exact fma; imported, not copied)
from util import NS

F32 = np.float32
INF = F32(np.inf)
DIM = {"quad2d": 2, "quad2d_sl": 2, "quad3d": 3, "quad3d_sl": 3}
LOAD = {"quad2d": None, "quad2d_sl": 5, "quad3d": None, "quad3d_sl": 10}


def fma(a, b, c):
    """fma32 where all three are finite; with an inf or a NaN among them IEEE fixes the result whatever the precision"""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    ok = np.isfinite(a) & np.isfinite(b) & np.isfinite(c)
    z = F32(0.0)
    exact = fma32(np.where(ok, a, z), np.where(ok, b, z), np.where(ok, c, z))
    with np.errstate(all="ignore"):
        special = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
    return np.where(ok, exact, special)


def cos_tilt(max_tilt):
    """the seventh threshold of a 3-D kind, as the host derives it: fp64 cosine of the fp32 value, rounded once"""
    mt = F32(max_tilt)
    return F32(-np.inf) if not mt < INF else F32(np.cos(np.float64(mt)))


def spec3(kind, pos_lo=None, pos_hi=None):
    """(pos_lo, pos_hi) as fp32 arrays of 3: None = unbounded, a scalar broadcasts, the third axis of a 2-D kind is unbounded"""
    d = DIM[kind]
    lo, hi = np.full(3, -np.inf, F32), np.full(3, np.inf, F32)
    if pos_lo is not None:
        lo[:d] = np.asarray(pos_lo, F32)
    if pos_hi is not None:
        hi[:d] = np.asarray(pos_hi, F32)
    return lo, hi


def parts(kind, s, pos_lo=None, pos_hi=None, max_tilt=None):
    """(nonfinite, outside, tilted) for states s [n, nS]: three bool arrays of n"""
    s = np.asarray(s, F32).reshape(-1, NS[kind])
    d = DIM[kind]
    lo, hi = spec3(kind, pos_lo, pos_hi)
    mt = INF if max_tilt is None else F32(max_tilt)
    with np.errstate(invalid="ignore", over="ignore"):
        nonfinite = (~(np.abs(s) < INF)).any(1)
        bodies = [s[:, 0:d]] + ([s[:, LOAD[kind]:LOAD[kind] + d]] if LOAD[kind] is not None else [])
        outside = np.zeros(len(s), bool)
        for b in bodies:
            outside |= (~(b >= lo[:d]) | ~(b <= hi[:d])).any(1)
        if d == 2:
            tilted = np.abs(s[:, 2]) > mt
        else:
            w, x, y, z = (s[:, 3 + i] for i in range(4))
            up = fma(w, w, fma(z, z, -fma(x, x, (y * y).astype(F32))))
            n2 = fma(w, w, fma(x, x, fma(y, y, (z * z).astype(F32))))
            tilted = up < (cos_tilt(mt) * n2).astype(F32)
    return nonfinite, outside, tilted


def rule(kind, s, pos_lo=None, pos_hi=None, max_tilt=None):
    nf, out, tilt = parts(kind, s, pos_lo, pos_hi, max_tilt)
    return nf | out | tilt


# ---- the spec and the commands of the GPU tests -----------------------------------------------------------------------------------------
# A fresh state is U[-1, 1) per component.  The box keeps about nine fresh states in ten; the tilt limit keeps every second one (2-D: |theta| <=
# 0.5 of U[-1, 1); 3-D: the body's z axis above the horizon, which half of the random quaternions are).  The commands turn every env at a
# strong rate of constant sign, so an attitude that starts inside the cone leaves it within a few steps, and keep the thrust moderate, so the
# reference's own rule (|pos|, |vel|) fires rarely but does fire.  Counted with the fp64 oracle before the values were settled (130 envs, 12
# steps, per kind): every env has 1 to 10 rule-only terminations and at least one step that does not end; tests/test_gpu_termination.py
# asserts the counts from the twin's own data.
def spec(kind):
    """(pos_lo, pos_hi, max_tilt) of the GPU tests"""
    d = DIM[kind]
    return (-0.97,) * d, (0.97,) * d, (0.5 if d == 2 else 1.6)


def commands(kind, n, T=12):
    """[T, n, nA] fp32 buffered commands: thrust near hover (quad2d: half of it), a turning rate of one sign per env"""
    from util import NA

    rng = np.random.RandomState(177 + n)
    nA = NA[kind]
    u = np.zeros((T, n, nA), F32)
    u[..., 0] = ((5.0 if kind == "quad2d" else 9.8) * rng.uniform(0.9, 1.1, (T, n))).astype(F32)
    sign = np.where(rng.uniform(size=(1, n, nA - 1)) < 0.5, -1.0, 1.0)
    lo, hi = (25.0, 40.0) if nA == 2 else (30.0, 50.0)
    u[..., 1:] = (sign * rng.uniform(lo, hi, (T, n, nA - 1))).astype(F32)
    if nA == 4:
        u[..., 3] *= F32(0.1)
    return u

"""Quantisation-exact fp64 restatement of the in-kernel policy actors, with a per-output error bound.  Test-only, NumPy only.

Each function restates one actor family of csrc/rmav_policy*.hpp in fp64 on EXACTLY the operands the kernel feeds its multiply-adds:
every value is quantised where the kernel quantises it (and nowhere else), and is carried in fp64, which holds every fp32 / bf16 /
f16 value and every product of two of them exactly.  What is left between a kernel and this file is

  * the fp32 accumulation error of the kernel's dot products, and
  * an activation that lands on the other side of a rounding boundary of the operand format (`undecided`),

and both are bounded here, per env and output row, from the reference's own numbers.  The constants of the bound are worst-case
derivations from the documented accuracy of the instructions, not measurements.

The arithmetic restated (k = 2 log2 e as the kernels' fp32 constant kTanhScale):

  bf16 (rmav_policy_mfma.hpp; the pair kernel of rmav_policy_pair.hpp computes the same per net)
      x' = bf16_rne(fl32(k x));  A = bf16_rne(W);  accumulators start from fl32(k b1), fl32(k b2), b3
      r = 1 / (1 + 2^acc);  layer-2 operand bf16_rne(fma(r, -2k, k));  layer-3 operand bf16_rne(fma(r, -2, 1))
  f16 / f16_shared (rmav_policy_pair.hpp)
      x' = f16_rtz(fl32(k x)), finite overflow saturating at 65504;  A1 = f16_rne(W1), A2' = f16_rne(fl32(-2k W2)),
      A3' = f16_rne(fl32(-2 W3));  biases fl32(k b1),  k b2 - sum_j A2'[i][j] / 2,  b3 - sum_j A3'[i][j] / 2 (fold_biases_f16, fp32);
      the operand handed on is f16_rne(r) itself.  f16_shared: ONE trunk, output rows 0..nA-1 the mean head, row 4 the value head.
  fp32 / fp32_mfma (rmav_policy.hpp, rmav_policy_mfma32.hpp): no quantisation; tanh(z) = fma(rcp(1 + exp2(fl32(k z))), -2, 1).

The bound (U = 2^-24):

  accumulation   e_z = C U (sum_j |a_ij| |x_j| + |b_i|),  C = 2 (K + 2) for the padded depth K (16 or 64): ONE ulp (not half) per
                 multiply-add and bias add, because the rounding inside the MFMA accumulator is not documented.  f16: plus
                 65 U sum_j |a_ij| / 2 for the fp32 row sum of the in-kernel bias fold and U |k b2| for the fold's fp32 product.
  activation     before it is rounded: delta = |A| (dr + 3 U r) + U |v|, where dr is the change of r over [z - e_z, z + e_z]
                 (to first order r (1 - r) ln2 e_z; the interval form stays valid where e_z is not small, e.g. behind a 1e30 state),
                 v_exp_f32 / v_rcp_f32 are 1 ulp each and the fma rounds once.
  boundaries     an unrounded activation farther than delta from every rounding boundary of the operand format gives the kernel
                 the reference's operand exactly: the error restarts at 0.  Otherwise it is `undecided` and the next layer's
                 bound gains |a_ij| * (one spacing of the format there).
  f16 subnormal  whether the matrix core flushes f16-subnormal operands is not documented: a product with such an operand
                 contributes |a| |q| (the reference itself does not flush).
  fp32 actors    the same propagation without rounding steps: the activation error delta is carried into the next layer.

`mutant=` applies one deliberate arithmetic error to the restatement (tests/test_policy_ref_host.py proves with them that the
bound is tight enough to see each of them on the inputs the GPU test uses)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

U = 2.0 ** -24
LN2 = float(np.log(2.0))
K32 = np.float32(2.8853900817779268)       # kTanhScale (csrc/rmav_policy_mfma.hpp), the fp32 the kernels multiply by
K = float(K32)
F16_MIN_NORMAL = 2.0 ** -14

# (significand bits incl. the implicit one, frexp exponent of the smallest normal, largest finite value)
BF16 = (8, -125, float((2.0 - 2.0 ** -7) * 2.0 ** 127))
F16 = (11, -13, 65504.0)

MUTANTS = ("act_trunc", "input_rne", "zero_slot", "swap_lanes", "fold_unrounded", "sat_inf")


def rowmap(s: int, h: int, j: int) -> int:
    """Hidden unit that B-slot (h, j) of K-slice s carries (csrc/rmav_policy_mfma.hpp; restated, not imported, from ppo._rowmap)."""
    r = 8 * (s & 1) + j
    return 32 * (s >> 1) + (r & 3) + 8 * (r >> 2) + 4 * h


def _spacing(ax, fmt):
    p, emin, _ = fmt
    with np.errstate(invalid="ignore"):
        _, e = np.frexp(np.where(np.isfinite(ax), ax, 1.0))
    e = np.where(ax == 0, emin, np.maximum(e, emin))
    return np.ldexp(1.0, e - p), e


def quantise(x, fmt, mode="rne", saturate=False):
    """x (fp64) rounded to the format: round to nearest even, or toward zero.  Overflow: rne -> inf; rtz -> the largest finite value
    (what IEEE round-toward-zero does, and what `saturate` = the kernel's v_cvt_pkrtz_f16_f32 claim is); rtz with saturate=False
    turns a finite overflow into inf (the `sat_inf` mutant)."""
    x = np.asarray(x, np.float64)
    s, _ = _spacing(np.abs(x), fmt)
    with np.errstate(invalid="ignore", over="ignore"):
        t = x / s
        q = (np.rint(t) if mode == "rne" else np.trunc(t)) * s
    big = np.abs(q) > fmt[2]
    if mode == "rne" or not saturate:
        q = np.where(big, np.copysign(np.inf, x), q)
    else:
        q = np.where(big & np.isfinite(x), np.copysign(fmt[2], x), q)
    return q


def _round_activation(v, delta, fmt, trunc=False):
    """(operand, operand error bound, undecided) of an unrounded activation v known to within delta."""
    av = np.abs(v)
    s, e = _spacing(av, fmt)
    q = quantise(v, fmt, "rtz" if trunc else "rne", saturate=True)
    t = av / s
    dist = np.abs(t - np.floor(t) - 0.5) * s
    # below the bottom of a normal binade the grid is twice as fine: its first boundary lies s / 4 under the bottom
    bottom = np.ldexp(0.5, e)
    dist = np.where(e > fmt[1], np.minimum(dist, av - bottom + 0.25 * s), dist)
    with np.errstate(invalid="ignore"):
        und = ~(dist > delta)
        err = np.where(und, np.floor(np.where(np.isfinite(delta), delta, np.inf) / s + 1.0) * s, 0.0)
    return q, err, und


def _logistic(z):
    with np.errstate(over="ignore", invalid="ignore"):
        return 1.0 / (1.0 + np.exp2(z))


def _dr(z, e, r):
    """Bound of |r(z') - r(z)| over |z' - z| <= e: the interval (r is monotone), and never less than the first-order term."""
    with np.errstate(over="ignore", invalid="ignore"):
        inter = np.maximum(r - _logistic(z + e), _logistic(z - e) - r)
        rr = r * (1.0 - r)
        lin = np.where(rr > 0, rr * LN2 * np.minimum(e, 1e300), 0.0)
    return np.maximum(inter, np.minimum(lin, 1.0))


def _dot(A, x, ex, b, eb, depth, f16=False, und=None):
    """z = A x + b on exact operands; e = accumulation + operand-error (+ fold, + f16-subnormal) bound; S = sum |a||x| + |b|;
    number of f16-subnormal activation operands per column."""
    absA, absx = np.abs(A), np.abs(x)
    with np.errstate(invalid="ignore", over="ignore"):
        z = A @ x + b[:, None]
        S = absA @ (absx + ex) + np.abs(b)[:, None]
        e = 2.0 * (depth + 2) * U * S + absA @ ex + eb[:, None]
    nsub = np.zeros(x.shape[1], np.int64)
    if f16:
        sub_a = (A != 0) & (absA < F16_MIN_NORMAL)
        sub_x = (x != 0) & (absx < F16_MIN_NORMAL)
        if und is not None:   # the kernel's operand may be the subnormal neighbour of a normal one
            sub_x |= und & (absx > 0) & (absx <= F16_MIN_NORMAL + ex)
        with np.errstate(invalid="ignore", over="ignore"):
            e = e + (absA * sub_a) @ absx + (absA * ~sub_a) @ (absx * sub_x)
        nsub = sub_x.sum(0) + int(sub_a.sum())
    return z, e, S, nsub


def _pad_cols(W, cols):
    out = np.zeros((W.shape[0], cols), np.float64)
    out[:, :W.shape[1]] = W
    return out


def _f32(a):
    return np.asarray(a, np.float32)


def normalise(obs, norm):
    """med3((x - mean_f) * rstd_f, -clip, clip) in fp32: subtract, multiply, clamp (csrc/rmav_kernels.hpp norm1)."""
    obs = _f32(obs)
    if norm is None:
        return obs
    mean_f, rstd_f, clip = norm
    nS = obs.shape[0]
    z = (obs - _f32(mean_f)[:nS, None]) * _f32(rstd_f)[:nS, None]
    c = np.float32(clip)
    return np.minimum(np.maximum(z, -c), c).astype(np.float32)


def _input16(obs, norm):
    """The padded layer-1 input [16, N] in fp32."""
    x = normalise(obs, norm)
    out = np.zeros((16, x.shape[1]), np.float32)
    out[:x.shape[0]] = x
    return out


@dataclass
class Result:
    """Every array [N, nA + 1]; columns 0..nA-1 the mean rows, the last one the value.
    undecided: activations of the net behind that output that may round either way (undecided_l1: those of the FIRST hidden layer,
    the operands of layer 2); subnormal: f16-subnormal operands of that net (subnormal_l12: those of layers 1 and 2);
    scale: sum_j |a_ij||x_j| + |b_i| of the output layer (the unit the accumulation constant C multiplies, times 2^-24)."""
    y: np.ndarray
    bound: np.ndarray
    undecided: np.ndarray
    subnormal: np.ndarray
    scale: np.ndarray
    undecided_l1: np.ndarray
    subnormal_l12: np.ndarray

    @property
    def mean(self):
        return self.y[:, :-1]

    @property
    def value(self):
        return self.y[:, -1]


def _swap(q, mutant, layer):
    """`zero_slot` = (layer, unit): that hidden unit's B slot reads 0 in every column; `swap_lanes` = layer: env 48 + i of every
    64-env wavefront reads env 16 + i's hidden fragment."""
    if mutant is None:
        return q
    name, arg = mutant if isinstance(mutant, tuple) else (mutant, None)
    if name == "zero_slot" and arg[0] == layer:
        q = q.copy()
        q[arg[1]] = 0.0
    if name == "swap_lanes" and arg == layer:
        q = q.copy()
        e = np.arange(q.shape[1])
        dst = e[(e % 64) >= 48]
        q[:, dst] = q[:, dst - 32]
    return q


def _name(mutant):
    return mutant[0] if isinstance(mutant, tuple) else mutant


def _quantised_net(fmt, W1, b1, W2, b2, W3, b3, x16, mutant=None):
    """One 2 x 64 net on the matrix cores; fmt = BF16 or F16 (with the tanh fold).  W3 / b3: the output rows wanted.  Returns
    (y [R, N], bound, undecided [N], subnormal [N], scale [R, N])."""
    f16 = fmt is F16
    m = _name(mutant)
    kx = (K32 * x16).astype(np.float32).astype(np.float64)            # ONE fp32 rounding
    if f16:
        xq = quantise(kx, F16, "rne" if m == "input_rne" else "rtz", saturate=(m != "sat_inf"))
    else:
        xq = quantise(kx, BF16)
    W1, W2, W3 = (_f32(w) for w in (W1, W2, W3))
    b1, b2, b3 = (_f32(b) for b in (b1, b2, b3))
    kb1 = (K32 * b1).astype(np.float64)
    A1 = quantise(_pad_cols(W1.astype(np.float64), 16), fmt)
    zero = np.zeros(64)
    if f16:
        s2, s3 = np.float32(-2.0 * 2.8853900817779268), np.float32(-2.0)
        W2s, W3s = (W2 * s2).astype(np.float64), (W3 * s3).astype(np.float64)      # scaled in fp32, then rounded once
        A2, A3 = quantise(W2s, F16), quantise(W3s, F16)
        src2, src3 = (W2s, W3s) if m == "fold_unrounded" else (A2, A3)
        kb2 = K * b2.astype(np.float64)                                            # exact in fp64; the kernel rounds it once
        bb2 = kb2 - 0.5 * src2.sum(1)
        bb3 = b3.astype(np.float64) - 0.5 * src3.sum(1)
        eb2 = 65.0 * U * np.abs(A2).sum(1) / 2 + U * np.abs(kb2)
        eb3 = 65.0 * U * np.abs(A3).sum(1) / 2
        act_a = (1.0, 1.0)
    else:
        A2, A3 = quantise(W2.astype(np.float64), BF16), quantise(W3.astype(np.float64), BF16)
        bb2, bb3 = (K32 * b2).astype(np.float64), b3.astype(np.float64)
        eb2, eb3 = zero, np.zeros(len(b3))
        act_a = (2.0 * K, 2.0)
    ex0 = np.zeros_like(xq)
    z, e, _, nsub = _dot(A1, xq, ex0, kb1, zero, 16, f16)
    n_und = np.zeros(xq.shape[1], np.int64)
    for layer, (A, b, eb, a) in enumerate(((A2, bb2, eb2, act_a[0]), (A3, bb3, eb3, act_a[1])), start=1):
        r = _logistic(z)
        if f16:
            v = r
            delta = _dr(z, e, r) + 3.0 * U * r
        else:
            c = K if layer == 1 else 1.0
            v = c - 2.0 * c * r                                                    # fma(r, -2k, k) / fma(r, -2, 1)
            delta = a * (_dr(z, e, r) + 3.0 * U * r) + U * np.abs(v)
        q, ex, und = _round_activation(v, delta, fmt, trunc=(m == "act_trunc"))
        q = _swap(q, mutant, layer)
        n_und += und.sum(0)
        z, e, S, ns = _dot(A, q, ex, b, eb, 64, f16, und)
        nsub = nsub + ns
        if layer == 1:
            und1, nsub12 = n_und.copy(), nsub.copy()
    return z, e, n_und, nsub, S, und1, nsub12


def _stack(parts):
    """[(y [R, N], bound, und [N], sub [N], S [R, N], und of layer 1 [N], sub of layers 1-2 [N]), ...] -> Result with [N, sum R] arrays."""
    y = np.concatenate([p[0] for p in parts]).T
    b = np.concatenate([p[1] for p in parts]).T
    und = np.concatenate([np.repeat(p[2][None], p[0].shape[0], 0) for p in parts]).T
    sub = np.concatenate([np.repeat(p[3][None], p[0].shape[0], 0) for p in parts]).T
    S = np.concatenate([p[4] for p in parts]).T
    und1, sub12 = (np.concatenate([np.repeat(p[k][None], p[0].shape[0], 0) for p in parts]).T for k in (5, 6))
    return Result(y, b, und, sub, S, und1, sub12)


def _two_nets(fmt, nets, obs, norm, mutant):
    x16 = _input16(obs, norm)
    return _stack([_quantised_net(fmt, *nets["pi"], x16, mutant), _quantised_net(fmt, *nets["vf"], x16, mutant)])


def bf16(nets, obs, norm=None, mutant=None) -> Result:
    """nets = {"pi": [W1, b1, W2, b2, W3, b3], "vf": [...]} (fp32 arrays), obs [nS, N] fp32: the bf16 actors (pair and one-wavefront)."""
    return _two_nets(BF16, nets, obs, norm, mutant)


def f16(nets, obs, norm=None, mutant=None) -> Result:
    return _two_nets(F16, nets, obs, norm, mutant)


def f16_shared(nets, obs, norm=None, mutant=None) -> Result:
    """nets = {"pi": [W1, b1, W2, b2, W3, b3], "vf": [Wv [1, 64], bv [1]]}: one trunk, the mean head and the value head."""
    W1, b1, W2, b2, W3, b3 = nets["pi"]
    Wv, bv = nets["vf"]
    W3 = np.concatenate([_f32(W3), _f32(Wv).reshape(1, -1)])
    b3 = np.concatenate([_f32(b3), _f32(bv).reshape(1)])
    return _stack([_quantised_net(F16, W1, b1, W2, b2, W3, b3, _input16(obs, norm), mutant)])


def _tanh_fast(z, e):
    """tanh_fast (rmav_policy.hpp) of a pre-activation known to within e: a = fl32(k z) [k's own rounding and the product: 2 U |a|],
    t = v_exp_f32(a) [1 ulp = 2 U], 1 + t [U], v_rcp_f32 [2 U]: r to within dr(e_a) + 5 U r (6 U: second order); fma(r, -2, 1) [U |v|]."""
    a = K * z
    ea = K * e + 2.0 * U * np.abs(a)
    r = _logistic(a)
    v = 1.0 - 2.0 * r
    return v, 2.0 * (_dr(a, ea, r) + 6.0 * U * r) + U * np.abs(v)


def _fp32_net(W1, b1, W2, b2, W3, b3, x16):
    W1 = _pad_cols(_f32(W1).astype(np.float64), 16)
    W2, W3 = _f32(W2).astype(np.float64), _f32(W3).astype(np.float64)
    b1, b2, b3 = (_f32(b).astype(np.float64) for b in (b1, b2, b3))
    x = x16.astype(np.float64)
    z, e, S, _ = _dot(W1, x, np.zeros_like(x), b1, np.zeros(64), 16)
    for A, b in ((W2, b2), (W3, b3)):
        h, eh = _tanh_fast(z, e)
        z, e, S, _ = _dot(A, h, eh, b, np.zeros(len(b)), 64)
    n = np.zeros(x.shape[1], np.int64)
    return z, e, n, n, S, n, n


def fp32(nets, obs, norm=None, mutant=None) -> Result:
    """The two fp32 actors (vector ALU, and v_mfma_f32_32x32x2_f32): same operands, only the summation order differs, and the bound
    holds for any order."""
    assert mutant is None
    x16 = _input16(obs, norm)
    return _stack([_fp32_net(*nets["pi"], x16), _fp32_net(*nets["vf"], x16)])


fp32_mfma = fp32

ACTORS = {"fp32": fp32, "fp32_mfma": fp32_mfma, "bf16": bf16, "bf16_1w": bf16, "f16": f16, "f16_shared": f16_shared}


def packed_operands(actor, nets):
    """The quantised weight matrices the reference multiplies by and the UNSCALED fp32 biases, as the packer stores them:
    {"pi": (A1 [64, 16], A2, A3 [rows, 64], b1, b2, b3), "vf": ...} (f16_shared: one entry "pi" with the stacked output rows)."""
    fmt = BF16 if actor.startswith("bf16") else F16
    out = {}
    items = dict(nets)
    if actor == "f16_shared":
        W1, b1, W2, b2, W3, b3 = nets["pi"]
        Wv, bv = nets["vf"]
        items = {"pi": [W1, b1, W2, b2, np.concatenate([_f32(W3), _f32(Wv).reshape(1, -1)]), np.concatenate([_f32(b3), _f32(bv).reshape(1)])]}
    for name, (W1, b1, W2, b2, W3, b3) in items.items():
        W1, W2, W3 = (_f32(w) for w in (W1, W2, W3))
        if fmt is F16:
            W2, W3 = W2 * np.float32(-2.0 * 2.8853900817779268), W3 * np.float32(-2.0)
        out[name] = (quantise(_pad_cols(W1.astype(np.float64), 16), fmt), quantise(W2.astype(np.float64), fmt),
                     quantise(W3.astype(np.float64), fmt), _f32(b1), _f32(b2), _f32(b3))
    return out

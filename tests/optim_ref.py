"""fp64 restatement of the two launches around the fused learner (csrc/rmav_optim.hpp; the expressions are include/rmav_ppo.h's), each
with a per-output first-order error bound, in the manner of oracle/sample_ref.py.  Test-only, NumPy only.  It also makes the inputs
tests/test_gpu_optim.py launches (adv_input, adam_case), so that tests/test_optim_host.py can show on the CPU that a wrong
expression (MUTANTS) leaves the bound on exactly those inputs.

U = 2^-24 (half an ulp of fp32 is at most U relative), E = 2^-53 (the same for fp64).  fp32 sqrt and divide are correctly rounded in
hipcc's default mode (-fhip-fp32-correctly-rounded-divide-sqrt), so each counts as ONE rounding, like +, - and *.  Every bound below is
the first-order sum of those roundings propagated through the expression; the tests assert SAFETY = 4 times it (sample_ref's factor:
it covers the second-order terms and nothing measured), plus FLOOR = 16 * 2^-149 for results in the subnormal range, where a rounding
is absolute.  Nothing here comes from GPU output.

rmav_adv_moments - x_j = the gathered samples, B of them, d_j = x_j - x_0 (exact in fp64):
    mean64 = x_0 + sum d / B,   M2 = sum (d - sum d / B)^2,   std64 = sqrt(M2 / (B - 1))          [B = 1: 0 / 0 = NaN]
    out[0] = fl32(mean64);   std = fl32(std64);   t = fl32(std + fl32(1e-8));   out[1] = fl32(1 / t)
  The kernel's fp64 part: every lane adds exact d and d^2 (at most B - 1 additions, each E relative to the running sum, which never
  exceeds sum |d| resp. sum d^2), converts (s1, s2) to (mean, s2 - s1^2 / n) and the moments are combined pairwise (Chan) over at most
  ~20 levels; every intermediate is bounded by |x_0| + max |d| resp. sum d^2.  So
      e64(mean) <= E (sum |d| + 64 (|x_0| + max |d|)),      e64(M2) <= E (B + 64) sum d^2
  and std64 inherits half the RELATIVE error of M2.  Then the fp32 roundings, one each:
      bound(out[0]) = e64(mean) + U |mean|
      e(std) = e64(std) + U std;   e(t) = e(std) + U t;   bound(out[1]) = out[1] e(t) / t + U out[1]

rmav_ppo_adam - the header's lines, per element (scalars: omb1 = fl32(1 - beta1), omb2 = fl32(1 - beta2): exact for beta >= 1/2
(Sterbenz), else one rounding each; step_size = fl32(lr / (1 - beta1^step)), bc2_sqrt = fl32(sqrt(1 - beta2^step)): one rounding each,
the fp64 behind them taken as exact).  lr, the betas and eps ARE their fp32 values: the spec holds floats.
      g = grad * grad_scale                       e(g)    = U |g|
      norm = fl32(sqrt(sum g^2))                  e(norm) = (2 U + n E) norm      each g_k is off by U relative, so is the root; + 1 rounding
      t = norm + 1e-6f; ratio = max / t           e(ratio) = ratio (e(norm) / t + 2 U)
      coef = ratio >= 1 ? 1 : ratio               e(coef) = e(ratio) if ratio < 1 + 8 U else 0    (the kernel may sit on the other side of 1)
      gh = g coef                                 e(gh)   = |gh| (U + e(coef) / coef) + U |gh|
      d = gh - m; td = omb1 d; m' = m + td        e(d) = e(gh) + U |d|;  e(td) = omb1 e(d) + (1 + r1) U |td|;  e(m') = e(td) + U |m'|
      a = beta2 v; b = gh gh; c = omb2 b; v' = a + c
                                                  e(a) = U a;  e(b) = 2 |gh| e(gh) + U b;  e(c) = omb2 e(b) + (1 + r2) U c;  e(v') = e(a) + e(c) + U v'
      s = sqrt(v'); q = s / bc2_sqrt; den = q + eps
                                                  e(s) = e(v') / (2 s) + U s;  e(q) = e(s) / bc2_sqrt + 2 U q;  e(den) = e(q) + U den
      r = m' / den; u = step_size r; p' = p - u   e(r) = e(m') / den + |r| e(den) / den + U |r|;  e(u) = step_size e(r) + 2 U |u|;
                                                  e(p') = e(u) + U |p'|
  (r1, r2 = 1 where the beta is below 1/2, else 0.)  Where fp32 overflows the restatement follows it: a result beyond FLT_MAX is an
  infinity, an infinite den makes r = u = 0 and p' = p exactly, and a NaN in grad reaches norm, coef and every output.  Outputs that
  are not finite get bound 0: the kernel has to produce the same infinity / a NaN.

`mutant=` applies one deliberate error (MUTANTS); tests/test_optim_host.py shows each lands at least 10 x outside the asserted bound
on the inputs below with SEED."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
E = 2.0 ** -53
SAFETY = 4.0
FLOOR = 16.0 * 2.0 ** -149
FMAX = float(np.finfo(np.float32).max)
EPS8 = float(np.float32(1e-8))
EPS6 = float(np.float32(1e-6))
# Chosen on the CPU (test_optim_host.py::test_every_mutant_leaves_the_bound): the first seed from 0 at which every mutant clears 10 x.
SEED = 0

MUTANTS = ("biased_std", "no_1e8", "no_1e6", "clip_after_moments", "no_bc1", "no_bc2", "eps_in_sqrt", "g_not_g2", "betas_swapped",
           "step_plus_one", "no_grad_scale")
MOMENT_MUTANTS = MUTANTS[:2]

KINDS = {"quad2d": (5, 2), "quad2d_sl": (9, 2), "quad3d": (10, 4), "quad3d_sl": (16, 4), "reinmav": (13, 4)}
# PPO's hyperparameters as the fp32 values the spec holds
LR, BETA1, BETA2, EPS = (float(np.float32(x)) for x in (3e-4, 0.9, 0.999, 1e-5))


def tensor_sizes(kind, shared):
    """numel of the 13 (shared: 9) parameter tensors, in the order of rmav_ppo_grad (rmav_ppo_grad_shared)."""
    ns, na = KINDS[kind]
    net = [64 * ns, 64, 64 * 64, 64]
    if shared:
        return net + [64 * na, na, 64, 1, na]
    return net + [64 * na, na] + net + [64, 1, na]


# ---- rmav_adv_moments ---------------------------------------------------------------------------------------------------------------------
ADV_INPUTS = ("normal", "constant", "offset")


def adv_input(which, B, seed=None):
    """The fp32 advantages test_gpu_optim.py feeds: N(0, 1); a constant; 1e4 + 1e-2 N(0, 1) (a naive fp32 sum of squares fails it)."""
    rng = np.random.default_rng([SEED if seed is None else seed, ADV_INPUTS.index(which), B])
    z = rng.standard_normal(B)
    x = {"normal": z, "constant": np.full(B, 0.37), "offset": 1e4 + 1e-2 * z}[which]
    return x.astype(np.float32)


def adv_moments(x, mutant=None):
    """x: the gathered samples (fp32 values) -> (out [2], bound [2]) in fp64; bound is the ASSERTED one."""
    assert mutant is None or mutant in MUTANTS, mutant
    x = np.asarray(x, np.float64)
    B = x.size
    d = x - x[0]
    sd = d.sum()
    mean = x[0] + sd / B
    dev = d - sd / B
    m2 = float((dev * dev).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        std = np.sqrt(np.float64(m2) / np.float64(B if mutant == "biased_std" else B - 1))
        t = std + np.float64(0.0 if mutant == "no_1e8" else EPS8)
        out1 = np.float64(1.0) / t
        sum_d2 = float((d * d).sum())
        e_mean = E * (np.abs(d).sum() + 64.0 * (abs(x[0]) + np.abs(d).max())) + U * abs(mean)
        e_std = (0.5 * E * (B + 64) * sum_d2 / m2 * std if m2 > 0 else 0.0) + U * std
        e_t = e_std + U * t
        e_out1 = out1 * e_t / t + U * out1
    out = np.array([mean, out1])
    bound = SAFETY * np.array([e_mean, e_out1]) + FLOOR
    bound[~np.isfinite(out)] = 0.0
    return out, bound


# ---- rmav_ppo_adam ------------------------------------------------------------------------------------------------------------------------
def _o(x):
    """fp32 overflow: beyond FLT_MAX a result is an infinity"""
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(x) > FMAX, np.copysign(np.inf, x), x)


def adam(grad, p, m, v, step, lr=LR, beta1=BETA1, beta2=BETA2, eps=EPS, max_grad_norm=0.5, grad_scale=1.0, mutant=None, exact=False):
    """One rmav_ppo_adam call in fp64 on flat arrays -> dict(p, m, v, norm, coef) and bound_* of each (the ASSERTED bounds).
    exact=True: plain fp64 with no fp32 overflow rule (what torch computes in float64); the bounds then mean nothing."""
    assert mutant is None or mutant in MUTANTS, mutant
    f64 = lambda a: np.asarray(a, np.float64)  # noqa: E731
    grad, p, m, v = f64(grad), f64(p), f64(m), f64(v)
    o = (lambda a: a) if exact else _o
    b1, b2 = (beta2, beta1) if mutant == "betas_swapped" else (beta1, beta2)
    omb1, omb2 = 1.0 - b1, 1.0 - b2
    r1, r2 = float(b1 < 0.5), float(b2 < 0.5)
    k = step + 1 if mutant == "step_plus_one" else step
    bc1 = 1.0 if mutant == "no_bc1" else 1.0 - b1 ** k
    bc2 = 1.0 if mutant == "no_bc2" else 1.0 - b2 ** k
    step_size, bc2_sqrt = lr / bc1, np.sqrt(bc2)
    with np.errstate(all="ignore"):
        g = o(grad * (1.0 if mutant == "no_grad_scale" else grad_scale))
        norm = float(o(np.sqrt((g * g).sum())))
        t = o(norm + (0.0 if mutant == "no_1e6" else EPS6))
        ratio = float(np.float64(max_grad_norm) / np.float64(t))
        coef = 1.0 if ratio >= 1.0 else ratio   # (a NaN stays)
        gh = o(g * coef)
        gm = g if mutant == "clip_after_moments" else gh   # what enters the moments
        d = o(gm - m)
        td = o(omb1 * d)
        m1 = o(m + td)
        a = o(b2 * v)
        b = o(gm if mutant == "g_not_g2" else gm * gm)
        c = o(omb2 * b)
        v1 = o(a + c)
        if mutant == "eps_in_sqrt":
            den = o(np.sqrt(v1 / bc2 + eps))
            s = q = den
        else:
            s = np.sqrt(v1)
            q = o(s / bc2_sqrt)
            den = o(q + eps)
        r = o(m1 / den)
        u = o(step_size * r)
        if mutant == "clip_after_moments":
            u = u * coef
        p1 = o(p - u)
        # ---- the bounds (the docstring's lines) -----------------------------------------------------------------------------------------
        n = grad.size
        e_norm = (2.0 * U + n * E) * norm
        e_ratio = ratio * (e_norm / t + 2.0 * U)
        e_coef = e_ratio if ratio < 1.0 + 8.0 * U else 0.0
        e_gh = np.abs(gh) * (U + e_coef / coef) + U * np.abs(gh)
        e_d = e_gh + U * np.abs(d)
        e_td = omb1 * e_d + (1.0 + r1) * U * np.abs(td)
        e_m = e_td + U * np.abs(m1)
        e_a = U * np.abs(a)
        e_b = 2.0 * np.abs(gh) * e_gh + U * b
        e_c = omb2 * e_b + (1.0 + r2) * U * c
        e_v = e_a + e_c + U * v1
        e_s = np.where(s > 0, e_v / (2.0 * s), 0.0) + U * s
        e_q = e_s / bc2_sqrt + 2.0 * U * q
        e_den = e_q + U * den
        e_r = np.where(np.isinf(den), 0.0, e_m / den + np.abs(r) * e_den / den + U * np.abs(r))
        e_u = step_size * e_r + 2.0 * U * np.abs(u)
        e_p = np.where(np.isinf(den), 0.0, e_u + U * np.abs(p1))
    out = {"p": p1, "m": m1, "v": v1, "norm": np.float64(norm), "coef": np.float64(coef)}
    for name, e in (("p", e_p), ("m", e_m), ("v", e_v), ("norm", e_norm), ("coef", e_coef)):
        bound = SAFETY * np.asarray(e, np.float64) + FLOOR
        out["bound_" + name] = np.where(np.isfinite(out[name]) & np.isfinite(bound), bound, 0.0)
    return out


# The calls test_gpu_optim.py makes per (kind, architecture): name -> (step, max_grad_norm, grad_scale, the norm of grad * grad_scale or a
# special gradient, carried moments?).  Steps 1, 2 and 1000; clip inactive, active (norm = 10 x max, once with a max small enough for the
# 1e-6 to matter) and absent; grad_scale 1, 1/2, 1/3; a zero gradient on non-zero moments; 1e30 everywhere; one NaN.
SCENARIOS = {
    "first_step_inactive": (1, 0.5, 1.0, 0.05, False),
    "active_half": (2, 0.5, 0.5, 5.0, True),
    "active_small_third": (1000, 1e-4, 1.0 / 3.0, 1e-3, True),
    "no_clip": (2, float("inf"), 1.0, 5.0, True),
    "zero_grad": (1000, 0.5, 1.0, "zero", True),
    "huge_no_clip": (2, float("inf"), 1.0, "huge", True),
    "huge_clipped": (2, 0.5, 1.0, "huge", True),
    "one_nan": (2, 0.5, 1.0, "nan", True),
}
FINITE_SCENARIOS = tuple(s for s in SCENARIOS if s not in ("one_nan",))


def adam_case(kind, shared, scenario, seed=None):
    """-> dict(grad, p, m, v: flat float32 arrays; step, max_grad_norm, grad_scale: the call's scalars)"""
    step, max_norm, scale, what, carried = SCENARIOS[scenario]
    n = sum(tensor_sizes(kind, shared))
    rng = np.random.default_rng([SEED if seed is None else seed, sorted(KINDS).index(kind), int(shared), sorted(SCENARIOS).index(scenario)])
    p = (0.3 * rng.standard_normal(n)).astype(np.float32)
    z = rng.standard_normal(n)
    if what == "zero":
        grad = np.zeros(n)
    elif what == "huge":
        grad = np.where(z > 0, 1e30, -1e30)
    elif what == "nan":
        grad = 5.0 * z / np.linalg.norm(z)
        grad[n // 3] = np.nan
    else:
        grad = what * z / (np.linalg.norm(z) * scale)
    typical = 1e-2 if isinstance(what, str) else what / scale / np.sqrt(n)
    m = (typical * rng.standard_normal(n) if carried else np.zeros(n)).astype(np.float32)
    v = ((typical * rng.standard_normal(n)) ** 2 if carried else np.zeros(n)).astype(np.float32)
    return dict(grad=grad.astype(np.float32), p=p, m=m, v=v, step=step, max_grad_norm=max_norm, grad_scale=float(np.float32(scale)))


def split(flat, kind, shared):
    """the flat array cut into the 13 / 9 tensors"""
    out, o = [], 0
    for s in tensor_sizes(kind, shared):
        out.append(flat[o:o + s])
        o += s
    return out


def excess(got, ref, bound):
    """max over the elements of |got - ref| / bound; inf where a non-finite reference value is not reproduced"""
    got, ref, bound = (np.asarray(a, np.float64) for a in (got, ref, bound))
    fin = np.isfinite(ref)
    with np.errstate(all="ignore"):
        diff = np.abs(got - ref)
        q = np.where(fin, np.where(diff == 0.0, 0.0, diff / bound), np.where((got == ref) | (np.isnan(got) & np.isnan(ref)), 0.0, np.inf))
    q = np.where(np.isnan(q), np.inf, q)
    return float(np.max(q))

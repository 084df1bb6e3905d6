"""numpy fp32 restatement of the wind / gust disturbance (rmav_set_disturbance, include/rmav.h) on oracle.philox, and step_ref: the
oracle's step with g_vec + d.  The spec is a dict with the keys of rmav_disturbance_spec: wind_lo (3), wind_hi (3), gust (3), gust_hold.

    wind   w_i = fma(hi_i - lo_i, u(W_i), lo_i)     Philox counter (env_lo, env_hi, reset index of the episode, 5 << 24)
    gust   q_i = fma(g_i + g_i, u(G_i), -g_i)       Philox counter (env_lo, env_hi, low word of b, (6 << 24) | (bits 32..47 of b) << 8),
                                                    b = t // gust_hold
    d_i = w_i + q_i                                 fp32, in this order;  u(x) = (x >> 8) * 2^-24;  key = (seed_lo, seed_hi)

fma in fp32: the product of two fp32 numbers is exact in fp64 (48 significant bits), u has at most 24 bits and so does the other
factor; the sum with the fp32 addend is rounded to fp64 first and then to fp32 - a double rounding that differs from the single one
only when the fp64 sum lands exactly on an fp32 tie, which the exact-arithmetic path below (fractions) rules out: fma32 is exact."""
from fractions import Fraction

import numpy as np

import oracle as O

F32 = np.float32
# the spec the GPU tests run (3-D values; the 2-D kinds read the first two components), and the all-zero one
SPEC = dict(wind_lo=(-1.0, -0.5, 0.25), wind_hi=(1.0, 0.75, 0.25), gust=(0.5, 0.25, 0.125), gust_hold=3)
ZERO = dict(wind_lo=(0.0, 0.0, 0.0), wind_hi=(0.0, 0.0, 0.0), gust=(0.0, 0.0, 0.0), gust_hold=1)
DIM = {"quad2d": 2, "quad2d_sl": 2, "quad3d": 3, "quad3d_sl": 3}


def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, exactly: rational arithmetic, then the nearest fp32 (ties to even)."""
    a, b, c = F32(a), F32(b), F32(c)
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if x == 0:
        # an exact zero: the sign rule of a sum of zeros / of exact cancellation in round-to-nearest is +0 unless both terms are -0
        prod_neg = (np.signbit(a) != np.signbit(b))
        return F32(-0.0) if (prod_neg and np.signbit(c) and float(a) * float(b) == 0.0) else F32(0.0)
    lo = F32(float(x))   # float(Fraction) is correctly rounded to fp64; then to fp32: may double-round, so fix up with the neighbours
    cands = [lo, np.nextafter(lo, F32(np.inf)), np.nextafter(lo, F32(-np.inf))]
    best = min(cands, key=lambda y: (abs(Fraction(float(y)) - x), int(np.frombuffer(F32(y).tobytes(), np.uint32)[0]) & 1))
    return F32(best)


def u01(x):
    return F32(int(x) >> 8) * F32(1.0 / 16777216.0)


def _key(seed):
    return (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def wind(spec, seed, env_id, reset_idx):
    """w [3] fp32 of the episode with reset index `reset_idx` (taken modulo 2^32)."""
    r = O.philox((env_id & 0xFFFFFFFF, (env_id >> 32) & 0xFFFFFFFF, reset_idx & 0xFFFFFFFF, 5 << 24), _key(seed))
    return np.array([fma32(F32(spec["wind_hi"][i]) - F32(spec["wind_lo"][i]), u01(r[i]), spec["wind_lo"][i]) for i in range(3)], F32)


def gust(spec, seed, env_id, t):
    """q [3] fp32 of the step whose step counter is t."""
    b = int(t) // int(spec["gust_hold"])
    r = O.philox((env_id & 0xFFFFFFFF, (env_id >> 32) & 0xFFFFFFFF, b & 0xFFFFFFFF, (6 << 24) | (((b >> 32) & 0xFFFF) << 8)), _key(seed))
    return np.array([fma32(F32(spec["gust"][i]) + F32(spec["gust"][i]), u01(r[i]), -F32(spec["gust"][i])) for i in range(3)], F32)


def disturbance(spec, seed, env_id, reset_idx, t):
    """d [3] fp32 = w + q (one fp32 addition per component)."""
    return (wind(spec, seed, env_id, reset_idx) + gust(spec, seed, env_id, t)).astype(F32)


def disturbance_now(spec, kind, seed, env_ids, reset_counts, t):
    """[3, N] fp32: what rmav_disturbance_now returns for envs with global ids env_ids whose records hold reset_counts (the running
    episode's reset index is the count - 1, modulo 2^32); row 2 is 0 for the 2-D kinds."""
    out = np.zeros((3, len(env_ids)), F32)
    for j, (e, rc) in enumerate(zip(env_ids, reset_counts)):
        out[:DIM[kind], j] = disturbance(spec, seed, int(e), (int(rc) - 1) & 0xFFFFFFFF, t)[:DIM[kind]]
    return out


def step_ref(kind, s, a, sbd, params, d, force_taut=-1):
    """oracle.step per env with g_vec + d: s [n, nS], a [n, nA], sbd [n] (-1 = None), d [3, n] -> (s_next, r, done, sbd_next).
    g_vec + d is the kernel's own sum: in fp32 for the plain kinds, in fp64 for the slung-load kinds."""
    n = len(s)
    o = np.empty((n, s.shape[1]), np.float64)
    r, dn, sb = np.empty(n), np.empty(n, bool), np.empty(n, np.int32)
    g0 = list(params.g_vec)
    for i in range(n):
        for c in range(DIM[kind]):
            params.g_vec[c] = float(F32(g0[c]) + F32(d[c, i])) if kind in ("quad2d", "quad3d") else float(g0[c]) + float(d[c, i])
        o[i], r[i], dn[i], q = O.step(kind, np.asarray(s[i], np.float64), np.asarray(a[i], np.float64), None if sbd[i] < 0 else int(sbd[i]),
                                      params=params, force_taut=force_taut)
        sb[i] = -1 if q is None else q
    for c in range(3):
        params.g_vec[c] = g0[c]
    return o, r, dn, sb


# ---- the inputs of the GPU parity test (tests/test_gpu_disturbance.py), shared with the host test that walks them with the oracle alone ----
# "walk": T = 8 > 2 * gust_hold agent steps under a time limit of 3 (two or more in-launch resets and wind redraws per env) from the
# handle's fresh states.  A taut tether step projects the load to exactly |tether| = L, so EVERY step behind a taut one starts on the
# tether edge, where the branch hangs on the last bit of a norm; the walk of the slung-load kinds therefore runs with a tether longer
# than any distance the U[-1, 1) states reach (always slack: both bodies fall under g_vec + d), and the taut branch is covered by
# "fresh": single steps from freshly reset states (reset indices 1, 2, 3: a taut / slack mixture, none on the edge) with the default tether.
PARITY = dict(seed=11, env_id_base=300, limit=3, steps=8, slack_tether=4.0, fresh=3)


def parity_params(kind, phase):
    """The oracle's params of a phase ("walk" | "fresh")."""
    p = O.default_params(kind)
    if phase == "walk" and kind.endswith("_sl"):
        p.tether_length = PARITY["slack_tether"]
    return p


def parity_actions(kind, n):
    """[steps + fresh, n, nA] fp32: the caller actions of the parity test (a fifth of the kind's action box around its middle)."""
    from util import BOX, NA

    rng = np.random.RandomState(1234 + n)
    lo, hi = BOX[kind]
    return (0.5 * (lo + hi) + 0.1 * (hi - lo) * rng.uniform(-1, 1, (PARITY["steps"] + PARITY["fresh"], n, NA[kind]))).astype(F32)


def oracle_walk(kind, n, spec=SPEC):
    """The parity test's inputs walked with the oracle alone -> (phase, t, pre-step state [n, nS] fp32, d [3, n]) per step.
    "walk": fresh states of reset index 0, step_ref under the spec, auto-reset at termination or at the time limit.
    "fresh": rmav_reset (the next reset index for every env), one step, three times; the step counter runs on."""
    seed, base, H = PARITY["seed"], PARITY["env_id_base"], PARITY["limit"]
    ids = base + np.arange(n)
    s = O.reset_states(kind, seed, ids, 0).astype(F32)
    rc, sbd, el = np.ones(n, np.int64), np.full(n, -1, np.int32), np.zeros(n, np.int64)
    acts = parity_actions(kind, n)
    p = parity_params(kind, "walk")
    t = 0
    for t in range(PARITY["steps"]):
        d = disturbance_now(spec, kind, seed, ids, rc, t)
        yield "walk", t, s.copy(), d
        o, _, dn, sbd = step_ref(kind, s, acts[t], sbd, p, d)
        el += 1
        fin = dn | (el >= H)
        s = o.astype(F32)
        for i in np.nonzero(fin)[0]:
            s[i] = O.reset_state(kind, seed, int(ids[i]), int(rc[i]))
            rc[i] += 1
            el[i] = 0
    for j in range(PARITY["fresh"]):
        t = PARITY["steps"] + j
        s = np.stack([O.reset_state(kind, seed, int(e), int(r)) for e, r in zip(ids, rc)]).astype(F32)
        rc = rc + 1
        yield "fresh", t, s.copy(), disturbance_now(spec, kind, seed, ids, rc, t)

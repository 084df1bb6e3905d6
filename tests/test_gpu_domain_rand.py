"""Per-episode domain randomisation (rmav_set_env_param_range, BatchedQuadrotor(randomize=...)): the constants an env runs an episode
with are redrawn inside the kernels whenever its state is.  Checked against the RNG specification (the tag-4 Philox block of
include/rmav.h) bit for bit, against the oracle run with each env's own constants, and against fixed per-env arrays for the degenerate
range.  Tolerances are the project's: TOL, CTRL_TOL, scaled_err and near_threshold (util.py); every oracle comparison asserts that what
it exempts as near a threshold is at most 1 % of what it compares."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
from util import BOX, CTRL_TOL, KINDS, NA, NS, TOL, near_threshold, random_cases, scaled_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mass", "load_mass", "tether_length")
RANGES = {"mass": (0.8, 1.25), "load_mass": (0.05, 0.2), "tether_length": (0.6, 1.4)}
_fmaf = C.CDLL("libm.so.6").fmaf
_fmaf.restype = C.c_float
_fmaf.argtypes = [C.c_float] * 3


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import gym_reinmav_amd as g

    return g


_cache = {}


def draw(seed, env_id, ep, name, lo=None, hi=None):
    """The specification: word `which` of Philox4x32-10(counter (env_lo, env_hi, ep, 4 << 24), key (seed_lo, seed_hi)) ->
    u = (x >> 8) * 2^-24, value = fmaf(hi - lo, u, lo) in fp32."""
    if lo is None:
        lo, hi = RANGES[name]
    key = (seed, int(env_id), int(ep) & 0xFFFFFFFF)
    if key not in _cache:
        _cache[key] = O.philox((env_id & 0xFFFFFFFF, env_id >> 32, int(ep) & 0xFFFFFFFF, 4 << 24), (seed & 0xFFFFFFFF, seed >> 32))
    x = int(_cache[key][NAMES.index(name)])
    u = np.float32(x >> 8) * np.float32(2.0 ** -24)
    lo32, hi32 = np.float32(lo), np.float32(hi)
    return np.float32(_fmaf(np.float32(hi32 - lo32), u, lo32))


def draws(seed, ids, eps, name, lo=None, hi=None):
    return np.array([draw(seed, int(e), int(k), name, lo, hi) for e, k in zip(ids, np.broadcast_to(eps, np.shape(ids)))], np.float32)


def ranged_names(kind):
    return NAMES if kind.endswith("_sl") else ("mass",)


def params_of(kind, vals, i):
    q = O.default_params(kind)
    q.mass = float(vals["mass"][i])
    if kind.endswith("_sl"):
        q.load_mass, q.tether_length = float(vals["load_mass"][i]), float(vals["tether_length"][i])
    return q


def oracle_steps(kind, prev, act, sbd, vals, idx):
    """the oracle from each env's own (state, action, steps_beyond_done, constants), for the envs of idx"""
    o = np.empty((len(idx), NS[kind]))
    r = np.empty(len(idx))
    d = np.empty(len(idx), bool)
    for j, i in enumerate(idx):
        q = params_of(kind, vals, i)
        o[j], r[j], d[j], _ = O.step(kind, prev[i].astype(np.float64), act[i].astype(np.float64), None if sbd[i] < 0 else int(sbd[i]), params=q)
    return o, r, d


class Forced:
    """Teacher-forced check of a trajectory against the oracle, over one or more launches of one handle."""

    def __init__(self, env, kind, seed, base, idx):
        self.env, self.kind, self.seed, self.base, self.idx = env, kind, seed, base, np.asarray(idx)
        self.n = env.num_envs
        self.prev = env.get_state()
        self.sbd = env.get_sbd()
        self.rc = env.get_reset_counts().copy()
        self.vals = {nm: env.get_env_param(nm) for nm in NAMES}
        self.compared = self.exempt = self.resets = 0
        self.max_resets = np.zeros(self.n, np.int64)

    def launch(self, tr, check_actions=None):
        kind, idx = self.kind, self.idx
        T = tr["obs"].shape[0]
        for k in range(T):
            act = tr["actions"][k]
            if check_actions == "controller":
                for i in idx[::8]:
                    q = params_of(kind, self.vals, i)
                    assert scaled_err(act[i], O.control(kind, self.prev[i].astype(np.float64), params=q)).max() <= CTRL_TOL
            o2, r, d = oracle_steps(kind, self.prev, act, self.sbd, self.vals, idx)
            dk = tr["done"][k].astype(bool)
            fin = np.isfinite(o2).all(axis=1)
            # exempt: a terminating norm within 1e-5 of its limit (util.near_threshold); the oracle and the device start from the same
            # fp32 state and the same constants, so the tether-edge rule of test_gpu_parity.py is not needed and not used
            near = near_threshold(kind, np.where(fin[:, None], o2, 0.0)) | ~fin   # (a state the oracle overflows from: exempt, and counted)
            # which finished episodes the time limit ended: the launch's own flags where it reports them (rmav_step_final, the *_boot
            # rollouts); otherwise a done at running length >= H (tr["at_limit"]) that the oracle does not terminate
            if "trunc" in tr:
                trunc = tr["trunc"][k][idx].astype(bool)
            elif "at_limit" in tr:
                trunc = tr["at_limit"][k][idx] & ~d
            else:
                trunc = np.zeros(len(idx), bool)
            self.compared += len(idx)
            self.exempt += int(near.sum())
            term = dk[idx] & ~trunc
            assert np.array_equal(term | near, d | near)
            alive = ~dk[idx] & ~d & ~near & fin
            assert scaled_err(tr["obs"][k][idx][alive], o2[alive]).max(initial=0.0) <= TOL
            ok = (term == d) & ~near & fin
            assert scaled_err(tr["rew"][k][idx][ok], r[ok]).max(initial=0.0) <= TOL
            # steps_beyond_done follows the device (terminations only; kept for the sampled envs)
            self.sbd[idx] = np.where(term, np.where(self.sbd[idx] < 0, 0, self.sbd[idx] + 1), self.sbd[idx])
            # a finished env: the fresh state of reset index rc, and the constants of that reset index from then on
            fi = np.nonzero(dk)[0]
            fs = fi[np.isin(fi, idx)]
            if len(fs):
                assert np.array_equal(tr["obs"][k][fs], O.reset_states(kind, self.seed, self.base + fs, self.rc[fs]))
            for nm in ranged_names(kind):
                if len(fi):
                    sel = fi if len(fi) <= 64 else fs
                    self.vals[nm][sel] = draws(self.seed, self.base + sel, self.rc[sel], nm)
                    rest = np.setdiff1d(fi, sel)
                    self.vals[nm][rest] = np.nan   # (not a sampled env: never used below)
            self.rc = self.rc + dk.astype(np.uint32)
            self.max_resets += dk
            self.resets += int(dk[idx].sum())
            self.prev = tr["obs"][k]

    def finish(self):
        env = self.env
        assert np.array_equal(env.get_reset_counts(), self.rc)
        for nm in ranged_names(self.kind):
            got = env.get_env_param(nm)
            assert np.array_equal(got[self.idx], draws(self.seed, self.base + self.idx, self.rc[self.idx] - 1, nm)), nm
            known = ~np.isnan(self.vals[nm])
            assert np.array_equal(got[known], self.vals[nm][known]), nm
        assert self.exempt <= 0.01 * self.compared, (self.exempt, self.compared)


def at_limit(done, limit, ln):
    """[T, N]: the steps at which a done may be a truncation - the running length (ln before the launch, updated in place) has
    reached the limit; no length ever passes it"""
    at = np.zeros(done.shape, bool)
    for k in range(done.shape[0]):
        ln += 1
        dk = done[k].astype(bool)
        at[k] = dk & (ln >= limit)
        assert (ln <= limit).all()
        ln[dk] = 0
    return at


def widen(env, kind, f=None):
    """half of the states three times as wide (util.random_cases): a good part of the envs ends its episode in the next step"""
    s, _ = random_cases(kind, env.num_envs, seed=5)
    env.set_state(s)
    return s


def make_env(G, kind, n, seed, base=0, **kw):
    env = G.BatchedQuadrotor(kind, n, seed=seed, env_id_base=base, **kw)
    for nm in ranged_names(kind):
        env.set_env_param_range(nm, *RANGES[nm])
    return env


# ---- 1. the draw rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["quad2d", "quad3d_sl"])
@pytest.mark.parametrize("base", [0, 2 ** 40 + 12345])
def test_draw_rule_bit_exact(G, kind, base):
    n, seed = 1500, 0x1234_5678_9ABC
    env = G.BatchedQuadrotor(kind, n, seed=seed, env_id_base=base)
    ids = base + np.arange(n)
    for nm in NAMES:   # (a parameter the kind does not read is accepted like rmav_set_env_param accepts it)
        assert env.get_env_param_range(nm) is None
        env.set_env_param_range(nm, *RANGES[nm])
        assert env.get_env_param_range(nm) == tuple(float(np.float32(v)) for v in RANGES[nm])
        got = env.get_env_param(nm)
        assert got.dtype == np.float32 and np.array_equal(got, draws(seed, ids, 0, nm)), nm
        lo, hi = np.float32(RANGES[nm][0]), np.float32(RANGES[nm][1])
        assert (got >= lo).all() and (got <= hi).all() and got.std() > 0.1 * (hi - lo)
    env.reset()
    for nm in NAMES:
        assert np.array_equal(env.get_env_param(nm), draws(seed, ids, 1, nm)), nm
        assert np.array_equal(env.get_env_param(nm, device_out=True).cpu().numpy(), draws(seed, ids, 1, nm)), nm
    twin = G.BatchedQuadrotor(kind, n, seed=seed, env_id_base=base, randomize=RANGES)
    twin.reset()
    for nm in NAMES:
        assert np.array_equal(twin.get_env_param(nm), env.get_env_param(nm))
    # a parameter without an array reports the shared value
    plain = G.BatchedQuadrotor(kind, 70, seed=1)
    assert np.array_equal(plain.get_env_param("mass"), np.full(70, np.float32(plain.params.mass)))
    assert np.array_equal(plain.get_env_param("tether_length", device_out=True).cpu().numpy(), np.full(70, np.float32(plain.params.tether_length)))
    for e in (env, twin, plain):
        e.close()


# ---- 2. single steps ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("limit", [None, 3])
def test_single_steps_vs_oracle(G, kind, limit):
    """rmav_step, rmav_step_final, rmav_step_control and rmav_control_step with auto-reset: each sampled env against the oracle with its
    own constants; a finished env returns the fresh state of its next reset index and holds that index's constants; the trailing
    control() of rmav_step_control on a just-reset env uses the new ones."""
    n, seed, base = 4096, 21, 777
    env = make_env(G, kind, n, seed, base, auto_reset=True, track_episodes=True, max_episode_steps=limit)
    s, _ = random_cases(kind, n, seed=5)      # half of the states three times as wide: a good part of them terminates at once
    env.set_state(s)
    idx = np.arange(0, n, 5)
    f = Forced(env, kind, seed, base, idx)
    rng = np.random.RandomState(3)
    lo, hi = BOX[kind]
    n_reset_ctrl = 0
    for it, call in enumerate(("step", "step_final", "step_control", "control_step", "step", "step_control")):
        a = rng.uniform(lo, hi, (n, NA[kind])).astype(np.float32)
        tr = {}
        if call == "step_control":   # a good part of the envs terminates in this very launch: its control() runs on fresh states
            env.set_state(s)
            f.prev = s.copy()
        if call == "step":
            obs, rew, done = env.step(a)
        elif call == "step_final":
            obs, rew, done, fin, trunc = env.step_final(a)
            tr["trunc"] = trunc[None]
        elif call == "step_control":
            obs, rew, done, nxt = env.step_control(a)
        else:
            a, obs, rew, done = env.control_step()
        if limit and "trunc" not in tr:   # which of the finished episodes the limit ended
            tr["trunc"] = (env.episode_truncated().astype(bool) & np.asarray(done).astype(bool))[None]
        tr.update(actions=a[None], obs=obs[None], rew=rew[None], done=np.asarray(done)[None])
        f.launch(tr, check_actions="controller" if call == "control_step" else None)
        if call == "step_control":   # control() of the state the launch left, with the constants now in force
            vals = {nm: env.get_env_param(nm) for nm in NAMES}
            dn = np.asarray(done).astype(bool)
            pick = np.concatenate([np.nonzero(dn)[0][:150], idx[:100]])
            n_reset_ctrl += int(dn[pick].sum())
            for i in pick:
                assert scaled_err(nxt[i], O.control(kind, obs[i].astype(np.float64), params=params_of(kind, vals, i))).max() <= CTRL_TOL
    assert f.resets >= 50 and n_reset_ctrl >= 20, (f.resets, n_reset_ctrl)
    f.finish()
    env.close()


# ---- 3. fused rollouts -------------------------------------------------------------------------------------------------------------
def _rollout(env, kind, T, mode, layout, fused, actions=None):
    want = ("actions", "obs", "rew", "done")
    if layout == "plain":
        tr = env.rollout(T, mode=mode, actions=actions, layout="aos", fused=fused, want=want)
        return {k: np.asarray(v) for k, v in tr.items()}
    import torch

    if layout == "pitched":
        tr = env.rollout(T, mode=mode, layout="soa", fused=fused, want=want, device_out=True, pitched=True)
        tr = {k: v.contiguous() for k, v in tr.items()}
    elif layout == "soa_dev":
        a = None if actions is None else torch.from_numpy(np.ascontiguousarray(actions.transpose(0, 2, 1))).cuda()
        tr = env.rollout(T, mode=mode, actions=a, layout="soa", fused=fused, want=want, device_out=True)
    else:
        tr = env.rollout_chunked(T, mode=mode, chunk=1024, want=want)
        tr = {k: env.unchunk(v) for k, v in tr.items()}
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in tr.items()}
    out["actions"], out["obs"] = out["actions"].transpose(0, 2, 1), out["obs"].transpose(0, 2, 1)
    return out


CONFIGS = [("random", 64, None, "plain"), ("random", 200, None, "pitched"), ("random", 64, 20, "chunked"), ("random", 200, 50, "plain"),
           ("buffer", 64, None, "plain"), ("buffer", 200, 30, "soa_dev"), ("controller", 64, None, "chunked"),
           ("controller", 200, 25, "pitched"), ("controller", 64, 10, "plain")]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode,T,limit,layout", CONFIGS)
def test_fused_rollouts_teacher_forced(G, kind, mode, T, limit, layout):
    n, seed, base = 4096, 11, 123456
    envs = [make_env(G, kind, n, seed, base, auto_reset=True, track_episodes=True, max_episode_steps=limit) for _ in range(2)]
    for e in envs:
        widen(e, kind)
    ln = np.zeros(n, np.int64)
    idx = np.arange(3, n, 16)
    f = Forced(envs[0], kind, seed, base, idx)
    rng = np.random.RandomState(9)
    lo, hi = BOX[kind]
    for launch in range(2):   # the second launch continues from the constants the first one left
        Tl = T if launch == 0 else 16
        acts = rng.uniform(lo, hi, (Tl, n, NA[kind])).astype(np.float32) if mode == "buffer" else None
        tr = _rollout(envs[0], kind, Tl, mode, layout, True, acts)
        if mode == "buffer":
            tr["actions"] = acts
        if limit:
            tr["at_limit"] = at_limit(tr["done"], limit, ln)
        f.launch(tr, check_actions="controller" if mode == "controller" else None)
        # the unfused call: the same bits
        tu = _rollout(envs[1], kind, Tl, mode, "plain" if layout in ("chunked", "pitched") else layout, False, acts)
        for key in ("obs", "rew", "done") + (("actions",) if mode != "buffer" else ()):
            assert np.array_equal(tr[key], tu[key]), (key, launch)
    f.finish()
    if mode == "random" and T == 200:
        assert int(f.max_resets.max()) >= 2, "no env reset more than once inside a launch"
    assert f.resets >= 10, f.resets
    for nm in NAMES:
        assert np.array_equal(envs[0].get_env_param(nm), envs[1].get_env_param(nm)), nm
    assert np.array_equal(envs[0].get_state(), envs[1].get_state())
    assert envs[0].episode_totals()["episodes"] == envs[1].episode_totals()["episodes"]
    for e in envs:
        e.close()


# ---- 5. the degenerate range -------------------------------------------------------------------------------------------------------
def _snapshot(env):
    eb = env.episode_buffers()
    return dict(state=env.get_state(), sbd=env.get_sbd(), rc=env.get_reset_counts(), tot=tuple(env.episode_totals().values()),
                **{k: np.asarray(v) for k, v in eb.items()}, **{nm: env.get_env_param(nm) for nm in NAMES})


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("limit", [None, 12])
def test_degenerate_range_equals_fixed_arrays(G, kind, limit):
    """lo == hi == v: every launch gives the bits of a handle holding N copies of v (rmav_set_env_param) - steps and fused rollouts."""
    n, seed = 4096 + 37, 4
    v = {"mass": 1.1, "load_mass": 0.15, "tether_length": 0.9}
    a_env = G.BatchedQuadrotor(kind, n, seed=seed, max_episode_steps=limit)
    b_env = G.BatchedQuadrotor(kind, n, seed=seed, max_episode_steps=limit)
    for nm in NAMES:
        a_env.set_env_param_range(nm, v[nm], v[nm])
        b_env.set_env_param(nm, np.full(n, v[nm], np.float32))
    _same(_snapshot(a_env), _snapshot(b_env))
    rng = np.random.RandomState(2)
    lo, hi = BOX[kind]
    for call in ("step", "step_final", "step_control", "control_step"):
        a = rng.uniform(lo, hi, (n, NA[kind])).astype(np.float32)
        ra = getattr(a_env, call)(*(() if call == "control_step" else (a,)))
        rb = getattr(b_env, call)(*(() if call == "control_step" else (a,)))
        for x, y in zip(ra, rb):
            assert np.array_equal(x, y), call
    for mode, T, fused in (("random", 64, True), ("controller", 40, True), ("buffer", 24, True), ("random", 5, True), ("random", 9, False)):
        acts = rng.uniform(lo, hi, (T, n, NA[kind])).astype(np.float32) if mode == "buffer" else None
        ta = a_env.rollout(T, mode=mode, actions=acts, layout="aos", fused=fused, want=("actions", "obs", "rew", "done"))
        tb = b_env.rollout(T, mode=mode, actions=acts, layout="aos", fused=fused, want=("actions", "obs", "rew", "done"))
        for key in ta:
            assert np.array_equal(ta[key], tb[key]), (mode, key)
        _same(_snapshot(a_env), _snapshot(b_env))
    assert a_env.episode_totals()["episodes"] > 100
    a_env.close()
    b_env.close()


# ---- 6. shard invariance -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["quad2d_sl", "quad3d_sl"])
def test_shard_invariance(G, kind):
    # (256 steps: from reset states a quadrotor3d-slungload episode lasts 60 - 90 steps - it has to fall out of its box - so a launch of
    # 96 steps sees at most one reset per env; the on-demand redraw of a second reset has to be part of this)
    n, seed, T = 4096, 31, 256
    full = make_env(G, kind, n, seed, 0)
    parts = [make_env(G, kind, n // 2, seed, b) for b in (0, n // 2)]
    tf = full.rollout(T, mode="random", layout="aos", want=("actions", "obs", "rew", "done"))
    tp = [p.rollout(T, mode="random", layout="aos", want=("actions", "obs", "rew", "done")) for p in parts]
    for key in tf:
        assert np.array_equal(tf[key], np.concatenate([t[key] for t in tp], axis=1)), key
    for nm in NAMES:
        assert np.array_equal(full.get_env_param(nm), np.concatenate([p.get_env_param(nm) for p in parts])), nm
    assert np.array_equal(full.get_state(), np.concatenate([p.get_state() for p in parts]))
    assert int((full.get_reset_counts() - 1).max()) >= 2
    for e in [full] + parts:
        e.close()


# ---- 7. the state rule -------------------------------------------------------------------------------------------------------------
def test_state_rule(G):
    from gym_reinmav_amd import _abi as A

    kind, n, seed = "quad3d_sl", 2048, 8
    env = make_env(G, kind, n, seed)
    ids = np.arange(n)
    v0 = {nm: env.get_env_param(nm) for nm in NAMES}
    env.set_state(env.get_state() * 0.5)
    env.set_reset_counts(env.get_reset_counts() + 3)
    env.step_count = 100
    for nm in NAMES:
        assert np.array_equal(env.get_env_param(nm), v0[nm]), nm
    env.seed(99)
    for nm in NAMES:
        assert np.array_equal(env.get_env_param(nm), v0[nm]), nm
    # explicit values on a ranged parameter last until each env's next reset; the range stays
    env.set_reset_counts(np.full(n, 1, np.uint32))
    fixed = np.full(n, 1.5, np.float32)
    env.set_env_param("mass", fixed)
    assert env.get_env_param_range("mass") is not None
    assert np.array_equal(env.get_env_param("mass"), fixed)
    widen(env, kind)   # every other env three times as wide: most of those end their episode in the first steps, the rest go on
    tr = env.rollout(8, mode="random", layout="aos", want=("done",))
    nres = tr["done"].astype(np.int64).sum(axis=0)
    got = env.get_env_param("mass")
    assert (nres == 0).sum() > 20 and (nres > 0).sum() > 50
    assert np.array_equal(got[nres == 0], fixed[nres == 0])
    hit = np.nonzero(nres > 0)[0][:300]
    assert np.array_equal(got[hit], draws(99, hit, nres[hit], "mass"))   # reset index of the running episode = 1 + resets - 1
    # NULL clears the range and the array
    env.set_env_param("mass", None)
    assert env.get_env_param_range("mass") is None
    assert np.array_equal(env.get_env_param("mass"), np.full(n, np.float32(env.params.mass)))
    env.set_env_param_range("tether_length", None)
    assert env.get_env_param_range("tether_length") is None and env.get_env_param_range("load_mass") is not None
    env.close()
    # without auto-reset only reset() redraws
    env = make_env(G, kind, n, seed, auto_reset=False)
    v0 = env.get_env_param("mass")
    s, a = random_cases(kind, n, seed=1)
    env.set_state(s)
    _, _, done = env.step(a)
    assert done.sum() > 100
    env.rollout(20, mode="random", want=())
    assert np.array_equal(env.get_env_param("mass"), v0)
    env.reset()
    assert np.array_equal(env.get_env_param("mass"), draws(seed, ids, 1, "mass"))
    # invalid ranges, ReinmavEnv
    L = A.lib()
    for lo, hi in ((0.0, 1.0), (-1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (1.0, float("inf")), (float("inf"), float("inf"))):
        assert L.rmav_set_env_param_range(env._h, 0, lo, hi) == A.ERR_INVALID, (lo, hi)
    assert L.rmav_set_env_param_range(env._h, 3, 1.0, 2.0) == A.ERR_INVALID
    assert np.array_equal(env.get_env_param("mass"), draws(seed, ids, 1, "mass"))
    env.close()
    r = G.BatchedQuadrotor("reinmav", 64)
    assert L.rmav_set_env_param_range(r._h, 0, 1.0, 2.0) == A.ERR_INVALID
    out = np.zeros(64, np.float32)
    assert L.rmav_get_env_param(r._h, 0, out.ctypes.data, A.HOST) == A.ERR_INVALID
    r.close()


# ---- 4. policy rollouts ------------------------------------------------------------------------------------------------------------
def _collector(G, env, kind, actor, T, boot=False, norm=False, seed=0):
    import torch

    from gym_reinmav_amd.obs_norm import RunningObsNorm
    from gym_reinmav_amd.ppo import FusedPolicyCollector, MlpPolicy

    torch.manual_seed(seed)
    on = RunningObsNorm(env.nS, f"cuda:{env.device}") if norm else None
    pol = MlpPolicy(env.nS, env.nA, obs_norm=on, value_network="shared" if actor == "shared" else "copy").cuda()
    with torch.no_grad():
        if kind.startswith("quad3d"):
            pol.pi[2].bias[0] = 9.8
    return FusedPolicyCollector(env, pol, T, f16_mfma=(actor == "f16"), f32_mfma=(actor == "f32m") or None,
                                bootstrap_truncated=boot)


def _collected(col):
    import torch

    torch.cuda.synchronize()
    tr = dict(actions=col.act.cpu().numpy().transpose(0, 2, 1), obs=col.obs[1:].cpu().numpy().transpose(0, 2, 1),
              rew=col.rew.cpu().numpy(), done=col.done.cpu().numpy())
    if col.trunc is not None:
        tr["trunc"] = col.trunc.cpu().numpy().astype(bool)
    return tr


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("actor", ["f32m", "f16", "shared"])
@pytest.mark.parametrize("variant", ["plain", "limit", "boot", "norm", "norm_boot"])
def test_policy_rollouts_teacher_forced(G, kind, actor, variant):
    """FusedPolicyCollector (rmav_rollout_policy / _boot / _norm): the env transitions of the in-kernel actor's own actions against the
    oracle with each env's constants, the redraw at every reset; and the same launch on a degenerate range gives the bits of fixed arrays."""
    n, seed, base, T = 2048, 17, 4242, 96
    boot, norm = variant.endswith("boot"), variant.startswith("norm")
    limit = 24 if (boot or variant == "limit") else None   # ("limit": rmav_rollout_policy on a time-limited handle, no bootstrap term asked for)
    env = make_env(G, kind, n, seed, base, max_episode_steps=limit)
    widen(env, kind)
    f = Forced(env, kind, seed, base, np.arange(1, n, 16))
    col = _collector(G, env, kind, actor, T, boot=boot, norm=norm)
    ln = np.zeros(n, np.int64)
    for _ in range(2):
        col.collect()
        tr = _collected(col)
        if limit and "trunc" not in tr:
            tr["at_limit"] = at_limit(tr["done"], limit, ln)
        f.launch(tr)
        col.roll_over()
    f.finish()
    assert f.resets >= 10, f.resets
    env.close()
    # degenerate range == fixed arrays, every output of the launch
    outs = []
    for ranged in (True, False):
        e = G.BatchedQuadrotor(kind, n, seed=seed, env_id_base=base, max_episode_steps=limit)
        widen(e, kind)
        for nm in ranged_names(kind):
            if ranged:
                e.set_env_param_range(nm, 1.1, 1.1)
            else:
                e.set_env_param(nm, np.full(n, 1.1, np.float32))
        c = _collector(G, e, kind, actor, T, boot=boot, norm=norm)
        c.collect()
        import torch

        torch.cuda.synchronize()
        o = dict(_collected(c), logp=c.logp.cpu().numpy(), val=c.val.cpu().numpy(), **_snapshot(e))
        if boot:
            o["boot"] = c.boot.cpu().numpy()
        outs.append(o)
        e.close()
    _same(outs[0], outs[1])


def test_policy_rollout_raw_abi_and_unsupported_actors(G):
    """rmav_rollout_policy straight through the ABI on a ranged handle equals the collector's launch; the fp32 vector-ALU and bf16
    actors return RMAV_ERR_INVALID."""
    import torch

    from gym_reinmav_amd import _abi as A

    kind, n, T, seed = "quad3d", 1024, 32, 3
    L = A.lib()
    env = make_env(G, kind, n, seed)
    widen(env, kind)
    col = _collector(G, env, kind, "f32m", T)
    col._pack()
    dev = col.obs.device
    act, obs = torch.empty((T, env.nA, n), device=dev), torch.empty((T, env.nS, n), device=dev)
    rew, done = torch.empty((T, n), device=dev), torch.empty((T, n), dtype=torch.uint8, device=dev)
    logp, val = torch.empty((T, n), device=dev), torch.empty((T + 1, n), device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for prec in (A.POLICY_FP32, A.POLICY_BF16_MFMA):
        assert L.rmav_rollout_policy(env._h, T, p(col.weights), p(act), p(obs), p(rew), p(done), p(logp), p(val), prec) == A.ERR_INVALID
    twin = make_env(G, kind, n, seed)
    widen(twin, kind)
    A.check(L.rmav_rollout_policy(twin._h, T, p(col.weights), p(act), p(obs), p(rew), p(done), p(logp), p(val), A.POLICY_FP32_MFMA))
    col.collect()
    torch.cuda.synchronize()
    assert torch.equal(col.obs[1:], obs) and torch.equal(col.act, act) and torch.equal(col.val, val) and torch.equal(col.done, done)
    assert np.array_equal(env.get_env_param("mass"), twin.get_env_param("mass"))
    assert int(done.sum()) > 50
    env.close()
    twin.close()


# ---- 9. the Python surface ---------------------------------------------------------------------------------------------------------
def test_python_surface(G):
    from gym_reinmav_amd.distributed import make_sharded

    rz = {"mass": (0.8, 1.2)}
    ve = G.QuadrotorVecEnv("quadrotor3d-v0", 512, seed=6, randomize=rz)
    assert np.array_equal(ve.env.get_env_param("mass"), draws(6, np.arange(512), 0, "mass", 0.8, 1.2))
    ve.reset()
    assert np.array_equal(ve.env.get_env_param("mass"), draws(6, np.arange(512), 1, "mass", 0.8, 1.2))
    ve.close()
    sh = make_sharded("quad3d", 1000, 1, 2, device=0, seed=6, randomize=rz)
    assert np.array_equal(sh.get_env_param("mass"), draws(6, 500 + np.arange(500), 0, "mass", 0.8, 1.2))
    sh.close()
    e = G.make("quadrotor3d-v0", seed=6, randomize=rz)   # the gym-shaped single env: reset() redraws
    assert np.array_equal(e._batch.get_env_param("mass"), draws(6, [0], 0, "mass", 0.8, 1.2))
    m = []
    for k in range(1, 4):
        e.reset()
        m.append(float(e._batch.get_env_param("mass")[0]))
        assert m[-1] == float(draw(6, 0, k, "mass", 0.8, 1.2))
        a = e.control()
        e.step(a)
        assert float(e._batch.get_env_param("mass")[0]) == m[-1]
    assert len(set(m)) == 3
    e.close()


def test_train_ppo2_with_randomize_runs():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "reinmav-gym_amd"), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_ppo2.py"), "--num_env", "1024", "--nsteps", "32",
                        "--num_timesteps", str(3 * 1024 * 32), "--randomize", "mass=0.8:1.2"], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]

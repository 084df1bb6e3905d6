"""Episode time limits (rmav_set_time_limit, BatchedQuadrotor(max_episode_steps=H)): truncation inside the step kernels, checked
against resets at the right moment, the oracle, the kernels without a limit and the single-step path, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from util import BOX, KINDS, TOL, near_threshold, scaled_err

pytestmark = pytest.mark.gpu

N = 4096


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import gym_reinmav_amd as g

    return g


def _lengths(done, ln0=None):
    """per step: the running length after the step (before a done resets it); done [T, N]"""
    T, n = done.shape
    ln = np.zeros(n, np.int64) if ln0 is None else ln0.copy()
    out = np.empty((T, n), np.int64)
    for k in range(T):
        ln += 1
        out[k] = ln
        ln[done[k].astype(bool)] = 0
    return out, ln


def _wide(G, kind):
    """the default constants with a wider box: the comparisons below are about the envs that do not terminate, and under the
    controller some leave the default box within 100 steps"""
    p = G._abi.default_params(G._abi.KIND_BY_NAME[kind])
    # (quadrotor2d: no box at all - its controller drives every env out of any box within 100 steps; the states stay finite)
    p.pos_limit = p.vel_limit = 1e30 if kind == "quad2d" else 20.0
    return p


@pytest.mark.parametrize("kind", KINDS)
def test_truncation_is_a_reset_at_the_right_moment(G, kind):
    H, T, seed = 25, 100, 5
    lim = G.BatchedQuadrotor(kind, N, seed=seed, max_episode_steps=H, params=_wide(G, kind))
    twin = G.BatchedQuadrotor(kind, N, seed=seed, params=_wide(G, kind))
    assert lim.max_episode_steps == H and twin.max_episode_steps is None
    tr = lim.rollout(T, mode="controller", layout="aos", want=("obs", "rew", "done"))
    obs, rew, done = [], [], []
    for j in range(T // H):
        t2 = twin.rollout(H, mode="controller", layout="aos", want=("obs", "rew", "done"))
        o = t2["obs"].copy()
        o[H - 1] = twin.reset()          # what auto-reset puts there at the limit
        obs.append(o)
        rew.append(t2["rew"])
        done.append(t2["done"])
    obs, rew, done = np.concatenate(obs), np.concatenate(rew), np.concatenate(done)
    marks = np.arange(H - 1, T, H)
    other = np.ones(T, bool)
    other[marks] = False
    keep = ~done.any(axis=0) & ~tr["done"][other].any(axis=0)
    assert keep.mean() >= 0.75, keep.mean()
    assert tr["done"][marks][:, keep].all()
    assert np.array_equal(tr["obs"][:, keep], obs[:, keep])
    assert np.array_equal(tr["rew"][:, keep], rew[:, keep])
    assert np.array_equal(lim.get_state()[keep], twin.get_state()[keep])
    assert np.array_equal(lim.get_reset_counts()[keep], twin.get_reset_counts()[keep])
    assert np.array_equal(lim.get_sbd()[keep], twin.get_sbd()[keep])
    assert (lim.episode_truncated()[keep] == 1).all()
    eb = lim.episode_buffers()
    assert (eb["last_length"][keep] == H).all() and (eb["cur_length"][keep] == 0).all()
    # totals: every finished episode of every env, with the lengths the done pattern implies
    lens, _ = _lengths(tr["done"])
    tot = lim.episode_totals()
    d = tr["done"].astype(bool)
    assert tot["episodes"] == int(d.sum()) and tot["length_sum"] == int(lens[d].sum())
    assert int(d[:, keep].sum()) == 4 * int(keep.sum())
    lim.close()
    twin.close()


def _teacher_forced(G, kind, H, launches, seed=11, base=123456):
    lo, hi = BOX[kind]
    env = G.BatchedQuadrotor(kind, N, seed=seed, env_id_base=base, max_episode_steps=H)
    prev = env.get_state()
    sbd = env.get_sbd()
    rc = env.get_reset_counts().copy()
    ids = base + np.arange(N)
    ret = np.zeros(N)
    ln = np.zeros(N, np.int64)
    last_trunc = np.zeros(N, np.uint8)
    fin_ret, fin_len, fin_n, n_trunc = 0.0, 0, 0, 0
    t = 0
    for T in launches:
        tr = env.rollout(T, mode="random", layout="aos", want=("actions", "obs", "rew", "done"))
        for k in range(T):
            if t < 3:
                assert np.array_equal(tr["actions"][k], O.random_actions(kind, seed, ids, t, lo, hi))
            t += 1
            sbd_prev = sbd.copy()
            o2, r, d, sbd = O.batch_step(kind, prev.astype(np.float64), tr["actions"][k].astype(np.float64), sbd)
            dk = tr["done"][k].astype(bool)
            at_limit = ln + 1 >= H
            # a finished episode was truncated iff its reward is the ordinary -dist (< 0), terminated iff the terminal 1 / 0
            trunc = dk & (tr["rew"][k] < 0)
            term = dk & ~trunc
            assert np.array_equal(dk, term | at_limit)
            assert np.array_equal(trunc, at_limit & ~term)
            ok = near_threshold(kind, o2)
            assert np.array_equal(term | ok, d | ok)
            sbd = np.where(term == d, sbd, np.where(term, np.where(sbd_prev < 0, 0, sbd_prev + 1), sbd_prev))
            alive = ~dk & ~d
            assert scaled_err(tr["obs"][k][alive], o2[alive]).max(initial=0.0) <= TOL
            same = term == d
            assert scaled_err(tr["rew"][k][same], r[same]).max(initial=0.0) <= TOL
            if dk.any():
                assert np.array_equal(tr["obs"][k][dk], O.reset_states(kind, seed, ids[dk], rc[dk]))
            rc = rc + dk.astype(np.uint32)
            ret += tr["rew"][k]
            ln += 1
            fin_ret += ret[dk].sum()
            fin_len += ln[dk].sum()
            fin_n += int(dk.sum())
            n_trunc += int(trunc.sum())
            last_trunc[dk] = trunc[dk]
            ret[dk] = 0
            ln[dk] = 0
            prev = tr["obs"][k]
    assert n_trunc > 0
    assert np.array_equal(env.get_reset_counts(), rc)
    assert np.array_equal(env.get_sbd(), sbd)
    assert np.array_equal(env.episode_truncated(), last_trunc)
    tot = env.episode_totals()
    assert tot["episodes"] == fin_n and tot["length_sum"] == fin_len
    assert abs(tot["return_sum"] - fin_ret) <= 1e-4 * max(1.0, abs(fin_ret))
    eb = env.episode_buffers()
    assert np.array_equal(eb["cur_length"], ln) and np.abs(eb["cur_return"] - ret).max() < 1e-3
    env.close()


@pytest.mark.parametrize("kind", KINDS)
def test_random_actions_with_a_limit_vs_oracle(G, kind):
    _teacher_forced(G, kind, 20, [64])
    _teacher_forced(G, kind, 40, [32, 32])   # lengths carry over the launch boundary


def _snapshot(env):
    eb = env.episode_buffers()
    return dict(state=env.get_state(), sbd=env.get_sbd(), rc=env.get_reset_counts(), trunc=env.episode_truncated(),
                ll=eb["last_length"], cl=eb["cur_length"], lr=eb["last_return"], cr=eb["cur_return"], tot=env.episode_totals())


def _same(a, b):
    for k in a:
        if k == "tot":   # (the return sums are float partial sums in a different order: fused per launch, single steps per step)
            assert (a[k]["episodes"], a[k]["length_sum"]) == (b[k]["episodes"], b[k]["length_sum"]), (a[k], b[k])
            assert abs(a[k]["return_sum"] - b[k]["return_sum"]) <= 1e-5 * max(1.0, abs(a[k]["return_sum"])), (a[k], b[k])
        else:
            assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("kind,n", [(k, 64) for k in KINDS] + [("quad3d", 65536), ("quad3d", 262144), ("quad3d", 1048576)])
def test_fused_equals_single_steps_under_a_limit(G, kind, n):
    import torch

    H, T = 7, 12
    nA = G._abi.ACTION_DIM[G._abi.KIND_BY_NAME[kind]]
    lo, hi = BOX[kind]
    g = torch.Generator(device="cuda").manual_seed(3)
    acts = [(lo + (hi - lo) * torch.rand((T, nA, n), generator=g, device="cuda")).contiguous() for _ in range(2)]
    for mode in ("random", "buffer"):
        envs = [G.BatchedQuadrotor(kind, n, seed=9, max_episode_steps=H) for _ in range(3)]
        outs = [[], [], []]
        for j in range(2):   # two launches: running lengths carry over
            a = acts[j] if mode == "buffer" else None
            for i, fused in enumerate((True, False)):
                tr = envs[i].rollout(T, mode=mode, actions=a, layout="soa", fused=fused, device_out=True,
                                     want=("obs", "rew", "done"))
                outs[i].append(tr)
            if mode == "buffer":   # T single steps through rmav_step (host arrays for the pinned one-wavefront path at 64 envs)
                steps = {"obs": [], "rew": [], "done": []}
                for k in range(T):
                    if n == 64:
                        o, r, d = envs[2].step(a[k].cpu().numpy(), layout="soa")
                        o, r, d = (torch.as_tensor(x, device="cuda") for x in (o, r, d.astype(np.uint8)))
                    else:
                        o, r, d = envs[2].step(a[k], layout="soa")
                    steps["obs"].append(o)
                    steps["rew"].append(r)
                    steps["done"].append(d)
                outs[2].append({k: torch.stack(v) for k, v in steps.items()})
        torch.cuda.synchronize()
        for i in (1, 2) if mode == "buffer" else (1,):
            for j in range(2):
                for key in ("obs", "rew", "done"):
                    assert torch.equal(outs[0][j][key].cpu(), outs[i][j][key].cpu()), (mode, i, j, key)
            _same(_snapshot(envs[0]), _snapshot(envs[i]))
        assert int(outs[0][0]["done"].sum()) >= n   # the limit fired
        for e in envs:
            e.close()


def _collect(G, env, actor, T, shared=False):
    import torch
    from gym_reinmav_amd import ppo as P

    torch.manual_seed(0)
    pol = P.MlpPolicy(env.nS, env.nA, init_logstd=0.5, value_network="shared" if shared else "copy").cuda()
    col = P.FusedPolicyCollector(env, pol, T, f16_mfma=(actor == "f16"))
    col.collect()
    return col


ACTORS = (("f32m", False), ("f16", False), ("f16", True))


def test_a_limit_that_never_fires_changes_nothing(G):
    import torch

    H, T, kind = 1 << 30, 16, "quad3d"
    pairs = [(G.BatchedQuadrotor(kind, N, seed=4), G.BatchedQuadrotor(kind, N, seed=4, max_episode_steps=H)) for _ in range(3)]
    acts = torch.rand((T, 4, N), device="cuda") * 10.0
    for mode, (a, b) in zip(("random", "controller", "buffer"), pairs):
        for fused in (True, False):
            ra = a.rollout(T, mode=mode, actions=acts if mode == "buffer" else None, fused=fused, device_out=True, want=("obs", "rew", "done"))
            rb = b.rollout(T, mode=mode, actions=acts if mode == "buffer" else None, fused=fused, device_out=True, want=("obs", "rew", "done"))
            for key in ra:
                assert torch.equal(ra[key], rb[key]), (mode, fused, key)
        sa, sb = _snapshot(a), _snapshot(b)
        sb.pop("trunc")
        sa.pop("trunc")
        _same(sa, sb)
    for actor, shared in ACTORS:
        a, b = G.BatchedQuadrotor(kind, N, seed=4), G.BatchedQuadrotor(kind, N, seed=4, max_episode_steps=H)
        ca, cb = _collect(G, a, actor, T, shared), _collect(G, b, actor, T, shared)
        for key in ("obs", "act", "rew", "done", "logp", "val"):
            assert torch.equal(getattr(ca, key), getattr(cb, key)), (actor, shared, key)
        a.close()
        b.close()
    for a, b in pairs:
        a.close()
        b.close()


@pytest.mark.parametrize("actor,shared", ACTORS)
def test_policy_rollouts_under_a_limit(G, actor, shared):
    import torch

    H, T, kind, seed = 16, 64, "quad3d", 21
    env = G.BatchedQuadrotor(kind, N, seed=seed, max_episode_steps=H)
    rc = env.get_reset_counts().copy()
    col = _collect(G, env, actor, T, shared)
    torch.cuda.synchronize()
    done = col.done.cpu().numpy().astype(bool)
    rew = col.rew.cpu().numpy()
    obs = col.obs[1:].cpu().numpy()   # [T][nS][N]
    lens, ln = _lengths(done)
    trunc = done & (rew < 0)
    assert np.array_equal(done | (lens < H), np.ones_like(done))   # done wherever the limit is reached
    assert (lens[trunc] == H).all() and trunc.sum() > 0           # and truncated only there
    ids = np.arange(N)
    for k in range(T):
        if done[k].any():
            assert np.array_equal(obs[k][:, done[k]].T, O.reset_states(kind, seed, ids[done[k]], rc[done[k]]))
        rc = rc + done[k].astype(np.uint32)
    assert torch.isfinite(col.val).all() and torch.isfinite(col.logp).all()
    tot = env.episode_totals()
    assert tot["episodes"] == int(done.sum()) and tot["length_sum"] == int(lens[done].sum())
    assert np.array_equal(env.episode_buffers()["cur_length"], ln)
    env.close()


def test_unsupported_policy_precisions_are_refused(G):
    import torch

    env = G.BatchedQuadrotor("quad3d", N, max_episode_steps=16)
    A = G._abi
    L = A.lib()
    w = torch.zeros(L.rmav_policy_weight_count(A.QUAD3D), device="cuda")
    lp, v = torch.empty((8, N), device="cuda"), torch.empty((9, N), device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for prec in (A.POLICY_FP32, A.POLICY_BF16_MFMA):
        assert L.rmav_rollout_policy(env._h, 8, p(w), None, None, None, None, p(lp), p(v), prec) == A.ERR_INVALID
        assert b"RMAV_POLICY_F16_MFMA" in L.rmav_last_error()
    from gym_reinmav_amd import ppo as P

    pol = P.MlpPolicy(env.nS, env.nA).cuda()
    for kw in (dict(f32_mfma=False), dict(bf16_mfma=True)):
        with pytest.raises(ValueError):
            P.FusedPolicyCollector(env, pol, 8, **kw)
    env.close()


def test_edge_semantics(G):
    A = G._abi
    kind, H = "quad3d", 10
    # no auto-reset: done every H steps, the state is not reset, steps_beyond_done untouched
    lim = G.BatchedQuadrotor(kind, N, seed=8, auto_reset=False, max_episode_steps=H, params=_wide(G, kind))
    twin = G.BatchedQuadrotor(kind, N, seed=8, auto_reset=False, params=_wide(G, kind))
    a = lim.rollout(3 * H, mode="controller", layout="aos")
    b = twin.rollout(3 * H, mode="controller", layout="aos")
    keep = ~b["done"].any(axis=0)
    assert keep.mean() >= 0.25
    assert np.array_equal(a["obs"][:, keep], b["obs"][:, keep])
    assert np.array_equal(a["rew"][:, keep], b["rew"][:, keep])
    expect = np.zeros(3 * H, bool)
    expect[H - 1::H] = True
    assert (a["done"][:, keep].astype(bool) == expect[:, None]).all()
    assert np.array_equal(lim.get_sbd(), twin.get_sbd()) and np.array_equal(lim.get_reset_counts(), twin.get_reset_counts())
    lim.close()
    twin.close()

    # a step that terminates at L == H is a termination: flag 0, the terminal reward, steps_beyond_done set
    env = G.BatchedQuadrotor(kind, 64, seed=1, max_episode_steps=1)
    s = env.get_state()
    s[0] = 0.0
    s[0, 0], s[0, 3], s[0, 7] = 2.99, 1.0, 9.0     # x just inside |pos| < 3, vx = 9: leaves the box in this step
    env.set_state(s)
    act = np.tile(np.array([9.8, 0, 0, 0], np.float32), (64, 1))
    o, r, d = env.step(act)
    assert d.all()
    tf = env.episode_truncated()
    assert tf[0] == 0 and r[0] == 1.0 and env.get_sbd()[0] == 0
    assert (tf[1:] == (r[1:] < 0)).all() and (env.get_sbd()[1:][tf[1:] == 1] == -1).all()
    env.close()

    # a handle without episode tracking counts from rmav_set_time_limit and from reset()
    def untermin(*trs):   # envs without a dynamic termination (a done with the terminal reward 1 / 0) in these rollouts
        return ~np.concatenate([(t["done"].astype(bool) & (t["rew"] >= 0)) for t in trs]).any(axis=0)

    def pattern(done, where):
        e = np.zeros(done.shape[0], bool)
        e[where] = True
        return (done.astype(bool) == e[:, None]).all(axis=0)

    env = G.BatchedQuadrotor(kind, N, seed=2, track_episodes=False, params=_wide(G, kind))
    env.rollout(7, mode="controller")
    env.max_episode_steps = 5
    tr = env.rollout(12, mode="controller")
    keep = untermin(tr)
    assert keep.mean() >= 0.25 and pattern(tr["done"], [4, 9])[keep].all()
    env.reset()
    t1 = env.rollout(3, mode="controller")
    t2 = env.rollout(4, mode="controller")
    keep = untermin(t1, t2)
    assert keep.mean() >= 0.25 and pattern(t1["done"], [])[keep].all() and pattern(t2["done"], [1])[keep].all()
    env.close()

    # seed() and set_step_count() keep running lengths
    env = G.BatchedQuadrotor(kind, N, seed=3, max_episode_steps=H, params=_wide(G, kind))
    t1 = env.rollout(4, mode="controller")
    env.seed(123)
    env.step_count = 1000
    t2 = env.rollout(2, mode="controller")
    env.step_count = 77
    t3 = env.rollout(6, mode="controller")
    keep = untermin(t1, t2, t3)
    assert keep.mean() >= 0.25 and pattern(np.concatenate([t1["done"], t2["done"], t3["done"]]), [9])[keep].all()
    assert (env.episode_buffers()["last_length"][keep] == H).all()

    # set / get round trip, refusals
    env.max_episode_steps = None
    assert env.max_episode_steps is None
    env.max_episode_steps = 1 << 30
    assert env.max_episode_steps == 1 << 30
    for bad in (-1, (1 << 30) + 1):
        assert A.lib().rmav_set_time_limit(env._h, bad) == A.ERR_INVALID
    v = C.c_int32()
    assert A.lib().rmav_get_time_limit(env._h, C.byref(v)) == 0 and v.value == 1 << 30
    env.close()
    rm = G.BatchedQuadrotor("reinmav", 64)
    assert A.lib().rmav_set_time_limit(rm._h, 10) == A.ERR_INVALID
    assert A.lib().rmav_set_time_limit(rm._h, 0) == 0
    rm.close()


@pytest.mark.parametrize("dict_infos,n", [(True, 256), (False, 8192)])
def test_vec_env_infos_carry_the_truncated_flag(G, dict_infos, n):
    H = 5
    for limit in (H, None):
        venv = G.QuadrotorVecEnv("quadrotor3d-v0", n, seed=6, dict_infos=dict_infos, max_episode_steps=limit)
        venv.reset()
        seen_trunc = 0
        for k in range(2 * H):
            act = venv.env.control(layout="aos", device_out=True)
            _, rew, done, infos = venv.step(act)
            d = done.cpu().numpy()
            r = rew.cpu().numpy()
            for i in range(n):
                info = infos[i]
                if not d[i]:
                    assert "TimeLimit.truncated" not in info and "episode" not in info
                    continue
                assert "episode" in info
                if limit is None:
                    assert "TimeLimit.truncated" not in info
                    continue
                assert info["TimeLimit.truncated"] == bool(r[i] < 0)
                if info["TimeLimit.truncated"]:
                    seen_trunc += 1
                    assert info["episode"]["l"] == H
        if limit:
            assert seen_trunc >= n // 4
        venv.close()


def test_gym_shaped_env_with_max_episode_steps(G):
    """The reference's smoke loop (test/test_quadrotor3d.py:13-22, without render) on make(..., max_episode_steps=50)."""
    H = 50
    seed = None
    for s in range(20):   # a start state the controller holds for 50 steps without a limit
        env = G.make("quadrotor3d-v0", seed=s)
        ok = True
        for _ in range(H):
            _, _, done, _ = env.step(env.control())
            if done:
                ok = False
                break
        env.close()
        if ok:
            seed = s
            break
    assert seed is not None
    env = G.make("quadrotor3d-v0", seed=seed, max_episode_steps=H)
    first = None
    for i in range(1, 2 * H + 1):
        _, reward, done, info = env.step(env.control())
        if done:
            first = first or i
            if i == H:
                assert info == {"TimeLimit.truncated": True} and reward < 0
            env.reset()
    assert first == H
    env.close()


def test_fused_policy_collector_reports_truncated_episodes(G):
    env = G.BatchedQuadrotor("quad3d", N, seed=12, max_episode_steps=8)
    col = _collect(G, env, "f32m", 32)
    done = col.done.cpu().numpy().astype(bool)
    rew = col.rew.cpu().numpy()
    tot = env.episode_totals()
    assert tot["episodes"] == int(done.sum()) and int((done & (rew < 0)).sum()) > 0
    env.close()

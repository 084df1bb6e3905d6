"""Frame skip (rmav_set_frame_skip) on the GPU.  The binding criterion is composition: one agent step of a handle with frame skip k equals,
bit for bit, k single steps of a plain handle under the same action, cut at each env's first termination, with R = r_0 (+ r_j in
order, fp32).  On top of it: fused = unfused = composition, the fp64 oracle at k x the per-step bar, the time limit, parameter ranges,
the policy rollouts and the Python classes.

Fresh U[-1, 1) states do not terminate within 8 held sub-steps, so the start states are crafted (`crafted`): lane e is planned to
terminate in sub-step j = e % (k + 1) (j = k: not at all), its deciding body on the x axis at sign * (pos_limit - (j + 0.5) v dt) with
x-velocity sign * v, v = 1, everything else 0.05 U[-1, 1), fp32.  Worst observed margin of case 3 is in profiles/r16/frame_skip.md."""
import numpy as np
import pytest

import oracle as O
from util import KINDS, NA, NS, TERM, TOL

pytestmark = pytest.mark.gpu

SEED, BASE, DT, V = 11, 300, 0.01, 1.0
SIZES = (1, 63, 65, 130)
SKIPS = (2, 3, 8)
TETHER = {"quad2d_sl": 0.5, "quad3d_sl": 1.5}
QUAD_X = {"quad2d": (0, 3), "quad2d_sl": (0, 3), "quad3d": (0, 7), "quad3d_sl": (0, 7)}       # (x, x-velocity) of the quadrotor
LOAD_X = {"quad2d_sl": (5, 7), "quad3d_sl": (10, 13)}                                          # ... of the load
UP = {"quad2d_sl": 1, "quad3d_sl": 2}                                                          # the quadrotor's "up" position component


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available()
    import gym_reinmav_amd as g

    return g


def crafted(kind, n, k, seed=3, first=0):
    """(states f32 [n, nS], actions f32 [n, nA], planned sub-step int [n]) of the recipe; `first`: sub-steps that pass before the planned
    one counts (the time-limit case plans a termination inside a later agent step)."""
    rng = np.random.RandomState(seed)
    s = 0.05 * rng.uniform(-1, 1, (n, NS[kind]))
    a = (0.5 * rng.uniform(-1, 1, (n, NA[kind]))).astype(np.float32)
    e = np.arange(n)
    j = e % (k + 1)
    sign = np.where((e // (k + 1)) % 2 == 0, 1.0, -1.0)
    ps, _, pos_limit, _ = TERM[kind]
    x = sign * (pos_limit - (first + j + 0.5) * V * DT)
    if kind in ("quad3d", "quad3d_sl"):
        s[:, 3] = 1.0
    s[:, ps] = 0.0
    s[:, ps.start] = x
    ix, iv = QUAD_X[kind]
    s[:, ix], s[:, iv] = x, sign * V
    if kind in LOAD_X:
        lx, lv = LOAD_X[kind]
        s[:, lx], s[:, lv] = x, sign * V
        s[:, 0:(2 if kind == "quad2d_sl" else 3)] = 0.0
        s[:, 0] = x
        s[:, UP[kind]] = 0.9 * TETHER[kind]
    return s.astype(np.float32), a, j


def f32_sum(R, r, first):
    return r.copy() if first else (R.astype(np.float32) + r.astype(np.float32)).astype(np.float32)


def compose(B, state, sbd, act, k):
    """k single steps of the plain handle B (no auto-reset) from (state, sbd) under `act`, per env cut at its first termination.
    -> obs, R (fp32, the contract's order), term, sbd after, sub-step index of the termination (k: none)."""
    n = len(state)
    B.set_state(state)
    B.set_sbd(sbd)
    obs, R = np.zeros_like(state), np.zeros(n, np.float32)
    term, at = np.zeros(n, bool), np.full(n, k)
    sbd_out = np.asarray(sbd, np.int32).copy()
    for j in range(k):
        o, r, d = B.step(act)
        live = ~term
        obs[live] = o[live]
        R[live] = f32_sum(R[live], r[live], j == 0)
        sbd_out[live] = B.get_sbd()[live]
        at[live & d] = j
        term |= d
    return obs, R, term, sbd_out, at


def same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert a.tobytes() == b.tobytes(), (what, np.argwhere(a != b)[:5])


def handles(G, kind, n, k, auto_reset=True, **kw):
    A_ = G.BatchedQuadrotor(kind, n, seed=SEED, env_id_base=BASE, auto_reset=auto_reset, frame_skip=k, **kw)
    B_ = G.BatchedQuadrotor(kind, n, seed=SEED, env_id_base=BASE, auto_reset=False, track_episodes=False)
    return A_, B_


# ---- 1. composition, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("k", SKIPS)
def test_one_agent_step_is_k_composed_steps(G, kind, n, k):
    import torch

    s0, act, plan = crafted(kind, n, k)
    sbd0 = np.where(np.arange(n) % 3 == 0, 0, -1).astype(np.int32)   # both branches of the terminal reward
    _, Bh = handles(G, kind, n, k)
    obs, R, term, sbd1, at = compose(Bh, s0, sbd0, act, k)
    same(at, plan, "every lane terminates at its planned sub-step")
    assert set(at) == set(np.arange(n) % (k + 1))
    for auto_reset in (False, True):
        for layout in ("aos", "soa"):
            for dev in (False, True):
                Ah = G.BatchedQuadrotor(kind, n, seed=SEED, env_id_base=BASE, auto_reset=auto_reset, frame_skip=k)
                assert Ah.frame_skip == k and Ah.step_count == 0
                Ah.set_state(s0)
                Ah.set_sbd(sbd0)
                rc0 = Ah.get_reset_counts()
                a_in = act if layout == "aos" else np.ascontiguousarray(act.T)
                if dev:
                    a_in = torch.from_numpy(a_in).cuda()
                if auto_reset:
                    o, r, d, fin, tr = Ah.step_final(a_in, layout=layout)
                else:
                    o, r, d = Ah.step(a_in, layout=layout)
                host = lambda x: x.cpu().numpy() if dev else np.asarray(x)   # noqa: E731
                o, r, d = host(o), host(r), host(d).astype(bool)
                o = o if layout == "aos" else o.T
                same(r, R, "reward")
                same(d, term, "done")
                same(Ah.get_sbd(), sbd1, "sbd")
                assert Ah.step_count == 1
                if auto_reset:
                    fin = host(fin) if layout == "aos" else host(fin).T
                    same(o[~term], obs[~term], "obs of the envs that go on")
                    same(fin[term], obs[term], "rmav_step_final: the pre-reset state")
                    assert not host(tr).any()
                    if term.any():
                        ids = BASE + np.nonzero(term)[0]
                        same(o[term], O.reset_states(kind, SEED, ids, rc0[term]), "the reset state")
                    same(Ah.get_reset_counts(), rc0 + term.astype(np.uint32), "reset counts")
                    same(Ah.get_state(), o, "state in place")
                else:
                    same(o, obs, "obs")
                Ah.close()
    Bh.close()


# ---- 2. fused = unfused = composition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", ["buffer", "random", "controller"])
@pytest.mark.parametrize("n,k,T", [(1, 2, 3), (63, 3, 9), (65, 8, 3), (130, 2, 9), (130, 8, 9)])
def test_fused_unfused_and_composition_agree(G, kind, mode, n, k, T):
    s0, _, _ = crafted(kind, n, k)
    rng = np.random.RandomState(7)
    acts = (0.5 * rng.uniform(-1, 1, (T, n, NA[kind]))).astype(np.float32)
    want = ("actions", "obs", "rew", "done")
    outs = []
    for fused in (True, False):
        Ah = G.BatchedQuadrotor(kind, n, seed=SEED, env_id_base=BASE, frame_skip=k)
        Ah.set_state(s0)
        tr = Ah.rollout(T, mode=mode, actions=acts if mode == "buffer" else None, layout="aos", fused=fused, want=want)
        tr = {key: np.asarray(v) for key, v in tr.items()}
        tr.update(state=Ah.get_state(), sbd=Ah.get_sbd(), rc=Ah.get_reset_counts(), t=np.array([Ah.step_count]),
                  tot=np.array(list(Ah.episode_totals().values()), np.float64), **Ah.episode_buffers())
        outs.append(tr)
        Ah.close()
    for key in outs[0]:
        if key != "tot":
            same(outs[0][key], outs[1][key], "fused vs unfused: " + key)
    # (episodes and length_sum exactly; return_sum is a double sum of per-wavefront fp32 partial sums whose grouping differs between one
    # launch and T: at most N T = 1170 terms, each partial sum within 1170 x 2^-24 = 7e-5 relative)
    a, b = outs[0]["tot"], outs[1]["tot"]
    assert a[0] == b[0] and a[2] == b[2] and abs(a[1] - b[1]) <= 1e-4 * max(1.0, abs(a[1])), (a, b)
    tr = outs[0]
    assert tr["t"][0] == T
    p = G.BatchedQuadrotor(kind, 1, auto_reset=False).params
    if mode == "random":   # the stream of the AGENT-step counter
        for t in range(T):
            same(tr["actions"][t], O.random_actions(kind, SEED, BASE + np.arange(n), t, p.act_lo, p.act_hi).astype(np.float32), "random actions")
    # teacher-forced composition on a plain handle, re-seeded from the stored obs at every agent step
    Bh = G.BatchedQuadrotor(kind, n, seed=SEED, env_id_base=BASE, auto_reset=False, track_episodes=False)
    prev, sbd = s0, np.full(n, -1, np.int32)
    ret, length = np.zeros(n, np.float32), np.zeros(n, np.int32)
    last_ret, last_len, episodes, len_sum, ret_sum = np.zeros(n, np.float32), np.zeros(n, np.int32), 0, 0, 0.0
    for t in range(T):
        if mode == "controller":
            Bh.set_state(prev)
            same(tr["actions"][t], Bh.control(), "control() once per agent step")
        obs, R, term, sbd, _ = compose(Bh, prev, sbd, tr["actions"][t], k)
        same(tr["rew"][t], R, f"reward of agent step {t}")
        same(tr["done"][t].astype(bool), term, f"done of agent step {t}")
        same(tr["obs"][t][~term], obs[~term], f"obs of agent step {t}")
        ret = (ret + R).astype(np.float32)
        length += 1
        last_ret[term], last_len[term] = ret[term], length[term]
        episodes, len_sum, ret_sum = episodes + int(term.sum()), len_sum + int(length[term].sum()), ret_sum + float(ret[term].astype(np.float64).sum())
        ret[term], length[term] = 0.0, 0
        prev = tr["obs"][t]
    assert tr["done"].any() or n == 1
    same(tr["sbd"], sbd, "sbd")
    same(tr["last_length"], last_len, "last_length counts agent steps")
    same(tr["cur_length"], length, "cur_length")
    same(tr["last_return"], last_ret, "last_return is a sum of R")
    same(tr["cur_return"], ret, "cur_return")
    assert tr["tot"][0] == episodes and tr["tot"][2] == len_sum and abs(tr["tot"][1] - ret_sum) <= 1e-4 * max(1.0, abs(ret_sum))
    Bh.close()


# ---- 3. against the fp64 oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", SKIPS)
def test_agent_step_matches_the_fp64_oracle(G, kind, k):
    n = 130
    s0, act, plan = crafted(kind, n, k)
    Ah = G.BatchedQuadrotor(kind, n, seed=SEED, env_id_base=BASE, auto_reset=False, frame_skip=k)
    Ah.set_state(s0)
    o, r, d = Ah.step(act)
    s, sbd = s0.astype(np.float64), np.full(n, -1)
    obs, R, term = s.copy(), np.zeros(n), np.zeros(n, bool)
    margin = np.inf
    ps, vs, pl, vl = TERM[kind]
    for j in range(k):
        live = ~term
        s2, rj, dj, sbd2 = O.batch_step(kind, s, act.astype(np.float64), sbd)
        margin = min(margin, float(np.abs(np.linalg.norm(s2[live][:, ps], axis=1) - pl).min()))
        obs[live], R[live] = s2[live], np.where(j == 0, rj[live], R[live] + rj[live])
        sbd = np.where(live, sbd2, sbd)
        term |= live & dj.astype(bool)
        s = np.where(live[:, None], s2, s)
    assert margin >= 4e-3, margin
    same(d, term, "done")
    same(np.array([plan[i] < k for i in range(n)]), term, "the oracle terminates every lane at its planned sub-step")
    bar = k * TOL
    eo = np.abs(o - obs) / np.maximum(1.0, np.abs(obs))
    er = np.abs(r - R) / np.maximum(1.0, np.abs(R))
    print(f"frame-skip oracle margin {kind} k={k}: obs {eo.max():.3g} rew {er.max():.3g} of {bar:.3g}; deciding norm >= {margin:.3g} from the limit")
    assert eo.max() <= bar and er.max() <= bar, (eo.max(), er.max(), bar)
    Ah.close()


# ---- 4. time limit -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_time_limit_counts_agent_steps(G, kind):
    n, k, H = 65, 4, 3
    # lanes planned to terminate inside the THIRD agent step (sub-steps 8 .. 11), lane % 5 == 4 not at all
    s0, act, plan = crafted(kind, n, k, first=2 * k)
    Ah = G.BatchedQuadrotor(kind, n, seed=SEED, env_id_base=BASE, frame_skip=k, max_episode_steps=H)
    Ah.set_state(s0)
    for t in range(H):
        o, r, d, fin, tr = Ah.step_final(act)
        if t < H - 1:
            assert not d.any() and not tr.any(), t
    term = plan < k
    assert term.any() and (~term).any()
    assert d.all()
    same(tr, ~term, "truncated exactly where the dynamics did not terminate: termination wins")
    same(Ah.episode_truncated().astype(bool), ~term, "last_trunc")
    same(Ah.episode_buffers()["last_length"], np.full(n, H, np.int32), "last_length = 3 agent steps")
    assert Ah.step_count == H
    Ah.close()


# ---- 5. range ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["quad3d", "quad2d_sl"])
def test_range_with_frame_skip(G, kind):
    n, k, T = 130, 3, 9
    s0, _, _ = crafted(kind, n, k)
    v = 1.125
    outs = []
    for ranged in (True, False):
        Ah = G.BatchedQuadrotor(kind, n, seed=SEED, env_id_base=BASE, frame_skip=k)
        if ranged:
            Ah.set_env_param_range("mass", v, v)
        else:
            Ah.set_env_param("mass", np.full(n, v, np.float32))
        Ah.set_state(s0)
        tr = Ah.rollout(T, mode="random", layout="aos", want=("actions", "obs", "rew", "done"))
        outs.append({**{key: np.asarray(x) for key, x in tr.items()}, "state": Ah.get_state(), "mass": Ah.get_env_param("mass")})
        Ah.close()
    assert outs[0]["done"].any()
    for key in outs[0]:
        same(outs[0][key], outs[1][key], "lo == hi vs N copies: " + key)
    # lo < hi: the constant changes exactly at a reset, and holds for all sub-steps (the composition with the OLD mass reproduces the step)
    Ah = G.BatchedQuadrotor(kind, n, seed=SEED, env_id_base=BASE, frame_skip=k, randomize={"mass": (0.8, 1.25)})
    Bh = G.BatchedQuadrotor(kind, n, seed=SEED, env_id_base=BASE, auto_reset=False, track_episodes=False)
    Ah.set_state(s0)
    rng = np.random.RandomState(9)
    sbd = Ah.get_sbd()
    changed = 0
    for t in range(3):
        act = (0.5 * rng.uniform(-1, 1, (n, NA[kind]))).astype(np.float32)
        m0, prev = Ah.get_env_param("mass"), Ah.get_state()
        o, r, d = Ah.step(act)
        m1 = Ah.get_env_param("mass")
        same(m1[~d], m0[~d], "no reset: the constant stays")
        assert (m1[d] != m0[d]).all()
        changed += int(d.sum())
        Bh.set_env_param("mass", m0)
        obs, R, term, sbd, _ = compose(Bh, prev, sbd, act, k)
        same(d, term, "done")
        same(r, R, "the old episode's constant holds for all of its sub-steps")
        same(o[~term], obs[~term], "obs")
    assert changed > 0
    Ah.close()
    Bh.close()


# ---- 6. policy rollouts ------------------------------------------------------------------------------------------------------------
def _policy(env, actor):
    import torch
    from gym_reinmav_amd.ppo import MlpPolicy

    torch.manual_seed(2)
    pol = MlpPolicy(env.nS, env.nA, init_logstd=-0.5, value_network="shared" if actor == "f16_shared" else "copy").cuda()
    with torch.no_grad():
        pol.pi[2].weight.mul_(30.0)
        pol.vf[-1].bias.uniform_(-0.5, 0.5)
    return pol


@pytest.mark.parametrize("actor", ["fp32_mfma", "f16", "f16_shared"])
@pytest.mark.parametrize("limited", [False, True])
@pytest.mark.parametrize("kind,n,k", [("quad3d", 33, 2), ("quad3d", 130, 3), ("quad2d_sl", 65, 8), ("quad3d_sl", 63, 3), ("quad2d", 1, 2)])
def test_policy_rollouts(G, actor, limited, kind, n, k):
    import torch
    from gym_reinmav_amd.ppo import FusedPolicyCollector

    T, H, CLIP = 9, 4, (-0.5, 0.5)
    s0, _, _ = crafted(kind, n, k)
    kw = dict(f16_mfma=(actor == "f16"), clip_actions=CLIP)
    Ah = G.BatchedQuadrotor(kind, n, seed=SEED, env_id_base=BASE, frame_skip=k, max_episode_steps=H if limited else None)
    Ah.set_state(s0)
    pol = _policy(Ah, actor)
    col = FusedPolicyCollector(Ah, pol, T, bootstrap_truncated=limited, **kw)
    col.collect()
    torch.cuda.synchronize()
    act, obs, rew, done = (x.cpu().numpy() for x in (col.act, col.obs, col.rew, col.done))
    logp, val = col.logp.cpu().numpy(), col.val.cpu().numpy()
    assert Ah.step_count == T and np.isfinite(act).all()
    # the composition: k plain steps under clip(actions[t]) from obs[t - 1]
    Bh = G.BatchedQuadrotor(kind, n, seed=SEED, env_id_base=BASE, auto_reset=False, track_episodes=False)
    # ... and the actor: a k = 1 handle's one-step launch from the same state, seed, env ids and step counter
    Ch = G.BatchedQuadrotor(kind, n, seed=SEED, env_id_base=BASE)
    col1 = FusedPolicyCollector(Ch, pol, 1, **kw)
    sbd = np.full(n, -1, np.int32)
    length = np.zeros(n, np.int32)
    trunc_seen = 0
    for t in range(T):
        prev = np.ascontiguousarray(obs[t].T)   # [nS, N] -> [N, nS]
        Ch.set_state(prev)
        Ch.step_count = t
        col1.collect()
        torch.cuda.synchronize()
        same(col1.logp[0].cpu().numpy(), logp[t], f"logp of agent step {t}")
        same(col1.val[0].cpu().numpy(), val[t], f"value of agent step {t}")
        same(col1.act[0].cpu().numpy(), act[t], f"stored action of agent step {t}")
        o, R, term, sbd, _ = compose(Bh, prev, sbd, np.ascontiguousarray(np.clip(act[t].T, *CLIP).astype(np.float32)), k)
        length += 1
        trunc = ~term & (length >= H) if limited else np.zeros(n, bool)
        same(rew[t], R, f"reward of agent step {t}")
        same(done[t].astype(bool), term | trunc, f"done of agent step {t}")
        fin = term | trunc
        same(obs[t + 1].T[~fin], o[~fin], f"obs of agent step {t}")
        if limited:
            boot, tr = col.boot.cpu().numpy()[t], col.trunc.cpu().numpy()[t].astype(bool)
            same(tr, trunc, "truncated flags")
            assert ((boot != 0) == trunc).all(), "boot_out is non-zero exactly on truncated agent steps"
            trunc_seen += int(trunc.sum())
        length[fin] = 0
    assert done.any()
    assert not limited or trunc_seen > 0
    for h in (Ah, Bh, Ch):
        h.close()


def test_policy_rollouts_refuse_the_actors_without_a_kernel(G):
    from gym_reinmav_amd.ppo import FusedPolicyCollector

    env = G.BatchedQuadrotor("quad3d", 65, frame_skip=2)
    with pytest.raises(ValueError):
        FusedPolicyCollector(env, _policy(env, "fp32"), 4, f32_mfma=False)
    with pytest.raises(ValueError):
        FusedPolicyCollector(env, _policy(env, "bf16"), 4, bf16_mfma=True)
    env.close()


# ---- 7. the classes ----------------------------------------------------------------------------------------------------------------
def test_gym_class_follows_two_plain_steps(G):
    from gym_reinmav_amd.registration import make

    a, b = make("quadrotor3d-v0", seed=4, frame_skip=2), make("quadrotor3d-v0", seed=4)
    assert a.frame_skip == 2 and b.frame_skip == 1
    np.testing.assert_array_equal(a.reset(), b.reset())
    for _ in range(3):
        u = a.control()
        np.testing.assert_array_equal(u, b.control())
        o, r, d, _ = a.step(u)
        _, r0, d0, _ = b.step(u)
        o1, r1, d1, _ = b.step(u)
        assert not d0 and not d1 and not d
        np.testing.assert_array_equal(o, o1)
        assert np.float32(r) == np.float32(np.float32(r0) + np.float32(r1))
    a.close()
    b.close()


def test_vec_env_reports_truncation_after_four_calls(G):
    from gym_reinmav_amd.vec_env import QuadrotorVecEnv

    env = QuadrotorVecEnv("quadrotor3d-v0", 65, seed=3, frame_skip=3, max_episode_steps=4, numpy_io=True)
    assert env.env.frame_skip == 3
    env.reset()
    act = np.full((65, 4), 0.1, np.float32)
    for t in range(4):
        _, _, done, infos = env.step(act)
        if t < 3:
            assert not np.asarray(done).any()
    assert np.asarray(done).all()
    assert all(i.get("TimeLimit.truncated") is True and i["episode"]["l"] == 4 for i in infos)
    env.close()


def test_evaluate_policy_counts_agent_steps(G):
    from gym_reinmav_amd.evaluate import evaluate_policy

    env = G.BatchedQuadrotor("quad3d", 130, seed=5, frame_skip=4, max_episode_steps=6)
    ev = evaluate_policy(_policy(env, "fp32_mfma"), env)
    assert ev["episodes"] == 130 and ev["unfinished"] == 0
    assert 1 <= ev["mean_length"] <= 6 and int(ev["lengths"].max()) <= 6
    assert env.step_count == 6
    env.close()


@pytest.mark.parametrize("kind", KINDS)
def test_back_to_one_gives_the_bits_of_a_handle_that_never_had_one(G, kind):
    n, T = 130, 9
    outs = []
    for touched in (True, False):
        env = G.BatchedQuadrotor(kind, n, seed=SEED, env_id_base=BASE)
        if touched:
            env.frame_skip = 4
            env.frame_skip = 1
        env.set_state(crafted(kind, n, 2)[0])
        tr = env.rollout(T, mode="random", layout="aos", want=("actions", "obs", "rew", "done"))
        o, r, d = env.step(np.zeros((n, NA[kind]), np.float32))
        outs.append({**{key: np.asarray(x) for key, x in tr.items()}, "o": o, "r": r, "d": d, "state": env.get_state(), "sbd": env.get_sbd()})
        env.close()
    for key in outs[0]:
        same(outs[0][key], outs[1][key], key)


def test_the_library_refuses_what_the_contract_refuses(G):
    import ctypes as C

    from gym_reinmav_amd import _abi as A

    L = A.lib()
    env = G.BatchedQuadrotor("quad3d", 4)
    for bad in (0, -3, 1025):
        assert L.rmav_set_frame_skip(env._h, bad) == A.ERR_INVALID
    v = C.c_int32()
    assert L.rmav_get_frame_skip(env._h, C.byref(v)) == 0 and v.value == 1
    env.frame_skip = 1024
    assert env.frame_skip == 1024
    env.frame_skip = 2
    with pytest.raises(A.RmavError):
        env.step_control(np.zeros((4, 4), np.float32))
    env.close()
    h = C.c_void_p()
    p = A.default_params(A.KIND_BY_NAME["reinmav"]) if "reinmav" in A.KIND_BY_NAME else None
    if p is not None:
        A.check(L.rmav_create(C.byref(h), A.KIND_BY_NAME["reinmav"], 4, 0, 0, 0, 0, C.byref(p), None))
        assert L.rmav_set_frame_skip(h, 2) == A.ERR_INVALID and L.rmav_set_frame_skip(h, 1) == 0
        L.rmav_destroy(h)

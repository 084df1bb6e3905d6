"""Termination rules (rmav_set_termination) on the GPU.  The main oracle is the EMULATED TWIN: a handle without the feature, same seed and env
ids, stepped one step at a time under the same buffered commands; after every step the test evaluates tests/term_ref.rule on the state of
every env whose done byte is 0 and, where it fires, emulates the termination - the reward from the twin's steps_beyond_done (set_sbd applies
its update), the fresh state of the reference's reset stream at the env's reset count (set_state), the reset count raised by one
(set_reset_counts).  The twin's observations, rewards, done bytes, final state, reset counts and steps_beyond_done are the bits the spec'd
handle stores from ONE fused launch.  Around it: every route gives the same bits; the episode records follow the stored rewards and done
bytes; each rule alone; the all-infinite spec and NULL are a handle without a spec; composition with every other feature; the three in-kernel
actors by replay; sharding; set semantics; refusals.  Every comparison is bit for bit except return_sum of the episode totals between routes
(1e-4 relative)."""
import ctypes as C
import math

import numpy as np
import pytest

import start_ref as SR
import term_ref as R
import test_gpu_disturbance as TD
from test_gpu_actuator import INIT, TAUS, u8
from test_gpu_disturbance import host, same, same_run
from test_gpu_start_state import compose_kw
from util import KINDS, NA, NS

pytestmark = pytest.mark.gpu

SEED, BASE = 11, 300
SIZES = (1, 63, 65, 130)
STEPS = (3, 12)          # below and above the 8-step threshold of the spare reset state
WANT = ("actions", "obs", "rew", "done")
F32 = np.float32
INF = math.inf


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available()
    import gym_reinmav_amd as g

    return g


def term_of(G, spec):
    lo, hi, tilt = spec
    return G.Termination(pos_lo=lo, pos_hi=hi, max_tilt=tilt)


def make(G, kind, n, term="spec", base=BASE, **kw):
    """A handle with the tests' seed and env ids.  term: "spec" (tests/term_ref.spec), "identity" (the all-infinite spec), a (lo, hi, tilt)
    triple, or None = the plain twin.  No reset: the running episodes are those of rmav_create (reset index 0), as the twin's."""
    if kw.get("reward") is True:
        kw["reward"] = TD.tracking(G)
    tc = None if term is None else G.Termination() if term == "identity" else term_of(G, R.spec(kind) if term == "spec" else term)
    return G.BatchedQuadrotor(kind, n, seed=SEED, env_id_base=base, termination=tc, **kw)


def ids(n, base=BASE):
    return base + np.arange(n)


def fresh_states(kind, env_ids, episodes):
    return SR.start_states(kind, SEED, env_ids, episodes, *SR.identity(kind))


def emulate(twin, kind, spec, o, r, d, base=BASE):
    """Behind one step of the plain twin: where the rule fires on the state of an env whose done byte is 0, the termination the spec'd handle
    performs inside its kernel -> the rule-only mask; o, r, d are updated in place."""
    n = twin.num_envs
    s, sbd, rc = twin.get_state(), twin.get_sbd(), twin.get_reset_counts()
    fire = R.rule(kind, s, *spec) & ~d
    if fire.any():
        r[fire] = np.where(sbd[fire] < 0, F32(1.0), F32(0.0))            # the reference's literal: 1 at the first termination, 0 beyond
        sbd[fire] = np.where(sbd[fire] < 0, 0, sbd[fire] + 1)
        s[fire] = fresh_states(kind, ids(n, base)[fire], rc[fire])
        rc[fire] += 1
        twin.set_state(s), twin.set_sbd(sbd), twin.set_reset_counts(rc)
        o[fire] = s[fire]
        d |= fire
    return fire


def twin_walk(twin, kind, acts, spec, base=BASE):
    obs, rew, done, only, pre = [], [], [], [], []
    for t in range(acts.shape[0]):
        o, r, d = twin.step(acts[t])
        o, r, d = host(o).copy(), host(r).copy(), u8(d).astype(bool)
        pre.append(d.copy())
        only.append(emulate(twin, kind, spec, o, r, d, base))
        obs.append(o), rew.append(r), done.append(d.astype(np.uint8))
    return dict(obs=np.stack(obs), rew=np.stack(rew), done=np.stack(done), only=np.stack(only), ref=np.stack(pre), state=twin.get_state(),
                rc=twin.get_reset_counts(), sbd=twin.get_sbd())


def check_against_twin(env, tr, tw, what=""):
    for key in ("obs", "rew", "done"):
        same(host(tr[key]).astype(tw[key].dtype), tw[key], f"{what}{key}")
    same(env.get_state(), tw["state"], f"{what}final state")
    same(env.get_reset_counts(), tw["rc"], f"{what}reset counts")
    same(env.get_sbd(), tw["sbd"], f"{what}steps_beyond_done")


# ---- 1. the emulated twin ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("n", SIZES)
def test_the_emulated_twin(G, kind, n, T):
    acts = R.commands(kind, n, T)
    env, twin = make(G, kind, n), make(G, kind, n, term=None)
    same(env.get_state(), twin.get_state(), "both start from the same state")
    tr = env.rollout(T, mode="buffer", actions=acts, layout="aos", want=WANT)       # ONE fused launch
    tw = twin_walk(twin, kind, acts, R.spec(kind))
    check_against_twin(env, tr, tw)
    if T == 12:   # the conditions of this oracle, from the twin's own data
        only, ends = tw["only"].sum(0), tw["done"].sum(0)
        assert only.min() >= 1, ("every env has a rule-only termination", kind, n, only.min())
        assert (T - ends).min() >= 1, ("every env has a step that does not end", kind, n)
        assert ends.max() >= 2, "the spare reset state and the on-demand second draw are used"
        assert n < 63 or kind in ("quad3d", "quad3d_sl") or tw["ref"].any() or kind == "quad2d_sl", "the reference's own rule fires too"
    env.close(), twin.close()


# ---- 2. routes --------------------------------------------------------------------------------------------------------------------------------
def routes(G, kind, n, T, fresh, modes=("buffer", "random", "controller")):
    """Every route over the same trajectory from a fresh handle each -> {mode: the base run}; all others are compared with it."""
    import torch

    acts = R.commands(kind, n, T)
    bases = {}
    for mode in modes:
        a_in = acts if mode == "buffer" else None
        env = fresh()
        base = TD.final(env, env.rollout(T, mode=mode, actions=a_in, layout="aos", want=WANT))
        env = fresh()
        others = {"fused = 0": TD.final(env, env.rollout(T, mode=mode, actions=a_in, layout="aos", fused=False, want=WANT))}
        env = fresh()
        singles = [env.rollout(1, mode=mode, actions=None if a_in is None else a_in[t:t + 1], layout="aos", want=WANT) for t in range(T)]
        others["single steps"] = TD.final(env, {key: np.concatenate([host(x[key]) for x in singles]) for key in WANT})
        env = fresh()
        soa_in = None if a_in is None else torch.from_numpy(np.ascontiguousarray(a_in.transpose(0, 2, 1))).cuda()
        others["feature-major, device"] = TD.final(env, env.rollout(T, mode=mode, actions=soa_in, layout="soa", want=WANT, device_out=True))
        if mode != "buffer":
            env = fresh()
            others["pitched"] = TD.final(env, {key: v.contiguous() for key, v in env.rollout(T, mode=mode, layout="soa", want=WANT, device_out=True, pitched=True).items()})
            if n == 130:
                env = fresh()
                ch = env.rollout_chunked(T, mode=mode, chunk=64, want=WANT)
                others["chunk-major"] = TD.final(env, {key: env.unchunk(v) for key, v in ch.items()})
        else:   # rmav_step itself
            env = fresh()
            steps = [env.step(acts[t]) for t in range(T)]
            others["rmav_step"] = TD.final(env, dict(actions=acts, obs=np.stack([host(x[0]) for x in steps]), rew=np.stack([host(x[1]) for x in steps]),
                                                     done=np.stack([u8(x[2]) for x in steps])))
        for name, other in others.items():
            same_run(base, other, f"{mode} {name}")
        bases[mode] = base
    return bases


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,T", [(1, 12), (63, 3), (65, 12), (130, 12), (130, 3)])
def test_every_route_gives_the_same_bits(G, kind, n, T):
    kw = dict(max_episode_steps=5) if n == 65 else {}
    bases = routes(G, kind, n, T, lambda: make(G, kind, n, **kw))
    if T == 12:
        assert bases["buffer"]["done"].any() and (n == 1 or bases["random"]["done"].any()), "episodes end inside the launch"
    # rmav_control_step is control-then-step
    a, b = make(G, kind, n, **kw), make(G, kind, n, **kw)
    for t in range(3):
        u = a.control()
        o1, r1, d1 = a.step(u)
        u2, o2, r2, d2 = b.control_step()
        same(u, u2, "control_step: the command"), same(o1, o2, "control_step: obs"), same(r1, r2, "control_step: rew"), same(u8(d1), u8(d2), "control_step: done")
    same(a.get_state(), b.get_state(), "control_step: state")
    a.close(), b.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", (1, 65, 130))
def test_step_final_reports_the_pre_reset_state(G, kind, n):
    """final_obs_out is the state the dynamics left - outside the rule where the rule fired, what the plain twin holds there - trunc_out is 0
    there, and the step's other outputs are the twin's"""
    T = 12
    acts = R.commands(kind, n, T)
    spec = R.spec(kind)
    env, twin = make(G, kind, n), make(G, kind, n, term=None)
    seen = 0
    for t in range(T):
        o, r, d, fin, tr = env.step_final(acts[t])
        o2, r2, d2 = twin.step(acts[t])
        o2, r2, d2 = host(o2).copy(), host(r2).copy(), u8(d2).astype(bool)
        pre = twin.get_state()
        only = emulate(twin, kind, spec, o2, r2, d2)
        d = u8(d).astype(bool)
        same(d, d2, "done"), same(r, r2, "rew"), same(o, o2, "obs")
        same(host(fin)[only], pre[only], "final_obs: the pre-reset state of a rule termination")
        assert R.rule(kind, host(fin)[only], *spec).all(), "... on which the rule fires"
        assert not u8(tr)[d].any(), "no time limit: nothing is truncated"
        assert not host(fin)[~d].any(), "the rows of running envs are not written"
        seen += int(only.sum())
        same(env.get_state(), twin.get_state(), "state")
    assert seen > 0
    env.close(), twin.close()


# ---- 3. episode records -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,H", [(65, None), (130, 4)])
def test_episode_records_follow_the_stored_rewards_and_done_bytes(G, kind, n, H):
    T = 12
    env = make(G, kind, n, max_episode_steps=H)
    tr = env.rollout(T, mode="buffer", actions=R.commands(kind, n, T), layout="aos", want=WANT)
    rew, done = host(tr["rew"]), u8(tr["done"]).astype(bool)
    cur, length = np.zeros(n, F32), np.zeros(n, np.int32)
    last_r, last_l = np.zeros(n, F32), np.zeros(n, np.int32)
    episodes, ret_sum, len_sum = 0, 0.0, 0
    for t in range(T):                                        # the in-order fp32 accumulation
        cur = (cur + rew[t]).astype(F32)
        length += 1
        d = done[t]
        last_r[d], last_l[d] = cur[d], length[d]
        episodes, ret_sum, len_sum = episodes + int(d.sum()), ret_sum + float(cur[d].astype(np.float64).sum()), len_sum + int(length[d].sum())
        cur[d], length[d] = 0, 0
    buf = env.episode_buffers()
    same(buf["last_return"], last_r, "last_return"), same(buf["last_length"], last_l, "last_length")
    same(buf["cur_return"], cur, "cur_return"), same(buf["cur_length"], length, "cur_length")
    tot = env.episode_totals()
    assert tot["episodes"] == episodes and tot["length_sum"] == len_sum and abs(tot["return_sum"] - ret_sum) <= 1e-4 * max(1.0, abs(ret_sum)), (tot, ret_sum)
    assert episodes >= n
    lt = u8(env.episode_truncated()).astype(bool)
    if H is None:
        assert not lt.any()
    else:   # the flag of each env's last finished episode: truncated iff it ran H steps without a termination - and some were, some were not
        assert (last_l[lt] == H).all() and lt.any() and (~lt & (last_l > 0)).any()
    env.close()


# ---- 4. each rule alone -----------------------------------------------------------------------------------------------------------------------
def alone(kind, which):
    d = R.DIM[kind]
    none = (-INF,) * d
    if which == "floor":
        return none[:-1] + (-0.5,), (INF,) * d, None
    if which == "walls":
        return (-0.6,) * (d - 1) + (-INF,), (0.6,) * (d - 1) + (INF,), None
    return None, None, (0.4 if d == 2 else 1.2)


@pytest.mark.parametrize("which", ("floor", "walls", "tilt"))
@pytest.mark.parametrize("kind", KINDS)
def test_each_rule_alone(G, kind, which):
    n, T = 130, 6
    spec = alone(kind, which)
    acts = R.commands(kind, n, T)
    env, twin = make(G, kind, n, term=spec), make(G, kind, n, term=None)
    seen = np.zeros(3, int)
    for t in range(T):
        o, r, d, fin, tr = env.step_final(acts[t])
        o2, r2, d2 = twin.step(acts[t])
        o2, r2, d2 = host(o2).copy(), host(r2).copy(), u8(d2).astype(bool)
        only = emulate(twin, kind, spec, o2, r2, d2)
        same(u8(d).astype(bool), d2, "done"), same(r, r2, "rew"), same(o, o2, "obs")
        nf, out, tilt = R.parts(kind, host(fin)[only], *spec)
        seen += (int(nf.sum()), int(out.sum()), int(tilt.sum()))
        assert (out if which != "tilt" else tilt).all(), "the stored terminal state is outside this rule"
    assert seen[0] == 0 and (seen[1] > 0) == (which != "tilt") and (seen[2] > 0) == (which == "tilt"), (which, seen)
    env.close(), twin.close()


@pytest.mark.parametrize("kind", ("quad2d_sl", "quad3d_sl"))
def test_the_load_leaves_first(G, kind):
    """a slung-load env whose load is outside the box while the quadrotor is inside ends; the quadrotor alone would not have"""
    n = 65
    d, L = R.DIM[kind], R.LOAD[kind]
    spec = ((-0.8,) * d, (0.8,) * d, None)
    env, twin = make(G, kind, n, term=spec), make(G, kind, n, term=None)
    s = env.get_state()
    s[:, :d] = np.clip(s[:, :d], -0.5, 0.5)
    s[:, L:L + d] = s[:, :d]
    s[::2, L + d - 1] -= F32(0.45)                   # every second load hangs 0.45 below its quadrotor: inside or outside by the height
    env.set_state(s), twin.set_state(s)
    acts = R.commands(kind, n, 1)
    o, r, dn, fin, tr = env.step_final(acts[0])
    dn, fin = u8(dn).astype(bool), host(fin)
    quad_out = (np.abs(fin[:, :d]) > F32(0.8)).any(1)
    load_out = (np.abs(fin[:, L:L + d]) > F32(0.8)).any(1)
    first = dn & load_out & ~quad_out
    assert first.sum() >= 3, "loads that left while their quadrotor was inside"
    o2, r2, d2 = twin.step(acts[0])
    assert not u8(d2)[first].any(), "the reference's rule does not end these"
    same(env.get_state()[first], fresh_states(kind, ids(n)[first], 1), "fresh state")
    running = ~dn
    assert running.any() and not R.rule(kind, env.get_state()[running], *spec).any()
    env.close(), twin.close()


@pytest.mark.parametrize("kind", KINDS)
def test_a_nan_component_ends_the_episode(G, kind):
    n = 65
    env, twin = make(G, kind, n, term="identity"), make(G, kind, n, term=None)
    s = env.get_state()
    bad = np.arange(n) % 3 == 0
    for i in np.nonzero(bad)[0]:
        s[i, i % NS[kind]] = np.nan
    env.set_state(s), twin.set_state(s)
    same(env.get_state(), s, "set_state is not tested by the rule")
    acts = R.commands(kind, n, 1)
    o, r, d = env.step(acts[0])
    d, r = u8(d).astype(bool), host(r)
    assert d[bad].all(), "done is 1"
    same(r[bad], np.ones(int(bad.sum()), F32), "the reward is the finite literal")
    now = env.get_state()
    assert np.isfinite(now).all(), "every env holds a finite state"
    same(now[bad], fresh_states(kind, ids(n)[bad], 1), "... the fresh one")
    o2, r2, d2 = twin.step(acts[0])
    t2 = twin.get_state()
    assert not u8(d2)[bad].any() and np.isnan(t2[bad]).any(1).all(), "a twin without a spec keeps its NaN"
    same(now[~bad & ~d], t2[~bad & ~d], "the other envs are the twin's")
    env.close(), twin.close()


# ---- 5. identity and NULL ---------------------------------------------------------------------------------------------------------------------
def with_spec(G, kind, n, how, **kw):
    """how: "never" = a handle that never had a spec; "identity" = the all-infinite spec assigned; "none" = the tests' spec assigned, then
    switched back with None"""
    env = make(G, kind, n, term=None, **kw)
    if how == "identity":
        env.termination = G.Termination()
        assert env.termination is not None
    elif how == "none":
        env.termination = term_of(G, R.spec(kind))
        env.termination = None
        assert env.termination is None
    return env


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,config", [(m, "all") for m in SIZES] + [(m, c) for m in (63, 130) for c in ("plain", "limit")])
def test_the_identity_and_none_store_the_bits_of_a_handle_without_a_spec(G, kind, n, config):
    outs = {}
    for how in ("never", "identity", "none"):
        env = with_spec(G, kind, n, how, **TD.CONFIGS[config])
        outs[how] = TD.run_ops(G, env, kind, n)
        env.close()
    for how in ("identity", "none"):
        assert set(outs[how]) == set(outs["never"])
        for key in outs["never"]:
            same(outs[how][key], outs["never"][key], f"{how}, {config}: {key}")
    done = np.concatenate([outs["never"][key].ravel() for key in outs["never"] if key.startswith("done:")])
    assert done.any() or config == "plain"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,T", [(65, 12), (130, 3)])
def test_the_identity_in_every_route(G, kind, n, T):
    """the all-infinite spec through every route of section 2, against ONE run of a handle that never had a spec"""
    bases = routes(G, kind, n, T, lambda: make(G, kind, n, term="identity"))
    for mode, base in bases.items():
        env = make(G, kind, n, term=None)
        plain = TD.final(env, env.rollout(T, mode=mode, actions=R.commands(kind, n, T) if mode == "buffer" else None, layout="aos", want=WANT))
        same_run(plain, base, f"identity, {mode}")


@pytest.mark.parametrize("actor", TD.ACTORS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,config", [(33, "plain"), (65, "norm_boot"), (130, "all")])
def test_the_identity_through_the_three_actors(G, actor, kind, n, config):
    outs = {}
    kw, norm = TD.POLICY_CONFIGS[config]
    for how in ("never", "identity", "none"):
        env = with_spec(G, kind, n, how, **({**kw, "reward": TD.tracking(G)} if kw.get("reward") else kw))
        outs[how] = TD.collect(env, actor, 12, norm, clip_actions=(-0.5, 0.5) if config == "all" else None)
        env.close()
    for how in ("identity", "none"):
        for key in outs["never"]:
            same(outs[how][key], outs["never"][key], f"{actor} {config} {how}: {key}")
    assert config == "plain" or outs["never"]["done"].any()


# ---- 6. composition ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_the_time_limit_termination_wins(G, kind):
    n, T, H = 130, 12, 3
    acts = R.commands(kind, n, T)
    spec = R.spec(kind)
    routes(G, kind, n, T, lambda: make(G, kind, n, max_episode_steps=H), modes=("buffer",))
    env = make(G, kind, n, max_episode_steps=H)
    length = np.zeros(n, int)
    at_limit = truncated = 0
    for t in range(T):
        o, r, d, fin, tr = env.step_final(acts[t])
        d, tr, fin = u8(d).astype(bool), u8(tr).astype(bool), host(fin)
        length += 1
        fired = np.zeros(n, bool)
        fired[d] = R.rule(kind, fin[d], *spec)
        assert not tr[fired].any(), "a rule termination is never truncated"
        assert (length[tr] == H).all() and (d[length == H]).all()
        at_limit += int((fired & (length == H)).sum())
        truncated += int(tr.sum())
        same(u8(env.episode_truncated())[d], tr[d].astype(np.uint8), "episode_truncated")
        length[d] = 0
    assert at_limit > 0 and truncated > 0, "rule terminations at L == H, and truncations"
    env.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", (65, 130))
def test_frame_skip_breaks_at_the_first_rule_termination(G, kind, n):
    """the twin with frame_skip = 1, stepped sub-step by sub-step: an env that ended inside an agent step is put back behind the later
    sub-steps; R is the fp32 sum of the sub-step rewards in order"""
    T, k = 6, 3
    acts = R.commands(kind, n, T)
    spec = R.spec(kind)
    routes(G, kind, n, T, lambda: make(G, kind, n, frame_skip=k), modes=("buffer", "random"))
    env, twin = make(G, kind, n, frame_skip=k), make(G, kind, n, term=None)
    tr = env.rollout(T, mode="buffer", actions=acts, layout="aos", want=WANT)
    obs, rew, done = [], [], []
    broke = 0
    for t in range(T):
        live = np.ones(n, bool)
        R_sum, o_t = np.zeros(n, F32), np.zeros((n, NS[kind]), F32)
        for j in range(k):
            snap = (twin.get_state(), twin.get_sbd(), twin.get_reset_counts())
            o, r, d = twin.step(acts[t])
            o, r, d = host(o).copy(), host(r).copy(), u8(d).astype(bool)
            emulate(twin, kind, spec, o, r, d)
            if not live.all():   # the envs that left this agent step earlier did not take this sub-step
                s, sbd, rc = twin.get_state(), twin.get_sbd(), twin.get_reset_counts()
                s[~live], sbd[~live], rc[~live] = snap[0][~live], snap[1][~live], snap[2][~live]
                twin.set_state(s), twin.set_sbd(sbd), twin.set_reset_counts(rc)
            R_sum[live] = r[live] if j == 0 else (R_sum[live] + r[live]).astype(F32)
            o_t[live] = o[live]
            broke += int((live & d).sum()) if j < k - 1 else 0
            live &= ~d
        obs.append(o_t), rew.append(R_sum), done.append((~live).astype(np.uint8))
    tw = dict(obs=np.stack(obs), rew=np.stack(rew), done=np.stack(done), state=twin.get_state(), rc=twin.get_reset_counts(), sbd=twin.get_sbd())
    check_against_twin(env, tr, tw, "frame skip: ")
    assert broke > 0, "agent steps that broke before their last sub-step"
    env.close(), twin.close()


@pytest.mark.parametrize("kind", KINDS)
def test_the_tracking_reward_pays_terminal_on_rule_terminations(G, kind):
    n, T = 130, 12
    acts = R.commands(kind, n, T)
    spec = R.spec(kind)
    routes(G, kind, n, T, lambda: make(G, kind, n, reward=True), modes=("buffer", "controller"))
    env, twin = make(G, kind, n, reward=True), make(G, kind, n, term=None, reward=True)
    seen = 0
    for t in range(T):
        o, r, d, fin, tr = env.step_final(acts[t])
        d, r, fin = u8(d).astype(bool), host(r), host(fin)
        o2, r2, d2 = twin.step(acts[t])
        d2 = u8(d2).astype(bool)
        only = d & ~d2
        assert (d | ~d2).all() and R.rule(kind, fin[only], *spec).all()
        same(r[only], np.full(int(only.sum()), -7.0, F32), "terminal on rule terminations")
        same(r[~only], host(r2)[~only], "every other reward is the twin's")
        s, sbd, rc = twin.get_state(), twin.get_sbd(), twin.get_reset_counts()   # (the twin follows where the rule ended an episode)
        s[only], sbd[only], rc[only] = env.get_state()[only], env.get_sbd()[only], env.get_reset_counts()[only]
        twin.set_state(s), twin.set_sbd(sbd), twin.set_reset_counts(rc)
        same(env.get_state(), twin.get_state(), "state"), same(env.get_reset_counts(), rc, "reset counts"), same(env.get_sbd(), sbd, "sbd")
        seen += int(only.sum())
    assert seen > 0
    env.close(), twin.close()


@pytest.mark.parametrize("kind", KINDS)
def test_actuator_lag_restarts_from_init_behind_a_rule_termination(G, kind):
    n, T = 130, 8
    acts = R.commands(kind, n, T)
    spec = R.spec(kind)
    lag = dict(actuator=G.Actuator(TAUS[NA[kind]], init=INIT[NA[kind]]))
    routes(G, kind, n, T, lambda: make(G, kind, n, **lag), modes=("buffer",))
    env = make(G, kind, n, **lag)
    init = np.asarray(INIT[NA[kind]], F32)
    seen = 0
    for t in range(T):
        o, r, d, fin, tr = env.step_final(acts[t])
        d, fin = u8(d).astype(bool), host(fin)
        fired = np.zeros(n, bool)
        fired[d] = R.rule(kind, fin[d], *spec)
        m = env.actuator_state()
        same(m[fired], np.tile(init, (int(fired.sum()), 1)), "m = init behind a rule termination")
        assert (m[~d] != init).any()
        seen += int(fired.sum())
    assert seen > 0
    env.close()


@pytest.mark.parametrize("config", ("ranged", "disturbed", "noisy", "start"))
@pytest.mark.parametrize("kind", KINDS)
def test_composition_by_route_equality(G, kind, config):
    n, T = 130, 12
    kw = dict(start_state=G.StartState(-0.75, 0.75)) if config == "start" else compose_kw(G, kind, config)
    bases = routes(G, kind, n, T, lambda: make(G, kind, n, **kw), modes=("buffer", "random"))
    base = bases["buffer"]
    assert base["done"].any() and base["rc"].max() >= 3
    if config == "start":   # every post-reset row lies in the start ranges: the rule's resets go through the map
        rows = base["obs"][base["done"].astype(bool)]
        assert len(rows) and (np.abs(rows) <= 0.75).all()
    if config != "noisy":    # the running envs' stored states satisfy the rule's complement
        running = ~base["done"].astype(bool)
        assert not R.rule(kind, base["obs"][running], *R.spec(kind)).any()


# ---- 7. in-kernel actors, by replay -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("actor", TD.ACTORS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,config", [(33, "plain"), (1, "norm_boot"), (63, "norm_boot"), (65, "plain"), (130, "norm_boot")])
def test_policy_rollouts_by_replay(G, actor, kind, n, config):
    kw, norm = TD.POLICY_CONFIGS[config]     # "norm_boot": a time limit with bootstrap_truncated, "plain": neither
    T = 12
    spec = R.spec(kind)
    env = make(G, kind, n, **kw)
    clip = (env.params.act_lo, env.params.act_hi)          # what clip_actions=True clips to
    out = TD.collect(env, actor, T, norm, clip_actions=True)
    env.close()
    # the stored actions, clipped on the host by the rule, replayed in buffer mode on a second spec'd handle from the same start
    u = np.clip(out["act"], F32(clip[0]), F32(clip[1])).astype(F32)      # [T, nA, n]
    twin = make(G, kind, n, **kw)
    tr = twin.rollout(T, mode="buffer", actions=np.ascontiguousarray(u), layout="soa", want=("obs", "rew", "done"))
    same(tr["obs"], out["obs"][1:], "obs"), same(tr["rew"], out["rew"], "rew"), same(u8(tr["done"]), u8(out["done"]), "done")
    same(twin.get_state(), out["state"], "final state"), same(twin.get_reset_counts(), out["rc"], "reset counts")
    same(twin.get_sbd(), out["sbd"], "steps_beyond_done")
    twin.close()
    done = u8(out["done"]).astype(bool)
    running = np.ascontiguousarray(out["obs"][1:].transpose(0, 2, 1))[~done]
    assert not R.rule(kind, running, *spec).any(), "no running env holds a state the rule ends"
    assert n == 1 or done.any()
    if config == "norm_boot":   # boot is 0 wherever the episode terminated: it is non-zero only on truncations
        trunc = u8(out["trunc"]).astype(bool)
        assert not out["boot"][done & ~trunc].any() and (trunc <= done).all()
        assert n == 1 or (done & ~trunc).any()


# ---- 8. sharding ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_two_shards_equal_the_whole(G, kind):
    n, k, T = 130, 65, 12
    acts = R.commands(kind, n, T)
    outs = []
    for first, count in ((0, n), (0, k), (k, n - k)):
        env = make(G, kind, count, base=BASE + first)
        tr = env.rollout(T, mode="buffer", actions=np.ascontiguousarray(acts[:, first:first + count]), layout="aos", want=WANT)
        outs.append((host(tr["obs"]), host(tr["rew"]), env.get_state(), env.get_reset_counts()))
        env.close()
    for i in range(4):
        axis = 1 if i < 2 else 0
        same(outs[0][i], np.concatenate([outs[1][i], outs[2][i]], axis=axis), f"shards {i}")
    assert outs[0][3].max() >= 3


# ---- 9. set semantics and refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_set_semantics(G, kind):
    from gym_reinmav_amd import _abi as A

    n, T = 65, 6
    acts = R.commands(kind, n, 2 * T)
    spec = R.spec(kind)
    env, twin = make(G, kind, n, term=None), make(G, kind, n, term=None)
    s0, rc0 = env.get_state(), env.get_reset_counts()
    tr = env.rollout(T, mode="buffer", actions=acts[:T], layout="aos", want=WANT)
    tw = twin.rollout(T, mode="buffer", actions=acts[:T], layout="aos", want=WANT)
    same(tr["obs"], tw["obs"], "before the set: a handle without a spec")
    env.termination = term_of(G, spec)
    same(env.get_state(), twin.get_state(), "a set touches no state"), same(env.get_reset_counts(), twin.get_reset_counts(), "... and no reset count")
    # get returns the last spec and whether it is enabled, also while it is switched off
    got = env.termination
    d = R.DIM[kind]
    assert got.pos_lo == tuple(float(F32(x)) for x in spec[0]) and got.pos_hi == tuple(float(F32(x)) for x in spec[1]) and got.max_tilt == float(F32(spec[2]))
    s, on = A.TerminationSpec(), C.c_int32(7)
    L = A.lib()
    assert L.rmav_get_termination(env._h, C.byref(s), C.byref(on)) == 0 and on.value == 1 and s._reserved == 0
    assert d == 3 or (s.pos_lo[2] == -INF and s.pos_hi[2] == INF)
    assert L.rmav_get_termination(env._h, None, None) == 0
    # a set mid-run acts from the next step: the emulated twin from here
    tr = env.rollout(T, mode="buffer", actions=acts[T:], layout="aos", want=WANT)
    check_against_twin(env, tr, twin_walk(twin, kind, acts[T:], spec), "after the set: ")
    assert u8(tr["done"]).any()
    env.termination = None
    assert L.rmav_get_termination(env._h, C.byref(s), C.byref(on)) == 0 and on.value == 0 and s.max_tilt == float(F32(spec[2]))
    tr = env.rollout(3, mode="buffer", actions=acts[:3], layout="aos", want=WANT)
    tw = twin.rollout(3, mode="buffer", actions=acts[:3], layout="aos", want=WANT)
    for key in WANT:
        same(tr[key], tw[key], f"after None: {key}")
    env.close(), twin.close()


def test_a_set_between_two_policy_rollouts_is_ordered_on_the_stream(G):
    """the policy kernels read the device copy, which the set rewrites in stream order: no synchronisation between the launches"""
    kind, n, T = "quad3d", 65, 12
    kw, norm = TD.POLICY_CONFIGS["norm_boot"]
    env = make(G, kind, n, term=((-INF,) * 3, (INF,) * 3, 3.0), **kw)
    TD.collect(env, "f16", T, norm)
    tight = ((-0.5,) * 3, (0.5,) * 3, 0.8)
    env.termination = term_of(G, tight)
    second = TD.collect(env, "f16", T, norm)
    done = u8(second["done"]).astype(bool)
    running = np.ascontiguousarray(second["obs"][1:].transpose(0, 2, 1))[~done]
    assert done.any() and len(running) and not R.rule(kind, running, *tight).any()
    env.close()


def test_a_captured_collector_collects_the_same_rollouts(G):
    import torch
    from gym_reinmav_amd.ppo import MlpPolicy, RolloutCollector

    kind, n, T = "quad2d", 65, 4
    spec = R.spec(kind)
    outs = []
    for graph in (False, True):
        env = make(G, kind, n, max_episode_steps=3)
        torch.manual_seed(4)
        pol = MlpPolicy(env.nS, env.nA, init_logstd=-0.5).cuda()
        col = RolloutCollector(env, pol, T, graph=graph, deterministic=True, bootstrap_truncated=True)
        runs = []
        for it in range(3):
            col.collect()
            torch.cuda.synchronize()
            runs.append((col.obs.cpu().numpy().copy(), col.act.cpu().numpy().copy(), col.done.cpu().numpy().copy(), env.get_state(), env.get_reset_counts()))
            col.roll_over()
        outs.append(runs)
        env.close()
    for it in range(3):
        for j, what in enumerate(("obs", "actions", "done", "state", "reset counts")):
            same(outs[0][it][j], outs[1][it][j], f"collect {it}: {what}")
    obs, done = outs[1][0][0], outs[1][0][2].astype(bool)       # [T + 1, nS, n], [T, n]
    running = np.ascontiguousarray(obs[1:].transpose(0, 2, 1))[~done]
    assert done.any() and not R.rule(kind, running, *spec).any()


def test_refusals(G):
    from gym_reinmav_amd import _abi as A
    from gym_reinmav_amd.ppo import FusedPolicyCollector

    L = A.lib()

    def refused(rc, word="termination"):
        assert rc == A.ERR_INVALID, rc
        msg = L.rmav_last_error().decode().lower()
        assert word in msg, msg

    def spec(lo, hi, tilt=INF, reserved=0):
        return A.TerminationSpec((C.c_float * 3)(*lo), (C.c_float * 3)(*hi), tilt, reserved)

    kind = "quad3d"
    env = make(G, kind, 8)
    good = env.termination
    nan = float("nan")
    ninf = (-INF,) * 3
    pinf = (INF,) * 3
    for bad in (spec((0.5, -INF, -INF), (0.25, INF, INF)),                 # lo > hi
                spec((nan, -INF, -INF), pinf), spec(ninf, (INF, nan, INF)), spec(ninf, pinf, nan),
                spec(ninf, pinf, -0.1), spec(ninf, pinf, 3.2), spec(ninf, pinf, -INF), spec(ninf, pinf, INF, 1),
                spec((INF, 0, 0), (-INF, 0, 0))):
        refused(L.rmav_set_termination(env._h, C.byref(bad)))
        now = env.termination
        assert now.pos_lo == good.pos_lo and now.pos_hi == good.pos_hi and now.max_tilt == good.max_tilt, "the spec in force stays"
    assert L.rmav_set_termination(env._h, C.byref(spec(ninf, pinf, float(F32(math.pi))))) == 0      # pi as fp32 rounds it
    env.termination = good
    # ReinmavEnv takes none
    rm = G.BatchedQuadrotor("reinmav", 4, seed=1)
    refused(L.rmav_set_termination(rm._h, C.byref(spec(ninf, pinf))))
    assert L.rmav_set_termination(rm._h, None) == 0
    with pytest.raises(ValueError):
        G.BatchedQuadrotor("reinmav", 4, seed=1, termination=G.Termination())
    rm.close()
    # the fp32 vector-ALU and bf16 actors
    for kwargs in (dict(f32_mfma=False), dict(bf16_mfma=True)):
        pol = TD.policy_of(env, "fp32_mfma", False)
        with pytest.raises(ValueError, match="termination"):
            FusedPolicyCollector(env, pol, 4, **kwargs)
    import torch
    w = torch.zeros(1 << 16, device="cuda")
    o = torch.zeros(1 << 16, device="cuda")
    for prec in (A.POLICY_FP32, A.POLICY_BF16_MFMA):
        refused(L.rmav_rollout_policy(env._h, 2, C.c_void_p(w.data_ptr()), None, None, None, None, C.c_void_p(o.data_ptr()), C.c_void_p(o.data_ptr()), prec))
    assert env.termination.max_tilt == good.max_tilt
    env.close()

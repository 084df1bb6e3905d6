"""Actuator lag (rmav_set_actuator) on the GPU.  The main oracle is the PRE-FILTERED TWIN: a handle without the feature, stepped one step
at a time with the m the numpy restatement (tests/actuator_ref.py, exact fp32 fma) computes from the same commands and the twin's own done
bytes, stores the bits of the lag handle - observations, rewards, done, final state, reset counts - and the restatement's m is the handle's
actuator_state().  Around it: every route gives the same bits; the state carries across launches and through a checkpoint; resets; tau = 0
is a handle without a spec; frame skip; composition with every other feature; the three in-kernel actors by replay; sharding; refusals;
a captured collector.  Every comparison is bit for bit except return_sum of the episode totals between routes (1e-4 relative)."""
import ctypes as C

import numpy as np
import pytest

import actuator_ref as R
import reward_ref as RW
import test_gpu_disturbance as TD
from test_gpu_disturbance import host, same, same_run
from util import BOX, KINDS, NA, NS

pytestmark = pytest.mark.gpu

SEED, BASE = 11, 300
SIZES = (1, 63, 65, 130)
STEPS = (3, 12)          # below and above the 8-step threshold of the spare reset state
WANT = ("actions", "obs", "rew", "done")
F32 = np.float32
TAUS = {2: (0.01, 0.02), 4: (0.01, 0.02, 0.015, 0.0)}                # one time constant per component (one of them: no lag)
INIT = {2: (1.5, -0.25), 4: (1.5, -0.25, 0.125, 0.0)}
# commands that end episodes inside a launch: the 2-D kinds at least twice per env in 12 steps (found with the CPU oracle; asserted below)
AMP = {"quad2d": 20.0, "quad2d_sl": 6000.0, "quad3d": 300.0, "quad3d_sl": 300.0}


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available()
    import gym_reinmav_amd as g

    return g


def make(G, kind, n, lag=True, base=BASE, tau=None, init="explicit", **kw):
    """A handle with the tests' seed and env ids; lag=False: the plain twin."""
    if kw.get("reward") is True:
        kw["reward"] = TD.tracking(G)
    act = None
    if lag:
        act = G.Actuator(TAUS[NA[kind]] if tau is None else tau, init=INIT[NA[kind]] if init == "explicit" else init)
    return G.BatchedQuadrotor(kind, n, seed=SEED, env_id_base=base, actuator=act, **kw)


def commands(kind, n, T=12):
    rng = np.random.RandomState(77 + n)
    nA = NA[kind]
    u = (AMP[kind] * np.where(rng.uniform(size=(T, n, nA)) < 0.5, -1.0, 1.0) * rng.uniform(0.5, 1.0, (T, n, nA))).astype(F32)
    u[..., 0] = np.abs(u[..., 0])
    if nA == 4:
        u[..., 1:] *= F32(0.01)
    assert not (u == 0).any()
    return u


def hover(env, kind, n, T, seed=3):
    """commands near the hover action: no episode ends"""
    rng = np.random.RandomState(seed + n)
    p = env.params
    h = np.zeros(NA[kind], F32)
    h[0] = p.mass * 9.8 / p.thrust_scale
    return (h[None, None, :] + 0.05 * rng.uniform(-1, 1, (T, n, NA[kind]))).astype(F32)


def lag_of(env):
    a = env.actuator
    return R.Lag(a.tau, env.params.dt, a.init, env.num_envs)


def u8(x):
    return host(x).astype(np.uint8)


def final(env, tr):
    """test_gpu_disturbance.final with the actuator state"""
    m = env.actuator_state() if env.actuator is not None else None
    out = TD.final(env, tr)
    if m is not None:
        out["m"] = m
    return out


def twin_walk(G, kind, n, acts, lag, k=1, **kw):
    """the plain twin stepped with the restatement's m -> obs, rew, done per agent step (k dynamics steps each), the twin's final state and rc"""
    twin = make(G, kind, n, lag=False, **kw)
    obs, rew, done = [], [], []
    for t in range(acts.shape[0]):
        live = np.ones(n, bool)
        r_sum = None
        for j in range(k):
            m = lag.step(acts[t], live=live)
            o, r, d = twin.step(m)
            d = u8(d).astype(bool)
            assert k == 1 or not d.any(), "the frame-skip twin wants commands that end no episode"
            r_sum = host(r).copy() if j == 0 else (r_sum + host(r)).astype(F32)
        lag.end_of_step(d)
        obs.append(host(o).copy()), rew.append(r_sum), done.append(d.astype(np.uint8))
    out = dict(obs=np.stack(obs), rew=np.stack(rew), done=np.stack(done), state=twin.get_state(), rc=twin.get_reset_counts(), sbd=twin.get_sbd())
    twin.close()
    return out


# ---- 1. the pre-filtered twin ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("n", SIZES)
def test_the_pre_filtered_twin(G, kind, n, T):
    acts = commands(kind, n, T)
    env = make(G, kind, n)
    lag = lag_of(env)
    same(env.actuator_state(), lag.m, "m = init when the feature is switched on")
    tr = env.rollout(T, mode="buffer", actions=acts, layout="aos", want=WANT)
    tw = twin_walk(G, kind, n, acts, lag)
    for key in ("obs", "rew", "done"):
        same(host(tr[key]).astype(tw[key].dtype), tw[key], f"{key}")
    same(env.get_state(), tw["state"], "final state")
    same(env.get_reset_counts(), tw["rc"], "reset counts")
    same(env.get_sbd(), tw["sbd"], "steps_beyond_done")
    same(env.actuator_state(), lag.m, "actuator state")
    same(env.actuator_state(layout="soa", device_out=True).T.contiguous(), lag.m, "actuator state, feature-major on the device")
    per_env = tw["done"].sum(0)
    if T == 12:
        assert per_env.min() >= (2 if kind in ("quad2d", "quad2d_sl") else 0) and per_env.max() >= 1, (kind, per_env.min(), per_env.max())
    env.close()


# ---- 2. routes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,T", [(1, 12), (63, 3), (65, 12), (130, 12), (130, 3)])
def test_every_route_gives_the_same_bits(G, kind, n, T):
    import torch

    acts = commands(kind, n, T)
    kw = dict(max_episode_steps=5) if n == 65 else {}

    def fresh():
        return make(G, kind, n, **kw)

    for mode in ("buffer", "random", "controller"):
        a_in = acts if mode == "buffer" else None
        env = fresh()
        base = final(env, env.rollout(T, mode=mode, actions=a_in, layout="aos", want=WANT))
        env = fresh()
        others = {"fused = 0": final(env, env.rollout(T, mode=mode, actions=a_in, layout="aos", fused=False, want=WANT))}
        env = fresh()
        singles = [env.rollout(1, mode=mode, actions=None if a_in is None else a_in[t:t + 1], layout="aos", want=WANT) for t in range(T)]
        others["single steps"] = final(env, {key: np.concatenate([host(x[key]) for x in singles]) for key in WANT})
        env = fresh()
        soa_in = None if a_in is None else torch.from_numpy(np.ascontiguousarray(a_in.transpose(0, 2, 1))).cuda()
        others["feature-major, device"] = final(env, env.rollout(T, mode=mode, actions=soa_in, layout="soa", want=WANT, device_out=True))
        if mode != "buffer":
            env = fresh()
            others["pitched"] = final(env, {key: v.contiguous() for key, v in env.rollout(T, mode=mode, layout="soa", want=WANT, device_out=True, pitched=True).items()})
            if n == 130:
                env = fresh()
                ch = env.rollout_chunked(T, mode=mode, chunk=64, want=WANT)
                others["chunk-major"] = final(env, {key: env.unchunk(v) for key, v in ch.items()})
        else:   # rmav_step itself, and rmav_step_control against step-then-control
            env = fresh()
            steps = [env.step(acts[t]) for t in range(T)]
            others["rmav_step"] = final(env, dict(actions=acts, obs=np.stack([host(x[0]) for x in steps]), rew=np.stack([host(x[1]) for x in steps]),
                                                  done=np.stack([u8(x[2]) for x in steps])))
        for name, other in others.items():
            same_run(base, other, f"{mode} {name}")
        assert "m" in base
    # rmav_control_step is control-then-step, rmav_step_control step-then-control: the command out, m inside
    a, b = fresh(), fresh()
    for t in range(3):
        u = a.control()
        same(a.actuator_state(), b.actuator_state(), "control() leaves m alone")
        o1, r1, d1 = a.step(u)
        u2, o2, r2, d2 = b.control_step()
        same(u, u2, "control_step: the command"), same(o1, o2, "control_step: obs"), same(r1, r2, "control_step: rew"), same(u8(d1), u8(d2), "control_step: done")
        o1, r1, d1 = a.step(acts[t])
        nxt1 = a.control()
        o2, r2, d2, nxt2 = b.step_control(acts[t])
        same(o1, o2, "step_control: obs"), same(nxt1, nxt2, "step_control: the next command"), same(u8(d1), u8(d2), "step_control: done")
        same(a.actuator_state(), b.actuator_state(), "step_control: m")
    a.close(), b.close()


# ---- 3. state across launches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_launch_splitting_and_the_checkpoint(G, kind, n):
    acts = commands(kind, n, 12)
    env = make(G, kind, n)
    whole = final(env, env.rollout(12, mode="buffer", actions=acts, layout="aos", want=WANT))
    env = make(G, kind, n)
    first = env.rollout(5, mode="buffer", actions=acts[:5], layout="aos", want=WANT)
    ckpt = dict(state=env.get_state(), sbd=env.get_sbd(), rc=env.get_reset_counts(), t=env.step_count, spec=env.actuator, m=env.actuator_state())
    second = env.rollout(7, mode="buffer", actions=acts[5:], layout="aos", want=WANT)
    split = final(env, {key: np.concatenate([host(first[key]), host(second[key])]) for key in WANT})
    same_run(whole, split, "5 + 7 steps")
    for restore_m in (True, False):
        env = make(G, kind, n, lag=False)
        env.set_state(ckpt["state"]), env.set_sbd(ckpt["sbd"]), env.set_reset_counts(ckpt["rc"])
        env.step_count = ckpt["t"]
        env.actuator = ckpt["spec"]
        same(env.actuator_state(), np.tile(np.asarray(ckpt["spec"].init, F32), (n, 1)), "a fresh handle starts from init")
        if restore_m:
            env.set_actuator_state(ckpt["m"])
            same(env.actuator_state(), ckpt["m"], "round trip")
        cont = env.rollout(7, mode="buffer", actions=acts[5:], layout="aos", want=("obs", "rew", "done"))
        if restore_m:
            for key in ("obs", "rew", "done"):
                same(cont[key], second[key], f"restored: {key}")
            same(env.get_state(), whole["state"], "restored: state"), same(env.actuator_state(), whole["m"], "restored: m")
        else:   # (a single env may have been reset by the checkpoint's last step: its m is init on both sides)
            # (a single env tells nothing: one that ends its episode with the continuation's first step emits the fresh state either way)
            assert (ckpt["m"] != np.asarray(ckpt["spec"].init, F32)[None]).any()
            assert n == 1 or not np.array_equal(host(cont["obs"]), host(second["obs"])), "the test sees the actuator state"
        env.close()


# ---- 4. resets --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", (1, 65, 130))
def test_resets(G, kind, n):
    acts = commands(kind, n, 12)
    init = np.asarray(INIT[NA[kind]], F32)
    for auto in (True, False):
        env = make(G, kind, n, auto_reset=auto)
        seen, finished = 0, np.zeros(n, bool)
        for T, single in ((3, False), (1, True), (8, False)):
            before = env.actuator_state()
            tr = env.rollout(T, mode="buffer", actions=acts[seen:seen + T], layout="aos", want=WANT) if not single else None
            d = u8(tr["done"])[-1].astype(bool) if tr else u8(env.step(acts[seen])[2]).astype(bool)
            finished |= u8(tr["done"]).any(0) if tr else d
            seen += T
            m = env.actuator_state()
            if auto:
                same(m[d], np.tile(init, (int(d.sum()), 1)), "finished envs start from init")
                assert not (m[~d] == init).all(axis=1).any(), "the others keep theirs"
            else:
                assert not (m == init).all(axis=1).any() and not np.array_equal(m, before), "without auto-reset a finished env keeps filtering"
        assert finished.any()
        env.reset()
        same(env.actuator_state(), np.tile(init, (n, 1)), "rmav_reset re-initialises")
        env.close()


# ---- 5. tau = 0 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_tau_zero_stores_the_bits_of_a_handle_without_a_spec(G, kind, n):
    """(caller and random actions, which contain no zero - asserted; the controller's may: the sign of a zero action is the one exception)"""
    outs = []
    for lag in (True, False):
        env = make(G, kind, n, lag=lag, tau=0.0, **TD.CONFIGS["limit"])
        outs.append(TD.run_ops(G, env, kind, n, ctrl=False))
        env.close()
    assert set(outs[0]) == set(outs[1])
    done = outs[1]["done:step_final"].astype(bool)
    for key in outs[1]:
        x, y = host(outs[0][key]), host(outs[1][key])
        if key.startswith("act:"):
            assert not (y == 0).any(), f"{key}: a zero action"
        if key.startswith("final:"):   # (rows of unfinished envs are not written)
            feature_major = x.shape == (NS[kind], n)
            same(x[:, done] if feature_major else x[done], y[:, done] if feature_major else y[done], key)
        else:
            same(x, y, f"tau = 0: {key}")


@pytest.mark.parametrize("actor", TD.ACTORS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,config", [(33, "plain"), (65, "norm_boot"), (130, "all")])
def test_tau_zero_through_the_three_actors(G, actor, kind, n, config):
    outs = []
    kw, norm = TD.POLICY_CONFIGS[config]
    for lag in (True, False):
        env = make(G, kind, n, lag=lag, tau=0.0, **kw)
        outs.append(TD.collect(env, actor, 12, norm, clip_actions=(-0.5, 0.5) if config == "all" else None))
        env.close()
    assert not (outs[1]["act"] == 0).any()
    for key in outs[1]:
        same(outs[0][key], outs[1][key], f"{actor} {config}: {key}")


# ---- 6. frame skip ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_frame_skip_filters_every_sub_step(G, kind, n):
    env = make(G, kind, n, frame_skip=3, init=None)
    acts = hover(env, kind, n, 4)
    lag = lag_of(env)
    tr = env.rollout(4, mode="buffer", actions=acts, layout="aos", want=WANT)
    tw = twin_walk(G, kind, n, acts, lag, k=3)
    assert not tw["done"].any()
    same(tr["obs"], tw["obs"], "obs"), same(tr["rew"], tw["rew"], "rew: summed in sub-step order"), same(env.actuator_state(), lag.m, "m after 12 dynamics steps")
    same(env.get_state(), tw["state"], "state")
    o, r, d = env.step(acts[0])                      # ... and the single-step kernel (an env that ends its episode here starts from init)
    for j in range(3):
        lag.step(acts[0])
    lag.end_of_step(u8(d).astype(bool))
    assert not u8(d).all()
    same(env.actuator_state(), lag.m, "k_step_al: three sub-steps")
    env.close()


def test_a_termination_inside_the_frame_skip_stops_the_filter(G):
    """quadrotor2d, one env, k = 3: with these commands (found with the CPU oracle) the first episode ends at sub-step 2 of 3 of the first
    agent step.  A handle without auto-reset mirrors a plain twin fed m sub-step by sub-step: m stops advancing with the sub-step that
    terminates; with auto-reset m is init after that step."""
    kind, n = "quad2d", 1
    acts = (commands(kind, n, 12) * F32(1.5)).astype(F32)
    env = make(G, kind, n, frame_skip=3, auto_reset=False)
    twin = make(G, kind, n, lag=False, auto_reset=False)
    lag = lag_of(env)
    hit = None
    for t in range(4):
        subs, d_t = 0, False
        for j in range(3):
            m = lag.step(acts[t])
            subs += 1
            d_t = bool(u8(twin.step(m)[2])[0])
            if d_t:
                break
        if t % 2:
            d = env.step(acts[t])[2]
        else:
            d = env.rollout(1, mode="buffer", actions=acts[t:t + 1], layout="aos", want=WANT)["done"][0]
        assert bool(u8(d)[0]) == d_t
        same(env.actuator_state(), lag.m, f"step {t}: m after {subs} sub-steps")
        same(env.get_state(), twin.get_state(), f"step {t}: state")
        if d_t and hit is None:
            hit = (t, subs)
    assert hit == (0, 2), f"the first episode should end at sub-step 2 of 3 of step 0, got {hit}: pick other commands"
    env.close(), twin.close()
    env = make(G, kind, n, frame_skip=3)
    assert u8(env.step(acts[0])[2])[0] == 1
    same(env.actuator_state(), np.asarray(INIT[2], F32)[None], "init after the step that ended the episode")
    env.close()


# ---- 7. composition ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", (63, 130))
def test_composition_with_every_other_feature(G, kind, n):
    import disturbance_ref as D
    import sensor_ref as SR

    kw = dict(max_episode_steps=3, randomize={"mass": (0.8, 1.2)}, reward=True, disturbance=TD.dist(G, D.SPEC))
    T = 6
    outs = {}
    for noisy in (True, False):
        env = make(G, kind, n, sensor_noise=G.SensorNoise(0.25) if noisy else None, **kw)
        acts = hover(env, kind, n, T)
        rw = env.reward
        m0 = lag_of(env).step(acts[0])
        tr = env.rollout(T, mode="buffer", actions=acts, layout="aos", want=WANT)
        obs_now = env.observe()
        outs[noisy] = dict(tr={k: host(v) for k, v in tr.items()}, obs_now=obs_now, state=env.get_state(), m=env.actuator_state(), rc=env.get_reset_counts())
        env.close()
    a, b = outs[True], outs[False]
    for key in ("rew", "done"):
        same(a["tr"][key], b["tr"][key], f"noise moves no {key}")
    for key in ("state", "m", "rc"):
        same(a[key], b[key], f"noise moves no {key}")
    same(a["tr"]["obs"][-1], a["obs_now"], "the rmav_observe rule: the last row is observe() right after the launch")
    same(b["tr"]["obs"][-1], b["state"], "without noise the row is the state")
    ref, bound = SR.o_ref(np.full(NS[kind], 0.25), SEED, BASE + np.arange(n), T, np.ascontiguousarray(b["state"], F32))
    assert (np.abs(a["obs_now"].astype(np.float64) - ref) / bound).max() <= 1.0
    assert np.abs(a["obs_now"] - b["state"]).max() > 0.01, "noise is there"
    # the action cost is that of the COMMAND: the reward of step 0 is tests/reward_ref.py on u within the reward tests' bar
    # (1e-6 max(1, M): test_gpu_reward.py), and far from it on m, which starts at init
    spec = {f: (tuple(getattr(rw, f)) if hasattr(getattr(rw, f), "__len__") else getattr(rw, f)) for f in rw.FIELDS}
    live = ~b["tr"]["done"][0].astype(bool)
    post, r0 = b["tr"]["obs"][0], b["tr"]["rew"][0].astype(np.float64)
    ref_u, M = RW.reward_ref(kind, post, acts[0], spec, np.zeros(n, bool))
    ref_m, _ = RW.reward_ref(kind, post, m0, spec, np.zeros(n, bool))
    assert live.any() and (np.abs(r0 - ref_u) / np.maximum(1.0, M))[live].max() <= 1e-6, "the reward reads u"
    assert (np.abs(r0 - ref_m) / np.maximum(1.0, M))[live].min() > 1e-4, "... and the test can tell u from m"


# ---- 8. policy rollouts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("actor", TD.ACTORS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,config", [(33, "plain"), (1, "norm_boot"), (63, "norm_boot"), (65, "plain"), (130, "norm_boot")])
def test_policy_rollouts_by_replay(G, actor, kind, n, config):
    kw, norm = TD.POLICY_CONFIGS[config]
    T = 12
    env = make(G, kind, n, **kw)
    clip = (env.params.act_lo, env.params.act_hi)          # what clip_actions=True clips to
    out = TD.collect(env, actor, T, norm, clip_actions=True)
    m_end = env.actuator_state()
    env.close()
    plain = make(G, kind, n, lag=False, **kw)
    first = TD.collect(plain, actor, 1, norm, clip_actions=True)
    plain.close()
    same(out["act"][0], first["act"][0], "the first action is that of a handle without lag")
    same(out["logp"][0], first["logp"][0], "... and its log-probability")
    # the stored actions, clipped on the host by the rule, replayed on a twin lag handle
    u = np.clip(out["act"], F32(clip[0]), F32(clip[1])).astype(F32)      # [T, nA, n]
    twin = make(G, kind, n, **kw)
    tr = twin.rollout(T, mode="buffer", actions=np.ascontiguousarray(u), layout="soa", want=("obs", "rew", "done"))
    same(tr["obs"], out["obs"][1:], "obs"), same(tr["rew"], out["rew"], "rew"), same(u8(tr["done"]), u8(out["done"]), "done")
    same(twin.get_state(), out["state"], "final state"), same(twin.actuator_state(), m_end, "final actuator state")
    same(twin.get_reset_counts(), out["rc"], "reset counts")
    assert kind != "quad3d" or n == 1 or np.abs(u - out["act"]).max() > 0, "the clip bites (quadrotor3d's box starts at 0)"
    twin.close()


# ---- 9. sharding ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_two_shards_equal_the_whole(G, kind):
    n, k, T = 130, 65, 12
    acts = commands(kind, n, T)
    outs = []
    for first, count in ((0, n), (0, k), (k, n - k)):
        env = make(G, kind, count, base=BASE + first)
        tr = env.rollout(T, mode="buffer", actions=np.ascontiguousarray(acts[:, first:first + count]), layout="aos", want=WANT)
        outs.append((host(tr["obs"]), host(tr["rew"]), env.get_state(), env.actuator_state()))
        env.close()
    for i in range(4):
        axis = 1 if i < 2 else 0
        same(outs[0][i], np.concatenate([outs[1][i], outs[2][i]], axis=axis), f"shards {i}")


# ---- 10. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(G):
    from gym_reinmav_amd import _abi as A
    from gym_reinmav_amd.ppo import FusedPolicyCollector

    L = A.lib()

    def refused(rc):
        assert rc == A.ERR_INVALID, rc
        msg = L.rmav_last_error().decode().lower()
        assert "actuator" in msg, msg

    env = make(G, "quad3d", 8)
    good = env.actuator
    nan, inf = float("nan"), float("inf")
    for tau, init in (((-0.1, 0, 0, 0), (0,) * 4), ((nan, 0, 0, 0), (0,) * 4), ((0, inf, 0, 0), (0,) * 4), ((0.1,) * 4, (0, nan, 0, 0)), ((0.1,) * 4, (inf, 0, 0, 0))):
        spec = A.ActuatorSpec((C.c_float * 4)(*tau), (C.c_float * 4)(*init))
        refused(L.rmav_set_actuator(env._h, C.byref(spec)))
        now = env.actuator
        assert now.tau == good.tau and now.init == good.init, "the spec in force stays"
    env2 = make(G, "quad2d", 8)
    for tau, init in (((0.1, 0.1, 0.1, 0), (0,) * 4), ((0.1, 0.1, 0, 0), (0, 0, 0, 1.0))):
        refused(L.rmav_set_actuator(env2._h, C.byref(A.ActuatorSpec((C.c_float * 4)(*tau), (C.c_float * 4)(*init)))))
    assert env2.actuator.tau == TAUS[2] or np.allclose(env2.actuator.tau, TAUS[2])
    # without a spec there is no state
    env2.actuator = None
    assert env2.actuator is None
    buf = np.zeros((8, 2), F32)
    refused(L.rmav_set_actuator_state(env2._h, buf.ctypes.data_as(C.POINTER(C.c_float)), A.HOST, A.AOS if hasattr(A, "AOS") else 1))
    with pytest.raises(G.RmavError):
        env2.actuator_state()
    s, on = A.ActuatorSpec(), C.c_int32(7)
    assert L.rmav_get_actuator(env2._h, C.byref(s), C.byref(on)) == 0 and on.value == 0 and list(s.tau)[:2] == [F32(x) for x in TAUS[2]]
    assert L.rmav_get_actuator(env2._h, None, None) == 0
    env2.close()
    # ReinmavEnv takes none
    rm = G.BatchedQuadrotor("reinmav", 4, seed=1)
    refused(L.rmav_set_actuator(rm._h, C.byref(A.ActuatorSpec())))
    rm.close()
    # the fp32 vector-ALU and bf16 actors
    for kwargs in (dict(f32_mfma=False), dict(bf16_mfma=True)):
        pol = TD.policy_of(env, "fp32_mfma", False)
        with pytest.raises(ValueError, match="actuator"):
            FusedPolicyCollector(env, pol, 4, **kwargs)
    import torch
    w = torch.zeros(1 << 16, device="cuda")
    o = torch.zeros(1 << 16, device="cuda")
    for prec in (A.POLICY_FP32, A.POLICY_BF16_MFMA):
        refused(L.rmav_rollout_policy(env._h, 2, C.c_void_p(w.data_ptr()), None, None, None, None, C.c_void_p(o.data_ptr()), C.c_void_p(o.data_ptr()), prec))
    assert env.actuator.tau == good.tau
    env.close()


# ---- 11. graph --------------------------------------------------------------------------------------------------------------------------------
def test_a_captured_collector_advances_the_actuator_state(G):
    import torch
    from gym_reinmav_amd.ppo import MlpPolicy, RolloutCollector

    kind, n, T = "quad3d", 65, 4
    outs = []
    for graph in (False, True):
        env = make(G, kind, n, init=None)
        torch.manual_seed(4)
        pol = MlpPolicy(env.nS, env.nA, init_logstd=-0.5).cuda()
        col = RolloutCollector(env, pol, T, graph=graph, deterministic=True)
        ms = []
        for it in range(3):
            col.collect()
            torch.cuda.synchronize()
            ms.append((env.actuator_state(), col.obs.cpu().numpy().copy(), col.act.cpu().numpy().copy()))
            col.roll_over()
        outs.append(ms)
        env.close()
    for it in range(3):
        for j, what in enumerate(("actuator state", "obs", "actions")):
            same(outs[0][it][j], outs[1][it][j], f"collect {it}: {what}")
    assert not np.array_equal(outs[0][0][0], outs[0][2][0]), "m moves from one collect to the next"

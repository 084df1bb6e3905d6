"""Start-state ranges (rmav_set_start_state) on the GPU.  The main oracle is the RE-SEEDED TWIN: a handle without the feature, same seed and
env ids, stepped one step at a time under the same commands; wherever its done byte is 1 its fresh state is the reference's draw v, which the
test overwrites with fma32(h, v, m) (tests/start_ref.py, the exact fp32 fma) through set_state.  The twin's observations, rewards, done bytes,
final state, reset counts and steps_beyond_done are the bits the spec'd handle stores from ONE fused launch.  Around it: reset(); every route
gives the same bits; the identity spec and None are a handle without a spec; composition with every other feature; the three in-kernel
actors by replay; sharding; set semantics; refusals.  Every comparison is bit for bit except return_sum of the episode totals between routes
(1e-4 relative)."""
import ctypes as C

import numpy as np
import pytest

import start_ref as R
import test_gpu_disturbance as TD
from test_gpu_disturbance import host, same, same_run
from test_gpu_actuator import INIT, TAUS, commands, u8
from util import KINDS, NA, NS

pytestmark = pytest.mark.gpu

SEED, BASE = 11, 300
SIZES = (1, 63, 65, 130)
STEPS = (3, 12)          # below and above the 8-step threshold of the spare reset state
WANT = ("actions", "obs", "rew", "done")
F32 = np.float32


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available()
    import gym_reinmav_amd as g

    return g


def start_of(G, lo_hi):
    lo, hi = lo_hi
    return G.StartState(tuple(float(x) for x in lo), tuple(float(x) for x in hi))


def make(G, kind, n, start="ranges", base=BASE, **kw):
    """A handle with the tests' seed and env ids.  start: "ranges" (tests/start_ref.ranges), "identity", or None = the plain twin.  The
    constructor keyword sets the spec and resets: such a handle's running episodes were drawn at reset index 1."""
    if kw.get("reward") is True:
        kw["reward"] = TD.tracking(G)
    ss = None if start is None else start_of(G, R.ranges(kind) if start == "ranges" else R.identity(kind))
    return G.BatchedQuadrotor(kind, n, seed=SEED, env_id_base=base, start_state=ss, **kw)


def ids(n, base=BASE):
    return base + np.arange(n)


def expected_start(kind, env_ids, episodes, lo_hi=None):
    lo, hi = lo_hi if lo_hi is not None else R.ranges(kind)
    return R.start_states(kind, SEED, env_ids, episodes, lo, hi)


def twin_of(G, kind, n, base=BASE, **kw):
    """The plain twin from the spec'd handle's start: reset once (index 1, as the constructor keyword does), then mapped by the test."""
    twin = make(G, kind, n, start=None, base=base, **kw)
    twin.reset()
    lo, hi = R.ranges(kind)
    twin.set_state(R.map_state(lo, hi, twin.get_state()))
    return twin


def twin_walk(twin, kind, acts):
    """The twin stepped one step at a time; after every step the envs whose done byte is 1 hold the reference's draw v and are overwritten
    with the mapped state -> obs (after the overwrite), rew, done per step."""
    lo, hi = R.ranges(kind)
    noisy = twin.sensor_noise is not None
    obs, rew, done = [], [], []
    for t in range(acts.shape[0]):
        o, r, d = twin.step(acts[t])
        o, d = host(o).copy(), u8(d).astype(bool)
        if d.any():
            s = twin.get_state()
            if not noisy:
                same(o[d], s[d], "the twin's post-reset observation is its fresh state")
            s[d] = R.map_state(lo, hi, s[d])
            twin.set_state(s)
            o[d] = twin.observe()[d] if noisy else s[d]
        obs.append(o), rew.append(host(r).copy()), done.append(d.astype(np.uint8))
    return dict(obs=np.stack(obs), rew=np.stack(rew), done=np.stack(done), state=twin.get_state(), rc=twin.get_reset_counts(), sbd=twin.get_sbd())


def check_against_twin(env, tr, tw, what=""):
    for key in ("obs", "rew", "done"):
        same(host(tr[key]).astype(tw[key].dtype), tw[key], f"{what}{key}")
    same(env.get_state(), tw["state"], f"{what}final state")
    same(env.get_reset_counts(), tw["rc"], f"{what}reset counts")
    same(env.get_sbd(), tw["sbd"], f"{what}steps_beyond_done")


# ---- 1. reset ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_reset_draws_the_mapped_state(G, kind, n):
    lo, hi = R.ranges(kind)
    env = make(G, kind, n)
    same(env.get_reset_counts(), np.full(n, 2, np.uint32), "the constructor keyword resets once: index 1")
    s1 = expected_start(kind, ids(n), 1)
    same(env.get_state(), s1, "the state behind the constructor")
    assert ((s1 >= lo) & (s1 <= hi)).all() and (s1[:, 1] == lo[1]).all() and (s1[:, 2] > 0).all()
    o2 = env.reset()                                             # a second reset: batch-major on the host
    s2 = expected_start(kind, ids(n), 2)
    same(o2, s2, "reset(): obs"), same(env.get_state(), s2, "reset(): state")
    assert n == 1 or not np.array_equal(s1, s2)
    o3 = env.reset(layout="soa", device_out=True)                # a third: feature-major on the device
    s3 = expected_start(kind, ids(n), 3)
    same(host(o3).T, s3, "reset(soa, device): obs"), same(env.get_state(layout="soa"), s3.T, "reset(soa, device): state")
    same(env.get_reset_counts(), np.full(n, 4, np.uint32), "reset counts")
    # a shifted reset counter moves the draw with it (set_reset_counts does not consult the spec, the next reset does)
    rc = (np.arange(n) * 7 + 40).astype(np.uint32)
    env.set_reset_counts(rc)
    same(env.get_state(), s3, "set_reset_counts leaves the state")
    same(env.reset(), expected_start(kind, ids(n), rc), "reset() at other indices")
    env.close()


# ---- 2. the re-seeded twin --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("n", SIZES)
def test_the_re_seeded_twin(G, kind, n, T):
    acts = commands(kind, n, T)
    env = make(G, kind, n)
    twin = twin_of(G, kind, n)
    same(env.get_state(), twin.get_state(), "both start from the same state")
    tr = env.rollout(T, mode="buffer", actions=acts, layout="aos", want=WANT)       # ONE fused launch
    tw = twin_walk(twin, kind, acts)
    check_against_twin(env, tr, tw)
    per_env = tw["done"].sum(0)
    if T == 12:   # the condition of this oracle: the spare AND the on-demand draw are exercised in every env
        assert per_env.min() >= (2 if kind in ("quad2d", "quad2d_sl") else 1), (kind, per_env.min(), per_env.max())
    # every post-reset row is the restatement at that env's reset index, inside the ranges
    lo, hi = R.ranges(kind)
    rc = np.full(n, 2, np.uint32)
    for t in range(T):
        d = tw["done"][t].astype(bool)
        if d.any():
            rows = host(tr["obs"])[t][d]
            same(rows, expected_start(kind, ids(n)[d], rc[d]), f"step {t}: post-reset rows")
            assert ((rows >= lo) & (rows <= hi)).all()
        rc += d.astype(np.uint32)
    env.close(), twin.close()


# ---- 3. routes --------------------------------------------------------------------------------------------------------------------------------
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
        if mode == "buffer" and T == 12:
            assert base["done"].any(), "episodes end inside the launch"
            if kw:
                assert base["rc"].min() >= 2 + 2, "with the limit every env was reset at least twice"
    # rmav_control_step is control-then-step
    a, b = fresh(), fresh()
    for t in range(3):
        u = a.control()
        o1, r1, d1 = a.step(u)
        u2, o2, r2, d2 = b.control_step()
        same(u, u2, "control_step: the command"), same(o1, o2, "control_step: obs"), same(r1, r2, "control_step: rew"), same(u8(d1), u8(d2), "control_step: done")
    same(a.get_state(), b.get_state(), "control_step: state")
    a.close(), b.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", (1, 65, 130))
def test_step_final_reports_the_unmapped_pre_reset_state(G, kind, n):
    """final_obs_out is the state the dynamics left - what a plain handle reports from the same state and action - and the post-reset
    observation is mapped; one size with a time limit, so that truncation resets are mapped too"""
    kw = dict(max_episode_steps=2) if n == 65 else {}
    acts = commands(kind, n, 6)
    env, twin = make(G, kind, n, **kw), twin_of(G, kind, n, **kw)
    lo, hi = R.ranges(kind)
    seen, truncated = 0, False
    for t in range(6):
        o, r, d, fin, tr = env.step_final(acts[t])
        o2, r2, d2, fin2, tr2 = twin.step_final(acts[t])
        d = u8(d).astype(bool)
        same(u8(d2), d.astype(np.uint8), "done"), same(r, r2, "rew"), same(u8(tr), u8(tr2), "truncated")
        same(host(fin)[d], host(fin2)[d], "final_obs: the pre-reset state, unmapped")
        same(host(o)[~d], host(o2)[~d], "obs of the running envs")
        if d.any():
            s = twin.get_state()
            s[d] = R.map_state(lo, hi, s[d])
            twin.set_state(s)
            same(host(o)[d], s[d], "the post-reset observation is mapped")
            seen += int(d.sum())
        truncated |= bool(u8(tr).any())
        same(env.get_state(), twin.get_state(), "state")
    assert seen > 0 and (truncated or not kw), "resets by termination and - with the limit - by truncation"
    env.close(), twin.close()


# ---- 4. identity ------------------------------------------------------------------------------------------------------------------------------
def with_spec(G, kind, n, how, **kw):
    """how: "never" = a handle that never had a spec; "identity" = the identity spec assigned (no reset: all three are at reset index 0);
    "none" = the tests' ranges assigned, then switched back with None"""
    env = make(G, kind, n, start=None, **kw)
    if how == "identity":
        env.start_state = start_of(G, R.identity(kind))
        assert env.start_state is not None
    elif how == "none":
        env.start_state = start_of(G, R.ranges(kind))
        env.start_state = None
        assert env.start_state is None
    return env


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,config", [(m, "all") for m in SIZES] + [(m, c) for m in (63, 130) for c in ("plain", "limit")])
def test_the_identity_and_none_store_the_bits_of_a_handle_without_a_spec(G, kind, n, config):
    outs = {}
    for how in ("never", "identity", "none"):
        env = with_spec(G, kind, n, how, **TD.CONFIGS[config])
        outs[how] = TD.run_ops(G, env, kind, n)
        outs[how]["reset"] = env.reset()
        env.close()
    for how in ("identity", "none"):
        assert set(outs[how]) == set(outs["never"])
        for key in outs["never"]:
            same(outs[how][key], outs["never"][key], f"{how}, {config}: {key}")
    done = np.concatenate([outs["never"][key].ravel() for key in outs["never"] if key.startswith("done:")])
    assert done.any() or config == "plain"


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


# ---- 5. composition ---------------------------------------------------------------------------------------------------------------------------
COMPOSE = {"ranged": dict(randomize={"mass": (0.8, 1.2), "tether_length": (0.4, 0.6)}), "skip": dict(frame_skip=3), "reward": dict(reward=True),
           "disturbed": "disturbance", "noisy": "sensor_noise", "lagged": "actuator"}


def compose_kw(G, kind, config):
    import disturbance_ref as D

    kw = COMPOSE[config]
    if kw == "disturbance":
        return dict(disturbance=TD.dist(G, D.SPEC))
    if kw == "sensor_noise":
        return dict(sensor_noise=G.SensorNoise(0.25))
    if kw == "actuator":
        return dict(actuator=G.Actuator(TAUS[NA[kind]], init=INIT[NA[kind]]))
    return dict(kw)


@pytest.mark.parametrize("config", sorted(COMPOSE))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", (65, 130))
def test_composition_with_every_other_feature(G, kind, n, config):
    import sensor_ref as SR

    T = 12
    acts = commands(kind, n, T)
    if config == "skip":   # (three dynamics steps per command: gentler commands still end episodes, asserted below)
        acts = (acts * F32(0.5)).astype(F32)
    env, twin = make(G, kind, n, **compose_kw(G, kind, config)), twin_of(G, kind, n, **compose_kw(G, kind, config))
    tr = env.rollout(T, mode="buffer", actions=acts, layout="aos", want=WANT)
    tw = twin_walk(twin, kind, acts)
    check_against_twin(env, tr, tw, f"{config}: ")
    assert tw["done"].any() and tw["rc"].max() >= 4, "a spare and an on-demand draw"
    if config == "lagged":     # m = init at the same resets: the twin's own auto-reset did that
        same(env.actuator_state(), twin.actuator_state(), "actuator state")
        last = tw["done"][-1].astype(bool)
        same(env.actuator_state()[last], np.tile(np.asarray(INIT[NA[kind]], F32), (int(last.sum()), 1)), "m = init where the last step reset")
    if config == "ranged":
        for name in ("mass",):
            same(env.get_env_param(name), twin.get_env_param(name), f"the constants of the running episodes: {name}")
    if config == "noisy":      # the observation a reset emits is the noisy observation of the mapped state (step t emits at the counter t + 1)
        rc, seen = np.full(n, 2, np.uint32), 0
        for t in range(T):
            d = tw["done"][t].astype(bool)
            if d.any():
                st = expected_start(kind, ids(n)[d], rc[d])
                ref, bound = SR.o_ref(np.full(NS[kind], 0.25), SEED, ids(n)[d], t + 1, st)
                rows = host(tr["obs"])[t][d]
                assert (np.abs(rows.astype(np.float64) - ref) / bound).max() <= 1.0, t
                assert np.abs(rows - st).max() > 0.01, "noise is there"
                seen += int(d.sum())
            rc += d.astype(np.uint32)
        assert seen > 0 and env.step_count == T
    env.close(), twin.close()


# ---- 6. in-kernel actors, by replay -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("actor", TD.ACTORS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,config", [(33, "plain"), (1, "norm_boot"), (63, "norm_boot"), (65, "plain"), (130, "norm_boot")])
def test_policy_rollouts_by_replay(G, actor, kind, n, config):
    kw, norm = TD.POLICY_CONFIGS[config]     # "norm_boot": a time limit with bootstrap_truncated, "plain": neither
    T = 12
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
    twin.close()
    # every post-reset observation row lies in [lo, hi] and is the restatement for that env and reset index
    lo, hi = R.ranges(kind)
    rc = np.full(n, 2, np.uint32)
    done = u8(out["done"]).astype(bool)
    for t in range(T):
        d = done[t]
        if d.any():
            rows = np.ascontiguousarray(out["obs"][t + 1].T[d])
            assert ((rows >= lo) & (rows <= hi)).all(), (t, rows)
            same(rows, expected_start(kind, ids(n)[d], rc[d]), f"step {t}: post-reset rows")
        rc += d.astype(np.uint32)
    same(rc, out["rc"], "reset counts follow the done bytes")
    assert config == "plain" or (done.sum(0) >= 2).all(), "with the limit every env is reset several times: the spare and the on-demand draw"


# ---- 7. sharding ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_two_shards_equal_the_whole(G, kind):
    n, k, T = 130, 65, 12
    acts = commands(kind, n, T)
    outs = []
    for first, count in ((0, n), (0, k), (k, n - k)):
        env = make(G, kind, count, base=BASE + first)
        tr = env.rollout(T, mode="buffer", actions=np.ascontiguousarray(acts[:, first:first + count]), layout="aos", want=WANT)
        outs.append((host(tr["obs"]), host(tr["rew"]), env.get_state(), env.get_reset_counts()))
        env.close()
    for i in range(4):
        axis = 1 if i < 2 else 0
        same(outs[0][i], np.concatenate([outs[1][i], outs[2][i]], axis=axis), f"shards {i}")
    assert outs[0][3].max() >= 4


# ---- 8. set semantics -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_set_semantics(G, kind):
    from gym_reinmav_amd import _abi as A

    n, T = 65, 12
    acts = commands(kind, n, T)
    env = make(G, kind, n, start=None)
    s0, rc0 = env.get_state(), env.get_reset_counts()
    env.start_state = start_of(G, R.ranges(kind))
    same(env.get_state(), s0, "a set draws nothing"), same(env.get_reset_counts(), rc0, "... and leaves the reset counts")
    # get / set round-trips the spec, also while it is switched off
    lo, hi = R.ranges(kind)
    got = env.start_state
    same(np.array(got.lo, F32), lo, "lo"), same(np.array(got.hi, F32), hi, "hi")
    s, on = A.StartStateSpec(), C.c_int32(7)
    L = A.lib()
    assert L.rmav_get_start_state(env._h, C.byref(s), C.byref(on)) == 0 and on.value == 1 and not any(s.lo[NS[kind]:]) and not any(s.hi[NS[kind]:])
    assert L.rmav_get_start_state(env._h, None, None) == 0
    # a launch enqueued after a set sees it: the running episodes (reset index 0) are the reference's, every later one is mapped
    import oracle as O

    same(s0, O.reset_states(kind, SEED, ids(n), 0), "the running episodes were drawn without the spec")
    tr = env.rollout(T, mode="buffer", actions=acts, layout="aos", want=WANT)
    done, rc = u8(tr["done"]).astype(bool), rc0.copy()
    for t in range(T):
        if done[t].any():
            same(host(tr["obs"])[t][done[t]], expected_start(kind, ids(n)[done[t]], rc[done[t]]), f"step {t}: the first resets after the set are mapped")
        rc += done[t].astype(np.uint32)
    assert done.any()
    env.start_state = None                                          # ... and one enqueued after the switch-off does not
    assert L.rmav_get_start_state(env._h, C.byref(s), C.byref(on)) == 0 and on.value == 0 and list(s.lo)[:NS[kind]] == list(lo)
    tr = env.rollout(T, mode="buffer", actions=acts, layout="aos", want=WANT)
    done = u8(tr["done"]).astype(bool)
    for t in range(T):
        if done[t].any():
            same(host(tr["obs"])[t][done[t]], O.reset_states(kind, SEED, ids(n)[done[t]], rc[done[t]]), f"step {t}: unmapped after None")
        rc += done[t].astype(np.uint32)
    same(env.get_reset_counts(), rc, "reset counts")
    with pytest.raises(G.RmavError):
        env.actuator_state()                                        # the gated filter does not show: there is no actuator state
    env.close()


def test_a_set_between_two_policy_rollouts_is_ordered_on_the_stream(G):
    """the policy kernels read the device copy, which the set rewrites in stream order: no synchronisation between the launches"""
    kind, n, T = "quad2d", 65, 12
    kw, norm = TD.POLICY_CONFIGS["norm_boot"]
    env = make(G, kind, n, **kw)
    first = TD.collect(env, "f16", T, norm)
    env.start_state = start_of(G, (np.full(NS[kind], 0.5, F32), np.full(NS[kind], 0.5, F32)))     # every component pinned
    second = TD.collect(env, "f16", T, norm)
    done = u8(second["done"]).astype(bool)
    assert done.any()
    for t in range(T):
        if done[t].any():
            assert (second["obs"][t + 1].T[done[t]] == F32(0.5)).all()
    d1 = u8(first["done"]).astype(bool)
    lo, hi = R.ranges(kind)
    assert d1.any() and all(((first["obs"][t + 1].T[d1[t]] >= lo) & (first["obs"][t + 1].T[d1[t]] <= hi)).all() for t in range(T))
    env.close()


def test_a_captured_collector_collects_the_same_rollouts(G):
    import torch
    from gym_reinmav_amd.ppo import MlpPolicy, RolloutCollector

    kind, n, T = "quad2d", 65, 4
    lo, hi = R.ranges(kind)
    outs = []
    for graph in (False, True):
        env = make(G, kind, n, max_episode_steps=3)
        torch.manual_seed(4)
        pol = MlpPolicy(env.nS, env.nA, init_logstd=-0.5).cuda()
        # (a captured collector carries the time limit's episode clock from one replay to the next on its bootstrap_truncated path)
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
    assert outs[1][2][4].min() >= 2 + 3, "the limit reset every env in every collect"
    obs, done = outs[1][0][0], outs[1][0][2].astype(bool)       # [T + 1, nS, n], [T, n]: the fresh rows lie in the ranges
    assert done.any() and all(((obs[t + 1].T[done[t]] >= lo) & (obs[t + 1].T[done[t]] <= hi)).all() for t in range(T))


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(G):
    from gym_reinmav_amd import _abi as A
    from gym_reinmav_amd.ppo import FusedPolicyCollector

    L = A.lib()

    def refused(rc, word="start"):
        assert rc == A.ERR_INVALID, rc
        msg = L.rmav_last_error().decode().lower()
        assert word in msg, msg

    def spec(lo, hi):
        return A.StartStateSpec((C.c_float * 16)(*lo), (C.c_float * 16)(*hi))

    kind = "quad3d"
    nS = NS[kind]
    env = make(G, kind, 8)
    good = env.start_state
    nan, inf = float("nan"), float("inf")
    z = [0.0] * 16
    for lo, hi in (([0.5] + z[1:], [0.25] + z[1:]),                    # lo > hi
                   ([nan] + z[1:], z), (z, [inf] + z[1:]), ([-inf] + z[1:], z), (z[:3] + [nan] + z[4:], z[:3] + [nan] + z[4:]),
                   (z[:nS] + [-0.5] + z[nS + 1:], z), (z, z[:15] + [1.0])):      # non-zero beyond nS
        refused(L.rmav_set_start_state(env._h, C.byref(spec(lo, hi))))
        now = env.start_state
        assert now.lo == good.lo and now.hi == good.hi, "the spec in force stays"
    # ReinmavEnv takes none
    rm = G.BatchedQuadrotor("reinmav", 4, seed=1)
    refused(L.rmav_set_start_state(rm._h, C.byref(spec(z, z))))
    assert L.rmav_set_start_state(rm._h, None) == 0
    with pytest.raises(ValueError):
        G.BatchedQuadrotor("reinmav", 4, seed=1, start_state=G.StartState(-0.5, 0.5))
    rm.close()
    # the fp32 vector-ALU and bf16 actors
    for kwargs in (dict(f32_mfma=False), dict(bf16_mfma=True)):
        pol = TD.policy_of(env, "fp32_mfma", False)
        with pytest.raises(ValueError, match="start"):
            FusedPolicyCollector(env, pol, 4, **kwargs)
    import torch
    w = torch.zeros(1 << 16, device="cuda")
    o = torch.zeros(1 << 16, device="cuda")
    for prec in (A.POLICY_FP32, A.POLICY_BF16_MFMA):
        refused(L.rmav_rollout_policy(env._h, 2, C.c_void_p(w.data_ptr()), None, None, None, None, C.c_void_p(o.data_ptr()), C.c_void_p(o.data_ptr()), prec), "start-state")
    assert env.start_state.lo == good.lo
    env.close()

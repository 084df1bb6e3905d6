"""Wind / gust disturbance (rmav_set_disturbance) on the GPU.  The pillars: rmav_disturbance_now is the contract's draw (the numpy
restatement tests/disturbance_ref.py, bit for bit, at the edges of every counter and across shards); the dynamics are the oracle's step
with g_vec + d (step_ref, teacher-forced from the GPU's own pre-step state, through in-launch resets and wind redraws); every route -
single step, fused and unfused rollouts, chunk-major - evaluates one body (bit equality); an all-zero spec and a constant wind reduce to
handles without the feature (bit equality: d enters exactly where gravity does); the controller keeps the undisturbed g_vec.

Tolerance: the project's parity bar is 1e-6 * max(1, |y|) for identical inputs; as tests/test_gpu_parity.py does for fp32 inputs
against fp64 arithmetic, 2e-6 is used, with either-branch acceptance where a slung-load step starts within 2e-6 of |tether| = L
(tests/test_disturbance_host.py shows that the inputs here contain no such step)."""
import numpy as np
import pytest

import disturbance_ref as R
import oracle as O
from util import CTRL_TOL, KINDS, NA, NS, near_threshold, scaled_err

pytestmark = pytest.mark.gpu

SEED, BASE, H, T = R.PARITY["seed"], R.PARITY["env_id_base"], R.PARITY["limit"], R.PARITY["steps"]
SIZES = (1, 63, 65, 130)
PTOL = 2e-6
WANT = ("actions", "obs", "rew", "done")
F32 = np.float32


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available()
    import gym_reinmav_amd as g

    return g


def dist(G, spec):
    return G.Disturbance(wind=tuple(zip(spec["wind_lo"], spec["wind_hi"])), gust=spec["gust"], hold=spec["gust_hold"])


def make(G, kind, n, spec=R.SPEC, base=BASE, **kw):
    """A handle with the tests' seed and env ids; spec: a dict of disturbance_ref, or None = a handle without a disturbance."""
    return G.BatchedQuadrotor(kind, n, seed=SEED, env_id_base=base, disturbance=None if spec is None else dist(G, spec), **kw)


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def same(a, b, what):
    a, b = np.ascontiguousarray(host(a)), np.ascontiguousarray(host(b))
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert a.tobytes() == b.tobytes(), (what, np.argwhere(a != b)[:5])


def now_ref(env, kind, spec, base=BASE):
    return R.disturbance_now(spec, kind, SEED, base + np.arange(env.num_envs), env.get_reset_counts(), env.step_count)


def set_tether(env, kind, phase):
    p, q = env.params, R.parity_params(kind, phase)
    p.tether_length = q.tether_length
    env.params = p
    return q


# ---- 1. rmav_disturbance_now ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_disturbance_now_is_the_contracts_draw(G, kind, n):
    env = make(G, kind, n, max_episode_steps=H)
    d0 = host(env.disturbance_now())
    assert d0.shape == (3, n) and d0.dtype == F32
    same(d0, now_ref(env, kind, R.SPEC), "fresh")
    if kind.startswith("quad2d"):
        assert (d0[2] == 0).all()
    rc0 = env.get_reset_counts()
    env.rollout(2, mode="random")                       # t = 2: the last step of gust block 0
    d2 = host(env.disturbance_now())
    same(d2, now_ref(env, kind, R.SPEC), "t = 2")
    keep = env.get_reset_counts() == rc0            # (a random action can end an episode early: that env has a new wind)
    same(d2[:, keep], d0[:, keep], "one wind, one gust block")
    assert keep.sum() >= n - n // 8
    env.rollout(1, mode="random")                       # t = 3: across the hold boundary, and the time limit has reset every env
    d3 = host(env.disturbance_now())
    same(d3, now_ref(env, kind, R.SPEC), "t = 3")
    assert (env.get_reset_counts() > rc0).all() and (d3[0] != d2[0]).all()
    env.rollout(4, mode="random", fused=False)
    same(env.disturbance_now(), now_ref(env, kind, R.SPEC), "after steps with resets")
    # the edges of the counters: the step counter around 2^32 and near 2^48, reset counts 0 (the running index wraps to 2^32 - 1) and 2^32 - 1
    rc = np.where(np.arange(n) % 3 == 0, 0, np.where(np.arange(n) % 3 == 1, 2**32 - 1, 7)).astype(np.uint32)
    env.set_reset_counts(rc)
    for t in (2**32 - 1, 2**32, 2**32 + 1, 3 * 2**32 - 1, 3 * 2**32, 2**48 - 2):
        env.step_count = t
        same(env.disturbance_now(), now_ref(env, kind, R.SPEC), f"t = {t}")
    env.close()


@pytest.mark.parametrize("kind", ("quad2d_sl", "quad3d"))
def test_disturbance_now_with_large_env_ids_and_across_shards(G, kind):
    n, big = 130, 2**40 + 77
    env = make(G, kind, n, base=big)
    env.step_count = 2**32 + 5
    whole = host(env.disturbance_now())
    same(whole, now_ref(env, kind, R.SPEC, base=big), "env_id_base > 2^40")
    a, b = make(G, kind, 70, base=big), make(G, kind, 60, base=big + 70)
    for e in (a, b):
        e.step_count = 2**32 + 5
    same(host(a.disturbance_now()), whole[:, :70], "shard 0")
    same(host(b.disturbance_now()), whole[:, 70:], "shard 1")
    for e in (env, a, b):
        e.close()


def test_a_4096_env_call_stays_inside_the_ranges(G):
    env = make(G, "quad3d", 4096)
    env.step_count = 12345
    d = host(env.disturbance_now())
    lo, hi, g = (np.array(R.SPEC[k], F32)[:, None] for k in ("wind_lo", "wind_hi", "gust"))
    assert (d >= lo - g).all() and (d <= hi + g).all()
    assert len(np.unique(d[0])) > 4000 and (np.abs(d[2] - F32(0.25)) <= g[2]).all()
    env.close()


# ---- 2. the dynamics are the oracle's step with g_vec + d --------------------------------------------------------------------------------------
def check_step(kind, p, s_pre, act, sbd, d, post, rew, term, what):
    """One batched device step against step_ref from the same inputs -> the worst scaled state error."""
    o, r, dn, _ = R.step_ref(kind, s_pre, act, sbd, p, d)
    err = scaled_err(post, o).max(axis=1)
    edge = np.zeros(len(s_pre), bool)
    if kind.endswith("_sl"):
        edge = np.abs(O.tether_slack(kind, s_pre.astype(np.float64), p)) < 2e-6
        for i in np.nonzero(edge)[0]:   # either branch of the oracle, from the very state and action the device saw
            alt = min(scaled_err(post[i], R.step_ref(kind, s_pre[i:i + 1], act[i:i + 1], sbd[i:i + 1], p, d[:, i:i + 1], force_taut=ft)[0][0]).max()
                      for ft in (0, 1))
            err[i] = min(err[i], alt)
    print(f"parity margin {kind} {what}: {err.max():.3g} of {PTOL:.3g} ({int(edge.sum())} tether-edge lanes)")
    assert err.max() <= PTOL, (what, float(err.max()), int(err.argmax()))
    near = near_threshold(kind, o, limits=(p.pos_limit, p.vel_limit)) | edge
    assert np.array_equal(term | near, dn | near), (what, np.nonzero((term != dn) & ~near)[0][:5])
    agree = (term == dn) & ~edge
    assert scaled_err(rew[agree], r[agree]).max() <= PTOL, what
    return o


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_step_follows_the_oracle_with_the_disturbed_gravity(G, kind, n):
    acts = R.parity_actions(kind, n)
    env = make(G, kind, n, max_episode_steps=H)
    p = set_tether(env, kind, "walk")
    seen = dict(trunc=0, done=0, redrawn=0, moved=0.0)
    d_prev = None
    for t in range(T):
        s_pre, sbd, rc = env.get_state(), env.get_sbd(), env.get_reset_counts()
        d = now_ref(env, kind, R.SPEC)
        same(env.disturbance_now(), d, f"disturbance_now before step {t}")
        o, r, dn, fin, tr = env.step_final(acts[t])
        post = np.where(dn[:, None], fin, o)
        ref = check_step(kind, p, s_pre, acts[t], sbd, d, post, r, dn & ~tr, f"n={n} walk step {t}")
        still, *_ = R.step_ref(kind, s_pre, acts[t], sbd, p, np.zeros_like(d))
        seen["moved"] = max(seen["moved"], float(scaled_err(ref, still).max()))
        seen["trunc"] += int(tr.sum())
        seen["done"] += int(dn.sum())
        assert np.array_equal(env.get_reset_counts(), rc + dn), "the reset index moves exactly with done"
        if d_prev is not None:   # d changes where the episode did, and inside a gust block only there
            assert (d[0] != d_prev[0])[done_prev].all(), t
            if t % R.SPEC["gust_hold"] != 0:
                same(d[:, ~done_prev], d_prev[:, ~done_prev], f"held through step {t}")
            seen["redrawn"] += int(done_prev.sum())
        d_prev, done_prev = d, dn.copy()
    assert seen["done"] >= 2 * n and seen["trunc"] >= n and seen["redrawn"] >= n and seen["moved"] > 1e-5, seen
    # freshly reset states with the default tether: the taut branch of the slung-load kinds (both bodies), no step on the tether edge
    p = set_tether(env, kind, "fresh")
    for j in range(R.PARITY["fresh"]):
        s_pre = env.reset()
        sbd = env.get_sbd()
        d = now_ref(env, kind, R.SPEC)
        o, r, dn, fin, tr = env.step_final(acts[T + j])
        check_step(kind, p, s_pre, acts[T + j], sbd, d, np.where(dn[:, None], fin, o), r, dn & ~tr, f"n={n} fresh step {j}")
    env.close()


# ---- 3. one body -------------------------------------------------------------------------------------------------------------------------------
def final(env, tr):
    tr = {key: host(v) for key, v in tr.items()}
    tot = env.episode_totals()
    tr.update(state=env.get_state(), sbd=env.get_sbd(), rc=env.get_reset_counts(), last_trunc=env.episode_truncated(),
              totals=np.array([tot[k] for k in sorted(tot)], np.float64), t=np.array([env.step_count]), **env.episode_buffers())
    env.close()
    return tr


def same_run(a, b, what):
    """Two runs of one trajectory through different launch groupings: every array bit for bit; of the totals (episodes, length_sum,
    return_sum) the two counts exactly and return_sum - a double sum of per-wavefront fp32 partial sums whose grouping differs between one
    launch and T: at most N T = 1040 terms, each partial sum within 1040 x 2^-24 = 6.2e-5 relative - within 1e-4 * max(1, |sum|), the
    bound of tests/test_gpu_frame_skip.py."""
    for key in a:
        x, y = a[key], np.asarray(b[key]).astype(a[key].dtype)
        if key in ("actions", "obs") and x.shape != y.shape:
            x = x.transpose(0, 2, 1)   # batch-major against feature-major
        if key == "totals":
            assert x[0] == y[0] and x[1] == y[1] and abs(x[2] - y[2]) <= 1e-4 * max(1.0, abs(x[2])), (what, x, y)
        else:
            same(x, y, f"{what}: {key}")


def tracking(G):
    return G.TrackingReward(goal=(0.3, -0.2, 0.5), alive=1.5, w_pos=2.0, w_vel=0.25, w_act=0.125, terminal=-7.0)


# (the reward variant of the kernels - RW = true - at 63 and 130 envs)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,rewarded", [(m, False) for m in SIZES] + [(63, True), (130, True)])
def test_fused_rollouts_equal_single_steps(G, kind, n, rewarded):
    acts = R.parity_actions(kind, n)[:T]
    kw = dict(max_episode_steps=H, reward=tracking(G) if rewarded else None)

    def fresh():
        return make(G, kind, n, **kw)

    for mode in ("buffer", "random", "controller"):
        a_in = acts if mode == "buffer" else None
        env = fresh()
        base = final(env, env.rollout(T, mode=mode, actions=a_in, layout="aos", want=WANT))
        env = fresh()
        unfused = final(env, env.rollout(T, mode=mode, actions=a_in, layout="aos", fused=False, want=WANT))
        env = fresh()
        singles = [env.rollout(1, mode=mode, actions=None if a_in is None else a_in[t:t + 1], layout="aos", want=WANT) for t in range(T)]
        stepped = final(env, {key: np.concatenate([host(x[key]) for x in singles]) for key in WANT})
        env = fresh()
        soa = env.rollout(T, mode=mode, actions=None if a_in is None else np.ascontiguousarray(a_in.transpose(0, 2, 1)), layout="soa", want=WANT,
                          device_out=True)
        soa = final(env, soa)
        chunked = None
        if mode != "buffer":   # the chunk-major layout: one launch per chunk
            env = fresh()
            ch = env.rollout_chunked(T, mode=mode, chunk=64, want=WANT)
            chunked = final(env, {key: env.unchunk(v) for key, v in ch.items()})
        for other, name in ((unfused, "fused = 0"), (stepped, "single steps"), (soa, "feature-major"), (chunked, "chunk-major")):
            if other is not None:
                same_run(base, other, f"{mode} {name}")
        assert base["done"].any() and (n == 1 or base["last_trunc"].any())   # (one env's last episode may have terminated instead)
        if mode == "buffer":   # ... and rmav_step itself
            env = fresh()
            steps = [env.step(acts[t]) for t in range(T)]
            st = final(env, dict(actions=acts, obs=np.stack([x[0] for x in steps]), rew=np.stack([x[1] for x in steps]),
                                 done=np.stack([x[2] for x in steps]).astype(np.uint8)))
            same_run(base, st, "rmav_step")


# ---- 4. / 5. reductions to handles without the feature --------------------------------------------------------------------------------------
def run_ops(G, env, kind, n, ctrl=True):
    """One sequence over the stepping entry points of rmav.h from the handle's fresh state -> {name: array}."""
    import torch

    rng = np.random.RandomState(21)
    acts = (R.parity_actions(kind, n)[0] + 0.05 * rng.uniform(-1, 1, (12, n, NA[kind]))).astype(F32)
    out = {}

    def put(name, **arrs):
        for key, v in arrs.items():
            out[key + ":" + name] = host(v).astype(np.uint8) if key in ("done", "trunc") else host(v)

    o, r, d = env.step(acts[0])
    put("step", obs=o, rew=r, done=d)
    o, r, d, fin, tr = env.step_final(torch.from_numpy(np.ascontiguousarray(acts[1].T)).cuda(), layout="soa")
    put("step_final", obs=o, rew=r, done=d, final=fin, trunc=tr)
    if ctrl:
        a, o, r, d = env.control_step()
        put("control_step", act=a, obs=o, rew=r, done=d)
        if env.frame_skip == 1:
            o, r, d, nxt = env.step_control(acts[2])
            put("step_control", obs=o, rew=r, done=d, next=nxt)
    i = 3
    for fused in (True, False):
        for mode, layout, dev in (("buffer", "aos", False), ("random", "soa", True), ("controller", "aos", False)):
            if mode == "controller" and not ctrl:
                continue
            a_in = acts[i:i + 3] if mode == "buffer" else None
            tr = env.rollout(3, mode=mode, actions=a_in, layout=layout, fused=fused, want=WANT, device_out=dev)
            put(f"rollout_{mode}_{int(fused)}", act=tr["actions"], obs=tr["obs"], rew=tr["rew"], done=tr["done"])
    out["state"], out["sbd"], out["rc"] = env.get_state(), env.get_sbd(), env.get_reset_counts()
    out["t"] = np.array([env.step_count])
    out.update({"buf:" + k: v for k, v in env.episode_buffers().items()})
    return out


CONFIGS = {"plain": dict(), "limit": dict(max_episode_steps=H),
           "all": dict(max_episode_steps=H, frame_skip=2, randomize={"mass": (0.8, 1.2), "tether_length": (0.4, 0.6)}, reward=True)}


# (every feature at once at all four sizes, the smaller configurations at 63 and 130 envs)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,config", [(m, "all") for m in SIZES] + [(m, c) for m in (63, 130) for c in ("plain", "limit")])
def test_an_all_zero_spec_stores_the_bits_of_a_handle_without_a_disturbance(G, kind, n, config):
    outs = []
    for spec in (R.ZERO, None):
        kw = dict(CONFIGS[config])
        if kw.get("reward"):
            kw["reward"] = tracking(G)
        env = make(G, kind, n, spec, **kw)
        assert (env.disturbance is None) == (spec is None)
        if spec is not None:
            assert not host(env.disturbance_now()).view(np.uint32).any(), "d = +0"
        outs.append(run_ops(G, env, kind, n))
        env.close()
    assert set(outs[0]) == set(outs[1])
    for key in outs[0]:
        same(outs[0][key], outs[1][key], f"{config}: {key}")
    done = np.concatenate([outs[0][key].ravel() for key in outs[0] if key.startswith("done:")])
    assert done.any() or config == "plain"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_a_constant_wind_is_a_handle_with_that_gravity(G, kind, n):
    """lo == hi == c, no gust: the bits of a plain handle whose g_vec is the kernel's own sum - float32(g) + float32(c) for the fp32
    kinds, the fp64 sum for the slung-load kinds - on caller and random actions (the controller reads g_vec and must NOT see c)."""
    c = (0.375, -0.625, 1.25)
    spec = dict(wind_lo=c, wind_hi=c, gust=(0.0, 0.0, 0.0), gust_hold=5)
    dim = R.DIM[kind]
    outs = []
    for disturbed in (True, False):
        env = make(G, kind, n, spec if disturbed else None, max_episode_steps=H)
        if not disturbed:
            p = env.params
            for i in range(dim):
                p.g_vec[i] = float(F32(p.g_vec[i]) + F32(c[i])) if kind in ("quad2d", "quad3d") else float(p.g_vec[i]) + float(F32(c[i]))
            env.params = p
        else:
            d = host(env.disturbance_now())
            same(d, np.repeat(np.array(c[:dim] + (0.0,) * (3 - dim), F32)[:, None], n, axis=1), "d = c")
        outs.append(run_ops(G, env, kind, n, ctrl=False))
        env.close()
    for key in outs[0]:
        same(outs[0][key], outs[1][key], key)
    # ... and it is not the still-air handle
    env = make(G, kind, n, None, max_episode_steps=H)
    still = run_ops(G, env, kind, n, ctrl=False)
    env.close()
    assert (still["obs:step"] != outs[0]["obs:step"]).any()


# ---- 4. / 5. / 2. the policy rollouts ----------------------------------------------------------------------------------------------------------
ACTORS = ("fp32_mfma", "f16", "f16_shared")


def policy_of(env, actor, norm):
    import torch
    from gym_reinmav_amd.obs_norm import RunningObsNorm
    from gym_reinmav_amd.ppo import MlpPolicy

    torch.manual_seed(2)
    on = None
    if norm:
        on = RunningObsNorm(env.nS, f"cuda:{env.device}", clip=2.0)
        on.update(torch.randn(64, env.nS, env.num_envs, device="cuda") * 1.7 + 0.4, env=env)
    pol = MlpPolicy(env.nS, env.nA, init_logstd=-0.5, value_network="shared" if actor == "f16_shared" else "copy", obs_norm=on).cuda()
    with torch.no_grad():
        pol.vf[-1].bias.uniform_(-0.5, 0.5)
    return pol


def collect(env, actor, steps, norm=False, **kw):
    """One fused policy rollout of `steps` agent steps -> every array the launch leaves, and the handle's state behind it."""
    import torch
    from gym_reinmav_amd.ppo import FusedPolicyCollector

    limited = env.max_episode_steps is not None
    col = FusedPolicyCollector(env, policy_of(env, actor, norm), steps, f16_mfma=(actor == "f16"), bootstrap_truncated=limited, **kw)
    col.collect()
    torch.cuda.synchronize()
    out = {key: getattr(col, key).cpu().numpy() for key in ("act", "obs", "rew", "done", "logp", "val")}
    if limited:
        out.update(boot=col.boot.cpu().numpy(), trunc=col.trunc.cpu().numpy())
    out.update(state=env.get_state(), sbd=env.get_sbd(), rc=env.get_reset_counts(), t=np.array([env.step_count]))
    return out


# the actors' kernel choices: without statistics and without a limit, with both (the *_boot tiles), and with every other feature on top
POLICY_CONFIGS = {"plain": (dict(), False), "norm_boot": (dict(max_episode_steps=H), True),
                  "all": (dict(max_episode_steps=H, frame_skip=2, randomize={"mass": (0.8, 1.2), "tether_length": (0.4, 0.6)}, reward=True), True)}


@pytest.mark.parametrize("actor", ACTORS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,config", [(m, "all") for m in SIZES] + [(65, "plain"), (130, "norm_boot")])
def test_an_all_zero_spec_stores_the_bits_of_the_undisturbed_policy_rollout(G, actor, kind, n, config):
    outs = []
    for spec in (R.ZERO, None):
        kw, norm = POLICY_CONFIGS[config]
        kw = dict(kw)
        if kw.get("reward"):
            kw["reward"] = tracking(G)
        env = make(G, kind, n, spec, **kw)
        outs.append(collect(env, actor, T, norm, clip_actions=(-0.5, 0.5) if config == "all" else None))
        env.close()
    for key in outs[0]:
        same(outs[0][key], outs[1][key], f"{actor} {config}: {key}")
    assert outs[0]["done"].any() or config == "plain"


@pytest.mark.parametrize("actor", ACTORS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_a_constant_wind_is_that_gravity_in_the_policy_kernels(G, actor, kind, n):
    """As test_a_constant_wind_is_a_handle_with_that_gravity, for the three actors: d enters the policy kernels exactly where gravity does."""
    c = (0.375, -0.625, 1.25)
    spec = dict(wind_lo=c, wind_hi=c, gust=(0.0, 0.0, 0.0), gust_hold=5)
    outs = []
    for disturbed in (True, False, None):
        env = make(G, kind, n, spec if disturbed else None, max_episode_steps=H)
        if disturbed is False:
            p = env.params
            for i in range(R.DIM[kind]):
                p.g_vec[i] = float(F32(p.g_vec[i]) + F32(c[i])) if kind in ("quad2d", "quad3d") else float(p.g_vec[i]) + float(F32(c[i]))
            env.params = p
        outs.append(collect(env, actor, T))
        env.close()
    for key in outs[0]:
        same(outs[0][key], outs[1][key], f"{actor}: {key}")
    assert outs[0]["done"].any() and (outs[0]["obs"][1] != outs[2]["obs"][1]).any(), "resets happen, and it is not the still-air handle"


@pytest.mark.parametrize("actor", ACTORS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", (65, 130))
def test_policy_rollouts_follow_the_oracle_with_the_disturbed_gravity(G, actor, kind, n):
    """Wind redraws and gust blocks inside a policy launch: every lane that goes on (the collector keeps no terminal observation) is
    step_ref from the stored observation and action under d of (running reset index, step counter) - the index moves with `done`."""
    env = make(G, kind, n, max_episode_steps=H)
    p = set_tether(env, kind, "walk")
    rc, t0 = env.get_reset_counts().astype(np.int64), env.step_count
    tr = collect(env, actor, T)
    env.close()
    moved, checked_after_reset = 0.0, 0
    for k in range(T):
        d = R.disturbance_now(R.SPEC, kind, SEED, BASE + np.arange(n), rc, t0 + k)
        go = ~tr["done"][k].astype(bool)
        if not go.any():   # (the step at which the time limit ends every episode)
            rc = rc + 1
            continue
        s_pre = np.ascontiguousarray(tr["obs"][k].T)[go]
        u = np.ascontiguousarray(tr["act"][k].T)[go]
        post = np.ascontiguousarray(tr["obs"][k + 1].T)[go]
        none = np.full(int(go.sum()), -1, np.int32)
        ref = check_step(kind, p, s_pre, u, none, d[:, go], post, tr["rew"][k][go], np.zeros(int(go.sum()), bool), f"{actor} n={n} step {k}")
        still, *_ = R.step_ref(kind, s_pre, u, none, p, np.zeros_like(d[:, go]))
        moved = max(moved, float(scaled_err(ref, still).max()))
        checked_after_reset += int((go & (rc > 1)).sum())
        rc = rc + tr["done"][k].astype(np.int64)
    assert np.array_equal(rc, tr["rc"]) and tr["trunc"].sum() >= n and checked_after_reset >= n and moved > 1e-5


@pytest.mark.parametrize("actor", ACTORS)
def test_a_set_between_two_policy_rollouts_is_ordered_on_the_stream(G, actor):
    """The policy kernels read the handle's device copy of the spec, which rmav_set_disturbance rewrites with a launch of its own: set A,
    rollout, set B, rollout, nothing synchronised in between - the first rollout has A's observations, the second B's."""
    import torch
    from gym_reinmav_amd.ppo import FusedPolicyCollector

    kind, n = "quad3d", 130
    spec_b = dict(R.SPEC, wind_lo=(0.5, 0.5, -1.0), wind_hi=(1.5, 0.75, -0.5), gust=(0.0, 0.25, 0.5), gust_hold=2)

    def run(first, second):
        env = make(G, kind, n, first)
        col = FusedPolicyCollector(env, policy_of(env, actor, False), 4, f16_mfma=(actor == "f16"))
        col.collect()
        o1 = col.obs.clone()
        col.roll_over()
        env.disturbance = dist(G, second)
        col.collect()
        o2 = col.obs.clone()
        torch.cuda.synchronize()
        env.close()
        return o1.cpu().numpy(), o2.cpu().numpy()

    a1, a2 = run(R.SPEC, R.SPEC)
    b1, _ = run(spec_b, spec_b)
    m1, m2 = run(R.SPEC, spec_b)
    same(m1, a1, "the rollout before the set keeps the first spec")
    assert (a1 != b1).any() and (m2 != a2).any(), "the rollout after the set has the second"


# ---- 6. the controller does not know the wind ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_the_controller_keeps_the_undisturbed_gravity(G, kind, n):
    env = make(G, kind, n, auto_reset=False)
    p = set_tether(env, kind, "walk")   # (a controller-driven slung load is taut, and every step behind a taut one starts on the tether edge)
    plain = make(G, kind, n, None, auto_reset=False)
    same(env.control(), plain.control(), "rmav_control does not depend on the spec")
    plain.close()

    def check(tag, s_pre, sbd, d, act, obs, rew, done):
        assert scaled_err(act, O.batch_control(kind, s_pre.astype(np.float64), params=p)).max() <= CTRL_TOL, tag
        check_step(kind, p, s_pre, act, sbd, d, obs, rew, done, tag)

    for j in range(2):
        s_pre, sbd, d = env.get_state(), env.get_sbd(), now_ref(env, kind, R.SPEC)
        a, o, r, dn = env.control_step()
        check(f"n={n} control_step {j}", s_pre, sbd, d, a, o, r, dn)
    s_pre, sbd, d = env.get_state(), env.get_sbd(), now_ref(env, kind, R.SPEC)
    o, r, dn, nxt = env.step_control(a)
    check_step(kind, p, s_pre, a, sbd, d, o, r, dn, f"n={n} step_control")
    assert scaled_err(nxt, O.batch_control(kind, o.astype(np.float64), params=p)).max() <= CTRL_TOL, "the trailing control()"
    env.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fused", (True, False))
def test_controller_rollouts_follow_the_oracle(G, kind, fused):
    n, steps = 65, 4
    env = make(G, kind, n, auto_reset=False)
    p = set_tether(env, kind, "walk")
    prev, sbd = env.get_state(), env.get_sbd()
    rc, t0 = env.get_reset_counts(), env.step_count
    tr = env.rollout(steps, mode="controller", layout="aos", fused=fused, want=WANT)
    for k in range(steps):
        d = R.disturbance_now(R.SPEC, kind, SEED, BASE + np.arange(n), rc, t0 + k)
        assert scaled_err(tr["actions"][k], O.batch_control(kind, prev.astype(np.float64), params=p)).max() <= CTRL_TOL, k
        check_step(kind, p, prev, tr["actions"][k], sbd, d, tr["obs"][k], tr["rew"][k], tr["done"][k].astype(bool), f"controller rollout step {k}")
        sbd = np.where(tr["done"][k].astype(bool), np.where(sbd < 0, 0, sbd + 1), sbd).astype(np.int32)
        prev = tr["obs"][k]
    env.close()


# ---- 7. API ------------------------------------------------------------------------------------------------------------------------------------
def test_round_trip_and_refusals(G):
    import ctypes as C

    import torch
    from gym_reinmav_amd import _abi as A
    from gym_reinmav_amd.ppo import FusedPolicyCollector, MlpPolicy

    L = A.lib()
    env = G.BatchedQuadrotor("quad3d", 65)
    s, on = A.DisturbanceSpec(), C.c_int32(7)
    assert L.rmav_get_disturbance(env._h, C.byref(s), C.byref(on)) == 0 and on.value == 0 and s.gust_hold == 0
    assert L.rmav_get_disturbance(env._h, None, None) == 0 and env.disturbance is None
    out = torch.zeros((3, 65), device="cuda")
    assert L.rmav_disturbance_now(env._h, out.data_ptr(), A.DEVICE) == A.ERR_INVALID and b"no disturbance" in L.rmav_last_error()
    env.disturbance = dist(G, R.SPEC)
    got = env.disturbance
    assert got.wind == tuple(zip(R.SPEC["wind_lo"], R.SPEC["wind_hi"])) and got.gust == R.SPEC["gust"] and got.hold == 3
    hostbuf = np.zeros((3, 65), F32)
    A.check(L.rmav_disturbance_now(env._h, hostbuf.ctypes.data_as(C.c_void_p), A.HOST))
    same(hostbuf, env.disturbance_now(), "host and device pointers")

    def spec(**kw):
        q = dist(G, R.SPEC).spec(A.QUAD3D)
        for k, (i, v) in kw.items():
            if i is None:
                setattr(q, k, v)
            else:
                getattr(q, k)[i] = v
        return q

    for bad in (dict(wind_lo=(0, float("nan"))), dict(wind_hi=(1, float("inf"))), dict(gust=(2, float("nan"))), dict(gust=(0, -0.5)),
                dict(wind_lo=(1, 5.0)), dict(gust_hold=(None, 0)), dict(gust_hold=(None, 1048577)), dict(gust_hold=(None, -3)),
                dict(wind_lo=(0, -3e38), wind_hi=(0, 3e38)), dict(gust=(1, 3e38))):
        assert L.rmav_set_disturbance(env._h, C.byref(spec(**bad))) == A.ERR_INVALID, bad
        assert len(L.rmav_last_error()) > 0
    assert env.disturbance.hold == 3, "a refused spec leaves the one in force"
    assert L.rmav_set_disturbance(env._h, C.byref(spec(gust_hold=(None, 1048576)))) == 0 and env.disturbance.hold == 1048576
    # the fp32 vector-ALU and bf16 actors have no disturbed kernel: the collector and the library refuse them, and only them
    with pytest.raises(ValueError, match="disturbed kernel"):
        FusedPolicyCollector(env, MlpPolicy(env.nS, env.nA).cuda(), 4, f32_mfma=False)
    with pytest.raises(ValueError, match="disturbed kernel"):
        FusedPolicyCollector(env, MlpPolicy(env.nS, env.nA).cuda(), 4, bf16_mfma=True)
    pol = MlpPolicy(env.nS, env.nA).cuda()
    n, steps = 65, 2
    f = lambda *shape: torch.zeros(shape, device="cuda")   # noqa: E731
    args = [x.data_ptr() for x in (f(1 << 16), f(steps, 4, n), f(steps, 10, n), f(steps, n), torch.zeros(steps, n, dtype=torch.uint8, device="cuda"),
                                   f(steps, n), f(steps + 1, n))]
    for precision in (A.POLICY_FP32, A.POLICY_BF16_MFMA):
        assert L.rmav_rollout_policy(env._h, steps, *args, precision) == A.ERR_INVALID
        assert b"disturbance" in L.rmav_last_error()
    for precision in (A.POLICY_FP32_MFMA, A.POLICY_F16_MFMA, A.POLICY_F16_SHARED):
        assert L.rmav_rollout_policy(env._h, steps, *args, precision) == 0, L.rmav_last_error()
    FusedPolicyCollector(env, pol, 4)
    env.disturbance = None
    assert env.disturbance is None and L.rmav_get_disturbance(env._h, C.byref(s), None) == 0 and s.gust_hold == 1048576
    FusedPolicyCollector(env, pol, 4)
    torch.cuda.synchronize()
    env.close()
    # RMAV_REINMAV takes no spec; NULL is accepted
    h = C.c_void_p()
    pr = A.default_params(A.REINMAV)
    A.check(L.rmav_create(C.byref(h), A.REINMAV, 4, 0, 0, 0, 0, C.byref(pr), None))
    assert L.rmav_set_disturbance(h, C.byref(spec())) == A.ERR_INVALID and len(L.rmav_last_error()) > 0
    assert L.rmav_set_disturbance(h, None) == 0
    L.rmav_destroy(h)
    # the keyword reaches every constructor
    venv = G.QuadrotorVecEnv("quadrotor3d-v0", 4, disturbance=dist(G, R.SPEC))
    assert venv.env.disturbance.hold == 3
    e1 = G.make("quadrotor2d-v0", disturbance=G.Disturbance(wind=0.5, gust=0.1, hold=2))
    assert e1.disturbance.hold == 2 and e1.disturbance_now().shape == (3,)
    e1.step(e1.control())
    e1.close()


@pytest.mark.parametrize("kind", KINDS)
def test_null_restores_the_old_kernels_bits(G, kind):
    n = 130
    outs = []
    for touched in (True, False):
        env = make(G, kind, n, None, max_episode_steps=H)
        if touched:
            env.disturbance = dist(G, R.SPEC)
            env.disturbance = None
        outs.append(run_ops(G, env, kind, n))
        env.close()
    for key in outs[0]:
        same(outs[0][key], outs[1][key], "set back to NULL: " + key)
    # a set takes effect on the next launch; nothing is synchronised in between
    import torch

    env, ref = make(G, kind, n, None, auto_reset=False), make(G, kind, n, None, auto_reset=False)
    act = torch.from_numpy(R.parity_actions(kind, n)[0]).cuda()
    o1, *_ = env.step(act)
    env.disturbance = dist(G, R.SPEC)
    o2, *_ = env.step(act)
    p1, *_ = ref.step(act)
    p2, *_ = ref.step(act)
    torch.cuda.synchronize()
    same(o1, p1, "the launch before the set")
    assert (host(o2) != host(p2)).any(), "the launch after it"
    env.close()
    ref.close()

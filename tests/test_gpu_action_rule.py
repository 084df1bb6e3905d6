"""The action rule of the in-kernel policy rollouts (rmav_set_policy_action_rule) on the GPU: the identity leaves every bit, the dynamics
take the clipped action while the stored one stays the policy's, the deterministic launch stores the mean, the rule composes with the
time limit / bootstrap / observation normalisation / parameter ranges, the refusals, the per-step collector's same semantics, and
evaluate_policy.  N = 131 (two full 64-env pairs and a partial one; four full 32-env fp32-MFMA wavefronts and a partial one), T = 12."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest

import oracle as O
from test_gpu_ppo import ACTOR_TOL, _check_rollout, _predicted_noise
from util import BOX, TOL, near_threshold, random_cases, scaled_err

pytestmark = pytest.mark.gpu

ACTORS = ("fp32_mfma", "f16", "f16_shared")
VARIANTS = ("plain", "limit_boot", "obs_norm", "ranged", "ranged_limit")
N, T, H, SEED, BASE = 131, 12, 7, 21, 1000
INF = math.inf
MASS = (0.8, 1.25)


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available()
    import gym_reinmav_amd as g

    return g


def _env(G, kind, variant="plain", n=N, seed=SEED, base=BASE, wide=True):
    """A handle of the variant; `wide`: half of the states three times as wide (util.random_cases), so that episodes end inside T steps."""
    kw = {}
    if variant in ("limit_boot", "ranged_limit"):
        kw["max_episode_steps"] = H
    if variant in ("ranged", "ranged_limit"):
        kw["randomize"] = {"mass": MASS}
    env = G.BatchedQuadrotor(kind, n, seed=seed, env_id_base=base, **kw)
    if wide:
        env.set_state(random_cases(kind, n, seed=5)[0])
    return env


def _policy(env, actor, variant="plain", head=30.0, logstd=None, seed=2):
    """The policy of test_fused_policy_rollout_matches_torch_policy_and_oracle (action head x 30, non-trivial biases and logstd); the
    shared-trunk architecture for the f16_shared actor; `obs_norm`: statistics far from the identity."""
    import torch
    from gym_reinmav_amd.obs_norm import RunningObsNorm
    from gym_reinmav_amd.ppo import MlpPolicy

    torch.manual_seed(seed)
    on = None
    if variant == "obs_norm":
        on = RunningObsNorm(env.nS, f"cuda:{env.device}", clip=2.0)
        on.update(torch.randn(64, env.nS, env.num_envs, device="cuda") * 1.7 + 0.4, env=env)
    pol = MlpPolicy(env.nS, env.nA, init_logstd=0.7, value_network="shared" if actor == "f16_shared" else "copy", obs_norm=on).cuda()
    with torch.no_grad():
        pol.pi[2].weight.mul_(head)
        pol.pi[2].bias.uniform_(-0.5, 0.5)
        pol.vf[-1].bias.uniform_(-0.5, 0.5)
        pol.logstd.copy_(torch.linspace(-0.5, 0.7, env.nA) if logstd is None else torch.full((env.nA,), float(logstd)))
    return pol


def _collector(env, pol, actor, variant="plain", steps=T, **kw):
    from gym_reinmav_amd.ppo import FusedPolicyCollector

    return FusedPolicyCollector(env, pol, steps, f16_mfma=(actor == "f16"), bootstrap_truncated=(variant == "limit_boot"), **kw)


def _outputs(col, env):
    """Every array the launch wrote and everything it left in the handle, as host arrays."""
    import torch

    torch.cuda.synchronize()
    out = {k: getattr(col, k).cpu().numpy() for k in ("act", "obs", "rew", "done", "logp", "val")}
    if col.boot is not None:
        out.update(boot=col.boot.cpu().numpy(), trunc=col.trunc.cpu().numpy())
    eb = env.episode_buffers()
    out.update(state=env.get_state(), sbd=env.get_sbd(), rc=env.get_reset_counts(), tot=np.array(list(env.episode_totals().values()), np.float64),
               mass=env.get_env_param("mass"), last_trunc=env.episode_truncated(), **{"eb_" + k: np.asarray(v) for k, v in eb.items()})
    return out


def _same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)


# ---- 1. the identity leaves the bits ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("actor", ACTORS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_identity_rule_leaves_every_bit(G, actor, variant):
    """A handle that never set a rule, a twin with the identity set explicitly (launches the same kernels), and a third whose rule is
    NOT the identity but binds nowhere - clip (-3e38, 3e38): routed to the normalised kernels with identity tables and, on a
    time-limited handle without a bootstrap request, the handle's scratch boot_out - write the same bits and leave the same handle."""
    kind = "quad3d"
    outs = []
    for rule in (None, (False, (-INF, INF)), (False, (-3e38, 3e38))):
        env = _env(G, kind, variant)
        if rule is not None:
            env.set_policy_action_rule(*rule)
        col = _collector(env, _policy(env, actor, variant), actor, variant, clip_actions=rule[1] if rule else False)
        assert env.get_policy_action_rule() == (False, (-INF, INF) if rule is None else tuple(np.float32(v) for v in rule[1]))
        col.collect()
        outs.append(_outputs(col, env))
        env.close()
    assert outs[0]["done"].sum() > 10 and np.isfinite(outs[0]["act"]).all()
    if variant in ("limit_boot", "ranged_limit"):
        assert outs[0]["last_trunc"].sum() > 0
    _same_bits(outs[0], outs[1], "identity set explicitly")
    _same_bits(outs[0], outs[2], "a rule that binds nowhere")


# ---- 2. clipping -------------------------------------------------------------------------------------------------------------------
_noise = {}


def _noise_of(t0, nA):
    """[T, N, nA] unit Gaussians of the launch that starts at step t0, from the Philox / Box-Muller spec - computed once per t0."""
    if t0 not in _noise:
        _noise[t0] = np.stack([_predicted_noise(SEED, BASE + np.arange(N), t0 + t) for t in range(T)])
        _noise[t0].setflags(write=False)
    return _noise[t0][:, :, :nA]


def _torch_forward(pol, col):
    import torch

    nS, nA = col.obs.shape[1], col.act.shape[1]
    with torch.no_grad():
        mean, val = pol(col.obs[:T].permute(1, 0, 2).reshape(nS, -1))
    return mean.reshape(nA, T, N), val.reshape(T, N)


@pytest.mark.parametrize("actor", ACTORS)
@pytest.mark.parametrize("kind,clip", [("quad3d", True), ("quad2d_sl", (-1.0, 1.0))])
def test_dynamics_take_the_clipped_action_and_the_stored_one_stays_unclipped(G, kind, clip, actor):
    import torch

    lo, hi = BOX[kind] if clip is True else clip
    env = _env(G, kind, wide=False)
    pol = _policy(env, actor)
    col = _collector(env, pol, actor, clip_actions=clip)
    rc0, t0 = env.get_reset_counts(), env.step_count
    col.collect()
    torch.cuda.synchronize()
    assert env.get_policy_action_rule() == (False, (lo, hi))
    # the stored action is the torch policy's mean + std * z, z from the noise spec - at the tolerances of the tests without a rule
    mean, _ = _torch_forward(pol, col)
    std = torch.exp(pol.logstd.detach())[:, None, None]
    z = ((col.act.permute(1, 0, 2) - mean) / std).cpu().numpy().transpose(1, 2, 0)   # implied noise [T, N, nA]
    zp = _noise_of(t0, env.nA)
    ztol = 2e-4 * 30 if actor == "fp32_mfma" else ACTOR_TOL[actor] * max(1.0, float(mean.abs().max())) / float(std.min())
    print(f"{kind} {actor}: implied-noise error {np.abs(z - zp).max():.3g} (tolerance {ztol:.3g})")
    assert np.abs(z - zp).max() < ztol
    logp_ref = -0.5 * (zp.astype(np.float64) ** 2).sum(2) - float(pol.logstd.detach().sum()) - 0.5 * env.nA * np.log(2 * np.pi)
    assert np.abs(col.logp.cpu().numpy() - logp_ref).max() < 1e-3
    act = col.act.cpu().numpy()
    outside = ((act < lo) | (act > hi)).mean()
    print(f"stored components outside [{lo}, {hi}]: {outside:.3f}")
    assert outside >= 0.10
    # the env side: the oracle teacher-forced with the clipped action reproduces obs / rew / done (and the reset states) ...
    used = np.clip(act, np.float32(lo), np.float32(hi)).astype(np.float32)
    forced = SimpleNamespace(obs=col.obs, act=torch.from_numpy(used), rew=col.rew, done=col.done)
    rc = _check_rollout(kind, SEED, forced, rc0, BASE)
    assert np.array_equal(env.get_reset_counts(), rc)
    # ... and with the stored, unclipped action it does not
    obs, done = col.obs.cpu().numpy(), col.done.cpu().numpy().astype(bool)
    worst = 0.0
    for t in range(T):
        o2, _, d, _ = O.batch_step(kind, obs[t].T.astype(np.float64), act[t].T.astype(np.float64))
        live = ~done[t] & ~d & ~near_threshold(kind, o2)
        worst = max(worst, float(scaled_err(obs[t + 1].T[live], o2[live]).max()))
    print(f"unclipped teacher forcing: worst live error {worst:.3g}")
    assert worst > 100 * TOL
    env.close()


# ---- 3. deterministic --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("actor", ACTORS)
def test_deterministic_launch_stores_the_mean(G, actor):
    import torch

    kind = "quad3d"
    runs = []
    for logstd in (-0.5, 1.0):
        env = _env(G, kind, wide=False)
        pol = _policy(env, actor, logstd=logstd)
        col = _collector(env, pol, actor, deterministic=True)
        col.collect()
        torch.cuda.synchronize()
        assert env.get_policy_action_rule() == (True, (-INF, INF))
        mean, val = _torch_forward(pol, col)
        tol = 2e-5 if actor == "fp32_mfma" else ACTOR_TOL[actor]
        err = float((col.act.permute(1, 0, 2) - mean).abs().max())
        print(f"{actor} logstd {logstd}: |act - mean| {err:.3g} (tolerance {tol * max(1.0, float(mean.abs().max())):.3g})")
        assert err < tol * max(1.0, float(mean.abs().max()))
        assert float((col.val[:T] - val).abs().max()) < tol * max(1.0, float(val.abs().max()))
        logp0 = -env.nA * logstd - 0.5 * env.nA * math.log(2 * math.pi)
        assert float((col.logp.double() - logp0).abs().max()) <= 1e-6 * abs(logp0)
        runs.append((col.act.cpu().numpy(), col.obs.cpu().numpy()))
        env.close()
    # policies that differ only in logstd: the same bits
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()


# ---- 4. the rule on, across the variants -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("actor", ACTORS)
@pytest.mark.parametrize("variant", VARIANTS[1:])
def test_rule_composes_with_limit_bootstrap_normalisation_and_ranges(G, actor, variant):
    """deterministic + clipped to the action space on a handle with a time limit (+ bootstrap), normalised observations, a ranged mass,
    a ranged mass and a limit: the stored actions, clipped on the host and replayed as caller actions (rollout(mode='buffer')) on a twin
    handle with the same seed, env-id base, states, limit and range, give bit-identical obs / rew / done and reset counts.

    Bit identity, not util.TOL, is what is asserted: the caller-action kernels and the actors' kernels run the same Env<K>::step from the
    same fp32 state and action in an uncontracted build, and the reset draws depend on (seed, env id, reset index) alone.  That the
    replay is bit-identical with the rule OFF on the parent commit has been argued from the code, NOT yet established by a run: if a
    rule-off replay differs there, this test's fallback is util.TOL on live envs, and this docstring has to say which one held."""
    import torch

    kind = "quad3d"
    lo, hi = BOX[kind]
    env, twin = _env(G, kind, variant), _env(G, kind, variant)
    col = _collector(env, _policy(env, actor, variant), actor, variant, deterministic=True, clip_actions=True)
    col.collect()
    torch.cuda.synchronize()
    act = col.act.cpu().numpy()
    assert ((act < lo) | (act > hi)).mean() >= 0.10
    tr = twin.rollout(T, mode="buffer", actions=np.clip(act, np.float32(lo), np.float32(hi)), layout="soa", want=("obs", "rew", "done"))
    got = dict(obs=col.obs[1:].cpu().numpy(), rew=col.rew.cpu().numpy(), done=col.done.cpu().numpy(), rc=env.get_reset_counts(),
               state=env.get_state(), mass=env.get_env_param("mass"))
    ref = dict(obs=tr["obs"], rew=tr["rew"], done=tr["done"], rc=twin.get_reset_counts(), state=twin.get_state(), mass=twin.get_env_param("mass"))
    _same_bits(got, ref, (variant, actor))
    assert got["done"].sum() > 10
    if variant == "limit_boot":
        trunc = col.trunc.cpu().numpy().astype(bool)
        assert trunc.sum() > 0 and (col.boot.cpu().numpy()[~trunc] == 0).all() and np.isfinite(col.boot.cpu().numpy()).all()
    env.close()
    twin.close()


# ---- 5. routing and refusals ---------------------------------------------------------------------------------------------------------
def test_routing_and_refusals(G):
    import torch
    from gym_reinmav_amd import _abi as A
    from gym_reinmav_amd.ppo import FusedPolicyCollector

    L = A.lib()
    env = _env(G, "quad3d")
    # set / get, and what set refuses (the rule in force stays)
    d, lo, hi = C.c_int32(), C.c_float(), C.c_float()
    get = lambda h: (A.check(L.rmav_get_policy_action_rule(h, C.byref(d), C.byref(lo), C.byref(hi))), (d.value, lo.value, hi.value))[1]  # noqa: E731
    assert get(env._h) == (0, -INF, INF)
    A.check(L.rmav_set_policy_action_rule(env._h, 1, -2.5, 7.0))
    assert get(env._h) == (1, -2.5, 7.0)
    for bad in ((0, 1.0, 0.5), (0, float("nan"), 1.0), (0, 0.0, float("nan")), (2, 0.0, 1.0), (-1, 0.0, 1.0)):
        assert L.rmav_set_policy_action_rule(env._h, *bad) == A.ERR_INVALID, bad
        assert b"clip_lo" in L.rmav_last_error() or b"deterministic" in L.rmav_last_error()
    assert get(env._h) == (1, -2.5, 7.0)
    A.check(L.rmav_set_policy_action_rule(env._h, 0, 3.0, 3.0))   # lo == hi and infinite bounds are rules
    A.check(L.rmav_set_policy_action_rule(env._h, 0, -INF, 0.0))
    assert L.rmav_get_policy_action_rule(env._h, None, C.byref(lo), C.byref(hi)) == A.ERR_INVALID
    assert env.get_policy_action_rule() == (False, (-INF, 0.0))
    # a rule + an actor without the kernels: RMAV_ERR_INVALID naming the rule; with the identity the same call runs
    pol = _policy(env, "fp32_mfma")
    dev = torch.device("cuda", env.device)
    buf = lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device=dev)  # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rew, done, logp, val = buf(T, N), buf(T, N, dt=torch.uint8), buf(T, N), buf(T + 1, N)
    for kw, prec in ((dict(f32_mfma=False), A.POLICY_FP32), (dict(bf16_mfma=True), A.POLICY_BF16_MFMA)):
        col = FusedPolicyCollector(env, pol, T, **kw)
        col._pack()
        call = lambda: L.rmav_rollout_policy(env._h, T, p(col.weights), None, None, p(rew), p(done), p(logp), p(val), prec)  # noqa: E731
        env.set_policy_action_rule(True)
        t0 = env.step_count
        assert call() == A.ERR_INVALID and b"action rule" in L.rmav_last_error(), L.rmav_last_error()
        assert env.step_count == t0
        env.set_policy_action_rule(False, None)
        A.check(call())
        for bad in (dict(deterministic=True), dict(clip_actions=True), dict(clip_actions=(-1.0, 1.0))):
            with pytest.raises(ValueError, match="action-rule"):
                FusedPolicyCollector(env, pol, T, **kw, **bad)
    torch.cuda.synchronize()
    env.close()
    r = G.BatchedQuadrotor("reinmav", 64)
    rp = _policy(r, "f16")
    col = FusedPolicyCollector(r, rp, T, f16_mfma=True)
    col._pack()
    r.set_policy_action_rule(False, (-1.0, 1.0))
    rew, done, logp, val = buf(T, 64), buf(T, 64, dt=torch.uint8), buf(T, 64), buf(T + 1, 64)
    assert L.rmav_rollout_policy(r._h, T, p(col.weights), None, None, p(rew), p(done), p(logp), p(val), A.POLICY_F16_MFMA) == A.ERR_INVALID
    assert b"action rule" in L.rmav_last_error()
    r.set_policy_action_rule()
    A.check(L.rmav_rollout_policy(r._h, T, p(col.weights), None, None, p(rew), p(done), p(logp), p(val), A.POLICY_F16_MFMA))
    torch.cuda.synchronize()
    r.close()


def test_the_rule_touches_the_policy_rollouts_only(G):
    """rmav_step and the caller-, random- and controller-action rollouts of a handle with a rule are those of a handle without."""
    kind, outs = "quad3d", []
    for ruled in (False, True):
        env = _env(G, kind, "ranged_limit")
        if ruled:
            env.set_policy_action_rule(True, (1.0, 2.0))
        a = np.random.RandomState(3).uniform(-5, 15, (T, N, env.nA)).astype(np.float32)
        o = {}
        for mode in ("random", "controller", "buffer"):
            tr = env.rollout(T, mode=mode, actions=a if mode == "buffer" else None, layout="aos", want=("actions", "obs", "rew", "done"))
            o.update({f"{mode}_{k}": v for k, v in tr.items()})
        o["step_obs"], o["step_rew"], o["step_done"] = env.step(a[0])
        o["state"], o["rc"] = env.get_state(), env.get_reset_counts()
        outs.append(o)
        env.close()
    _same_bits(outs[0], outs[1], "step / rollout")


# ---- 6. the collectors agree -------------------------------------------------------------------------------------------------------
def test_per_step_collector_has_the_same_semantics(G):
    """RolloutCollector(deterministic=True, clip_actions=True) - eager and graph-captured: the same bits - against FusedPolicyCollector
    with the same arguments from the same state: actions and values within the fp32 actor's tolerance while an env's first episode runs."""
    import torch
    from gym_reinmav_amd.ppo import RolloutCollector

    kind, n, steps = "quad3d", 256, 8
    lo, hi = BOX[kind]
    cols, envs = [], []
    for which in ("fused", "eager", "graph"):
        env = _env(G, kind, n=n)
        rc0 = env.get_reset_counts()
        pol = _policy(env, "fp32_mfma")
        if which == "fused":
            col = _collector(env, pol, "fp32_mfma", steps=steps, deterministic=True, clip_actions=True)
        else:
            col = RolloutCollector(env, pol, steps, graph=(which == "graph"), deterministic=True, clip_actions=True)
        col.collect()
        torch.cuda.synchronize()
        cols.append(col)
        envs.append(env)
    fused, eager, graph = cols
    for k in ("act", "obs", "rew", "done", "logp", "val"):
        assert torch.equal(getattr(eager, k), getattr(graph, k)), k
    assert np.array_equal(envs[1].get_state(), envs[2].get_state()) and np.array_equal(envs[1].get_reset_counts(), envs[2].get_reset_counts())
    act = eager.act.cpu().numpy()
    assert ((act < lo) | (act > hi)).mean() >= 0.10
    # the env was stepped with the clipped action: the oracle agrees (teacher-forced, _check_rollout's rule)
    forced = SimpleNamespace(obs=eager.obs, act=torch.clamp(eager.act, lo, hi), rew=eager.rew, done=eager.done)
    _check_rollout(kind, SEED, forced, rc0, BASE)
    logp0 = float(-eager.policy.logstd.detach().double().sum()) - 0.5 * envs[1].nA * math.log(2 * math.pi)
    assert float((eager.logp - logp0).abs().max()) <= 1e-6 * abs(logp0) and float((fused.logp - logp0).abs().max()) <= 1e-6 * abs(logp0)
    # envs with no done so far (in either): the trajectories have not been reset apart
    live = torch.ones(n, dtype=torch.bool, device=eager.act.device)
    n_cmp = 0
    for t in range(steps):
        sa = max(1.0, float(eager.act[t].abs().max()))
        sv = max(1.0, float(eager.val[t].abs().max()))
        ea = float((fused.act[t] - eager.act[t])[:, live].abs().max())
        ev = float((fused.val[t] - eager.val[t])[live].abs().max())
        print(f"t {t}: live {int(live.sum())}, |act| err {ea:.3g} / {2e-5 * sa:.3g}, |val| err {ev:.3g} / {2e-5 * sv:.3g}")
        assert ea < 2e-5 * sa and ev < 2e-5 * sv
        n_cmp += int(live.sum())
        live &= (fused.done[t] == 0) & (eager.done[t] == 0)
    assert n_cmp > steps * n // 4 and int(live.sum()) < n
    for e in envs:
        e.close()


# ---- 7. evaluate_policy ------------------------------------------------------------------------------------------------------------
def test_evaluate_policy(G):
    import torch
    from gym_reinmav_amd.evaluate import evaluate_policy, first_episode_stats

    kind, n, limit = "quad2d", 256, 32
    mk = lambda: G.BatchedQuadrotor(kind, n, seed=SEED, env_id_base=BASE, max_episode_steps=limit)  # noqa: E731
    env = mk()
    pol = _policy(env, "fp32_mfma", head=10.0)
    res = evaluate_policy(pol, env)
    assert env.get_policy_action_rule() == (True, BOX[kind])
    assert res["episodes"] == n and res["unfinished"] == 0 and bool(res["finished"].all())
    assert int(res["lengths"].max()) <= limit and int(res["lengths"].min()) >= 1
    # = first_episode_stats of a hand-run rollout of `limit` steps on an identically seeded env
    hand = mk()
    hand.reset()
    col = _collector(hand, pol, "fp32_mfma", steps=limit, deterministic=True, clip_actions=True)
    col.collect()
    torch.cuda.synchronize()
    ret, ln, fin = first_episode_stats(col.rew, col.done)
    assert torch.equal(ret, res["returns"]) and torch.equal(ln, res["lengths"]) and torch.equal(fin, res["finished"])
    assert res["mean_return"] == float(ret.double().mean()) and res["mean_length"] == float(ln.double().mean())
    assert res["std_return"] == float(ret.double().std(unbiased=False)) and res["std_return"] > 0
    assert int(ln.min()) < limit   # some episode terminated on its own
    # ... and of the env's own episode statistics: the first finished episode of every env that finished exactly one
    eb, once = hand.episode_buffers(), (col.done != 0).sum(0).cpu().numpy() == 1
    assert once.sum() > 0 and np.array_equal(np.asarray(eb["last_return"])[once], ret.cpu().numpy()[once])
    # fresh identically seeded envs: identical bits, whatever the chunk; other actors run
    for kw in (dict(), dict(chunk=5), dict(chunk=64, n_steps=limit)):
        e2 = mk()
        r2 = evaluate_policy(pol, e2, **kw)
        assert all(torch.equal(r2[k], res[k]) for k in ("returns", "lengths", "finished")), kw
        assert all(r2[k] == res[k] for k in ("mean_return", "std_return", "mean_length", "episodes", "unfinished")), kw
        e2.close()
    e3 = mk()
    r3 = evaluate_policy(pol, e3, f16_mfma=True, n_steps=7, chunk=4)
    assert r3["episodes"] + r3["unfinished"] == n and r3["unfinished"] > 0 and int(r3["lengths"].max()) == 7
    e3.close()
    # the statistics of a policy's obs_norm are read, never written
    npol = _policy(env, "f16_shared", "obs_norm", head=10.0)
    before = npol.obs_norm.buf.clone()
    r4 = evaluate_policy(npol, env)
    torch.cuda.synchronize()
    assert r4["episodes"] == n and before.cpu().numpy().tobytes() == npol.obs_norm.buf.cpu().numpy().tobytes()
    for e in (env, hand):
        e.close()

"""Sensor noise (rmav_set_sensor_noise) on the GPU.  The pillars: observe() is the contract's draw (the fp64 restatement
tests/sensor_ref.py, within its bound, at the edges of the step counter, with wide env ids and across shards); ONE rule - what an
operation emits has the bits of observe() called right after it - for every stepping entry point and launch grouping; the twin - a
handle with a spec leaves everything but observations bit-identical to one without, and every observation row inside the
restatement's bound around the twin's row; the reductions (an all-zero spec, a set-then-None handle, single zero components); the
policy rollouts of the three actors (a T-step launch is T one-step launches, the values are those of the stored noisy rows, the
dynamics ran from the true state, the bootstrap term is the value of the noisy terminal observation; the all-zero spec and the
set-then-None handle reduce to the plain kernels' bits); the moments of the device's draw; the API.

The bound inherits oracle/sample_ref.py's ASSUMED 2-ulp figures for logf, sqrtf and sincospif (see tests/sensor_ref.py)."""
import numpy as np
import pytest

import disturbance_ref as D
import sensor_ref as R
import test_gpu_bootstrap as TB
import test_gpu_disturbance as TD
from test_gpu_disturbance import CONFIGS, final, host, run_ops, same, same_run, tracking
from util import KINDS, NS

pytestmark = pytest.mark.gpu

SEED, BASE, H, T = D.PARITY["seed"], D.PARITY["env_id_base"], D.PARITY["limit"], D.PARITY["steps"]
SIZES = (1, 63, 65, 130)
SIGMA = 0.25
WIDE_BASE = 2**40 + 12345
WANT = ("actions", "obs", "rew", "done")
F32 = np.float32


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available()
    import gym_reinmav_amd as g

    return g


def make(G, kind, n, sigma=SIGMA, base=BASE, seed=SEED, **kw):
    """A handle with the tests' seed and env ids; sigma: a scalar or nS values, None = a handle without sensor noise."""
    if kw.get("reward") is True:
        kw["reward"] = tracking(G)
    return G.BatchedQuadrotor(kind, n, seed=seed, env_id_base=base, sensor_noise=None if sigma is None else G.SensorNoise(sigma), **kw)


def sig(kind, sigma=SIGMA):
    return np.full(NS[kind], sigma) if np.isscalar(sigma) else np.asarray(sigma, np.float64)


def rows(x, nS):
    """[..., n, nS] whatever the layout."""
    x = host(x)
    return x if x.shape[-1] == nS and x.shape[-2:] != (nS, nS) else np.swapaxes(x, -1, -2)


def inside(o, s, kind, ids, b, what, sigma=SIGMA, seed=SEED, mask=None):
    """The observation rows o [n, nS] of the true states s [n, nS] at the step counter b lie inside the restatement's bound."""
    ref, bound = R.o_ref(sig(kind, sigma), seed, ids, b, np.ascontiguousarray(s, F32))
    err = np.abs(o.astype(np.float64) - ref) / bound
    if mask is not None:
        err = err[mask]
    assert err.size == 0 or err.max() <= 1.0, (what, b, float(err.max()))


# ---- 1. observe() --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_observe_is_the_restatement(G, kind, n):
    for base in (BASE, WIDE_BASE):
        env = make(G, kind, n, base=base)
        ids = base + np.arange(n)
        s = env.get_state()
        inside(env.observe(), s, kind, ids, 0, "fresh")
        same(env.observe(layout="soa", device_out=True).T.contiguous(), env.observe(), "layouts and mem")
        acts = D.parity_actions(kind, n)
        for t in range(3):
            env.step(acts[t])
        s = env.get_state()
        assert env.step_count == 3
        inside(env.observe(), s, kind, ids, 3, "after steps")
        assert np.abs(env.observe() - s).max() > 0.01, "noise is there"
        for b in (2**32 - 1, 2**32 + 1, 3 * 2**32, 2**48 - 2):
            env.step_count = b
            same(env.get_state(), s, "the step counter moves no state")
            inside(env.observe(), s, kind, ids, b, "late step counters")
        env.close()


@pytest.mark.parametrize("kind", KINDS)
def test_two_shards_equal_the_whole(G, kind):
    n, k = 130, 63
    outs = []
    for first, count in ((0, n), (0, k), (k, n - k)):
        env = make(G, kind, count, base=WIDE_BASE + first, max_episode_steps=H)
        fresh = env.observe()
        tr = env.rollout(T, mode="random", layout="aos", want=WANT)
        outs.append((fresh, host(tr["obs"]), env.observe()))
        env.close()
    for i in range(3):
        axis = 1 if i == 1 else 0
        same(outs[0][i], np.concatenate([outs[1][i], outs[2][i]], axis=axis), f"shards {i}")


# ---- 2. the one rule ---------------------------------------------------------------------------------------------------------------------------
ONE_RULE = {"plain": dict(), "all": CONFIGS["all"]}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,config", [(m, "plain") for m in SIZES] + [(63, "all"), (130, "all")])
def test_every_operation_emits_the_bits_of_observe(G, kind, n, config):
    import torch

    env = make(G, kind, n, **ONE_RULE[config])
    nS = NS[kind]
    acts = D.parity_actions(kind, n)

    def rule(obs, what):
        same(rows(obs, nS) if host(obs).ndim == 2 else rows(obs, nS)[-1], env.observe(), f"{config}: {what}")

    rule(env.reset(), "reset")
    rule(env.reset(layout="soa", device_out=True), "reset, feature-major on the device")
    rule(env.step(acts[0])[0], "step")
    rule(env.step(torch.from_numpy(np.ascontiguousarray(acts[1].T)).cuda(), layout="soa")[0], "step, feature-major on the device")
    rule(env.step_final(acts[2])[0], "step_final")
    rule(env.control_step()[1], "control_step")
    if env.frame_skip == 1:
        rule(env.step_control(acts[3])[0], "step_control")
    for mode in ("buffer", "random", "controller"):
        for fused in (True, False):
            for layout in ("aos", "soa"):
                a_in = None
                if mode == "buffer":
                    a_in = acts[:3] if layout == "aos" else np.ascontiguousarray(acts[:3].transpose(0, 2, 1))
                tr = env.rollout(3, mode=mode, actions=a_in, layout=layout, fused=fused, want=WANT, device_out=layout == "soa")
                rule(tr["obs"], f"rollout {mode} fused={fused} {layout}")
        tr = env.rollout(1, mode=mode, actions=None if mode != "buffer" else acts[4:5], layout="aos", want=WANT)
        rule(tr["obs"], f"single-step rollout {mode}")
        if mode != "buffer":
            ch = env.rollout_chunked(3, mode=mode, chunk=64, want=WANT)
            rule(env.unchunk(ch["obs"]), f"chunk-major {mode}")
    rule(env.reset(), "reset after steps")
    assert env.step_count > 0
    env.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,config", [(m, "limit") for m in SIZES] + [(63, "all"), (130, "all")])
def test_fused_rollouts_equal_single_steps(G, kind, n, config):
    acts = D.parity_actions(kind, n)[:T]

    def fresh():
        return make(G, kind, n, **CONFIGS[config])

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
        soa = final(env, env.rollout(T, mode=mode, actions=None if a_in is None else np.ascontiguousarray(a_in.transpose(0, 2, 1)), layout="soa",
                                     want=WANT, device_out=True))
        chunked = None
        if mode != "buffer":
            env = fresh()
            ch = env.rollout_chunked(T, mode=mode, chunk=64, want=WANT)
            chunked = final(env, {key: env.unchunk(v) for key, v in ch.items()})
        for other, name in ((unfused, "fused = 0"), (stepped, "single steps"), (soa, "feature-major"), (chunked, "chunk-major")):
            if other is not None:
                same_run(base, other, f"{mode} {name}")
        assert base["done"].any()
        if mode == "buffer":   # ... and rmav_step itself
            env = fresh()
            steps = [env.step(acts[t]) for t in range(T)]
            st = final(env, dict(actions=acts, obs=np.stack([x[0] for x in steps]), rew=np.stack([x[1] for x in steps]),
                                 done=np.stack([x[2] for x in steps]).astype(np.uint8)))
            same_run(base, st, "rmav_step")


# ---- 3. the twin --------------------------------------------------------------------------------------------------------------------------------
def obs_rows_of(out, nS):
    """run_ops' observation arrays in the order it produced them -> [(key, b of the first row, rows [T, n, nS])]; final_obs rides on
    its step's counter."""
    res, t = [], 0
    for key, v in out.items():
        if key.startswith("obs:"):
            x = rows(v, nS)
            x = x[None] if x.ndim == 2 else x
            res.append((key, t + 1, x))
            t += x.shape[0]
        elif key.startswith("final:"):
            res.append((key, t, rows(v, nS)[None]))
    return res


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,config", [(m, "all") for m in SIZES] + [(63, "plain"), (130, "limit")])
def test_the_twin(G, kind, n, config):
    nS, ids = NS[kind], BASE + np.arange(n)
    outs = []
    for sigma in (SIGMA, None):
        env = make(G, kind, n, sigma, **CONFIGS[config])
        outs.append(run_ops(G, env, kind, n))
        outs[-1]["control"] = env.control()
        env.close()
    noisy, twin = outs
    assert list(noisy) == list(twin)
    for key in noisy:
        if not key.startswith(("obs:", "final:")):
            same(noisy[key], twin[key], f"{config}: {key}")
    checked = 0
    for (key, b0, o), (_, _, s) in zip(obs_rows_of(noisy, nS), obs_rows_of(twin, nS)):
        for k in range(o.shape[0]):
            mask = None
            if key.startswith("final:"):   # only the finished envs' rows are written
                mask = np.broadcast_to(noisy["done:step_final"].astype(bool)[:, None], o[k].shape)
            inside(o[k], s[k], kind, ids, b0 + k, f"{config}: {key}[{k}]", mask=mask)
            checked += 1
    assert checked >= 2 + 6 * 3
    assert int(noisy["t"][0]) == b0 + o.shape[0] - 1


# ---- 4. reductions ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_an_all_zero_spec_and_a_set_then_none_handle_store_the_bits_of_a_plain_handle(G, kind, n):
    outs = {}
    for name in ("plain", "zero", "off"):
        env = make(G, kind, n, {"plain": None, "zero": 0.0, "off": SIGMA}[name], **CONFIGS["all"])
        if name == "off":
            env.sensor_noise = None
        assert (env.sensor_noise is None) == (name != "zero")
        outs[name] = run_ops(G, env, kind, n)
        env.close()
    plain = outs["plain"]
    for key, v in plain.items():
        if key.startswith("obs:"):
            x = host(v)
            assert not ((x == 0) & np.signbit(x)).any(), f"{key}: the plain run holds a -0.0 observation"
    for name in ("zero", "off"):
        assert set(outs[name]) == set(plain)
        for key in plain:
            if key.startswith("final:"):   # (rows of unfinished envs are not written)
                m = plain["done:step_final"].astype(bool)
                same(rows(outs[name][key], NS[kind])[m], rows(plain[key], NS[kind])[m], f"{name}: {key}")
            else:
                same(outs[name][key], plain[key], f"{name}: {key}")


@pytest.mark.parametrize("kind", KINDS)
def test_zero_components_equal_the_twins(G, kind):
    n, nS = 65, NS[kind]
    sigma = [0.0 if c % 3 == 1 else SIGMA for c in range(nS)]
    zero = np.array(sigma) == 0
    outs = []
    for s in (sigma, None):
        env = make(G, kind, n, s, **CONFIGS["all"])
        outs.append(run_ops(G, env, kind, n))
        env.close()
    for (key, _, o), (_, _, s) in zip(obs_rows_of(outs[0], nS), obs_rows_of(outs[1], nS)):
        if key.startswith("obs:"):
            assert not ((s == 0) & np.signbit(s)).any()
            same(o[..., zero], s[..., zero], f"{key}: sigma = 0")
            assert (o[..., ~zero] != s[..., ~zero]).mean() > 0.99, key


@pytest.mark.parametrize("actor", TD.ACTORS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,config", [(m, "all") for m in SIZES] + [(65, "plain"), (130, "norm_boot")])
def test_the_reductions_through_the_three_actors(G, actor, kind, n, config):
    """An all-zero spec and a set-then-None handle store the bits of a handle without the feature through the policy rollouts too (the form
    of test_gpu_disturbance's all-zero test): the *_sn kernels with sigma = 0, identity tables and the calm disturbance against the kernels
    a plain handle launches."""
    outs = {}
    for name in ("plain", "zero", "off"):
        kw, norm = TD.POLICY_CONFIGS[config]
        env = make(G, kind, n, {"plain": None, "zero": 0.0, "off": SIGMA}[name], **kw)
        if name == "off":
            env.sensor_noise = None
        assert (env.sensor_noise is None) == (name != "zero")
        outs[name] = TD.collect(env, actor, T, norm, clip_actions=(-0.5, 0.5) if config == "all" else None)
        env.close()
    x = outs["plain"]["obs"]
    assert not ((x == 0) & np.signbit(x)).any(), "the plain run holds a -0.0 observation"
    for name in ("zero", "off"):
        for key in outs["plain"]:
            same(outs[name][key], outs["plain"][key], f"{actor} {config} {name}: {key}")
    assert outs["plain"]["done"].any() or config == "plain"


# ---- 5. policy rollouts: the three actors ---------------------------------------------------------------------------------------------------
VALUE_TOL = {"fp32_mfma": TB.VALUE_TOL["f32m"], "f16": TB.VALUE_TOL["f16"], "f16_shared": TB.VALUE_TOL["f16"]}   # values against the torch policy
POLICY_CONFIGS = TD.POLICY_CONFIGS


def policy_of(env, actor, norm):
    """test_gpu_disturbance.policy_of with the value head's last layer scaled by 4.  The share test below tells a net that read the noisy
    observation from one that read the true state by 10 x VALUE_TOL; the f16 actors' tolerance is 200 x the fp32 one (4e-3 against 2e-5),
    and a freshly initialised value head moves by about that much under sigma = 0.25, so its sensitivity is raised - for every actor alike."""
    import torch

    pol = TD.policy_of(env, actor, norm)
    with torch.no_grad():
        pol.vf[-1].weight.mul_(4.0)
    return pol


def collect(env, pol, actor, steps, **kw):
    """test_gpu_disturbance.collect with a given policy."""
    import torch
    from gym_reinmav_amd.ppo import FusedPolicyCollector

    limited = env.max_episode_steps is not None
    col = FusedPolicyCollector(env, pol, steps, f16_mfma=(actor == "f16"), bootstrap_truncated=limited, **kw)
    col.collect()
    torch.cuda.synchronize()
    out = {key: getattr(col, key).cpu().numpy() for key in ("act", "obs", "rew", "done", "logp", "val")}
    if limited:
        out.update(boot=col.boot.cpu().numpy(), trunc=col.trunc.cpu().numpy())
    out.update(state=env.get_state(), sbd=env.get_sbd(), rc=env.get_reset_counts(), t=np.array([env.step_count]))
    return out


def one_step_launches(G, actor, kind, n, config):
    """T one-step launches of an actor -> (policy, params, per-launch records)."""
    import torch
    from gym_reinmav_amd.ppo import FusedPolicyCollector

    kw, norm = POLICY_CONFIGS[config]
    env = make(G, kind, n, **kw)
    p = TD.set_tether(env, kind, "walk")
    pol = policy_of(env, actor, norm)
    limited = env.max_episode_steps is not None
    col = FusedPolicyCollector(env, pol, 1, f16_mfma=(actor == "f16"), bootstrap_truncated=limited, clip_actions=(-0.5, 0.5) if config == "all" else None)
    recs = []
    for k in range(T):
        pre = env.get_state()
        col.collect()
        torch.cuda.synchronize()
        rec = {key: getattr(col, key).cpu().numpy().copy() for key in ("act", "obs", "rew", "done", "logp", "val")}
        if limited:
            rec.update(boot=col.boot.cpu().numpy().copy(), trunc=col.trunc.cpu().numpy().copy())
        rec.update(pre=pre, post=env.get_state(), observe=env.observe(layout="soa"))
        recs.append(rec)
        col.roll_over()
    tail = dict(state=env.get_state(), sbd=env.get_sbd(), rc=env.get_reset_counts(), t=np.array([env.step_count]))
    env.close()
    return pol, p, recs, tail


@pytest.mark.parametrize("actor", TD.ACTORS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", (65, 130))
@pytest.mark.parametrize("config", ("plain", "norm_boot", "all"))
def test_policy_rollouts(G, actor, kind, n, config):
    """Configuration "all" (frame skip, randomised constants, tracking reward, clipped actions) checks the launch groupings, observe() and
    the values; the dynamics-from-the-true-state and bootstrap checks against the oracle run for "plain" and "norm_boot", whose single
    sub-step with the handle's own constants is what disturbance_ref.step_ref restates."""
    import torch

    nS, ids = NS[kind], BASE + np.arange(n)
    kw, norm = POLICY_CONFIGS[config]
    env = make(G, kind, n, **kw)
    TD.set_tether(env, kind, "walk")
    whole = collect(env, policy_of(env, actor, norm), actor, T, clip_actions=(-0.5, 0.5) if config == "all" else None)
    env.close()
    pol, p, recs, tail = one_step_launches(G, actor, kind, n, config)
    # a T-step launch equals T one-step launches, bit for bit in every array
    for k, rec in enumerate(recs):
        for key in ("act", "rew", "done", "logp") + (("boot", "trunc") if "boot" in rec else ()):
            same(whole[key][k], rec[key][0], f"{config}: {key}[{k}]")
        same(whole["obs"][k], rec["obs"][0], f"{config}: obs[{k}]")
        same(whole["obs"][k + 1], rec["obs"][1], f"{config}: obs[{k + 1}]")
        same(whole["val"][k], rec["val"][0], f"{config}: val[{k}]")
        same(whole["val"][k + 1], rec["val"][1], f"{config}: the bootstrap value behind step {k}")
        same(rec["obs"][1], rec["observe"], f"{config}: obs[k + 1] of a one-step launch is observe()")
    for key in tail:
        same(whole[key], tail[key], f"{config}: {key}")
    # val[k] is the value of the STORED noisy obs[k]; the value of the true state is somewhere else
    missed = []
    for k, rec in enumerate(recs):
        with torch.no_grad():
            v = pol(torch.from_numpy(rec["obs"][0]).cuda())[1].cpu().numpy()
            v_true = pol(torch.from_numpy(np.ascontiguousarray(rec["pre"].T)).cuda())[1].cpu().numpy()
        tol = VALUE_TOL[actor] * max(1.0, float(np.abs(v).max()))
        assert np.abs(rec["val"][0] - v).max() < tol, (config, k, float(np.abs(rec["val"][0] - v).max()), tol)
        missed.append(np.abs(rec["val"][0] - v_true) > 10 * tol)
        print(f"{actor} {config} {kind} n={n} step {k}: max |val - V(noisy obs)| = {np.abs(rec['val'][0] - v).max():.3g} of {tol:.3g}; "
              f"share missing V(true state) by 10 x: {missed[-1].mean():.3f}")
        inside(rec["obs"][0].T, rec["pre"], kind, ids, k, f"{config}: the actor's observation")
    share = float(np.mean(missed))
    assert share > 0.5, (config, share)
    if config == "all":
        return
    # the dynamics ran from the TRUE state: step_ref (d = 0) from get_state before and the stored action, for the lanes that went on
    checked = 0
    for k, rec in enumerate(recs):
        go = ~rec["done"][0].astype(bool)
        act = np.ascontiguousarray(rec["act"][0].T)
        none = np.full(n, -1, np.int32)
        if go.any():
            m = int(go.sum())
            TD.check_step(kind, p, rec["pre"][go], act[go], none[:m], np.zeros((3, m)), rec["post"][go], rec["rew"][0][go], np.zeros(m, bool),
                          f"sensor {config} n={n} step {k}")
            checked += m
        if "trunc" in rec and rec["trunc"][0].any():
            # boot = the torch value of fma(sigma, z_ref(b = t + 1), s_final), s_final rebuilt by the oracle
            tr = rec["trunc"][0].astype(bool)
            s_fin, _, dn, _ = D.step_ref(kind, rec["pre"][tr], act[tr], none[:int(tr.sum())], p, np.zeros((3, int(tr.sum()))))
            assert not dn.any()
            o_fin, _ = R.o_ref(sig(kind), SEED, ids[tr], k + 1, s_fin.astype(F32))
            with torch.no_grad():
                v = pol(torch.from_numpy(np.ascontiguousarray(o_fin.astype(F32).T)).cuda())[1].cpu().numpy()
            assert np.abs(rec["boot"][0][tr] - v).max() < VALUE_TOL[actor] * max(1.0, float(np.abs(v).max())), (config, k)
            assert (rec["boot"][0][~tr] == 0).all()
    assert checked >= n
    if config == "norm_boot":
        assert sum(int(r["trunc"][0].sum()) for r in recs) >= n


# ---- 6. a set between two policy rollouts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("actor", TD.ACTORS)
def test_a_set_between_two_policy_rollouts_is_ordered_on_the_stream(G, actor):
    """The policy kernels read the handle's device copy of the spec, which rmav_set_sensor_noise rewrites with a launch of its own: set A,
    rollout, set B, rollout, nothing synchronised in between - the first rollout has A's observations, and the FIRST row the second one
    stores is already B's: it lies inside the restatement's bound with B's sigma around the true state (and outside with A's)."""
    import torch
    from gym_reinmav_amd.ppo import FusedPolicyCollector

    kind, n, sigma_b = "quad3d", 130, 0.5
    ids = BASE + np.arange(n)

    def run(second):
        env = make(G, kind, n, SIGMA)
        col = FusedPolicyCollector(env, TD.policy_of(env, actor, False), 4, f16_mfma=(actor == "f16"))
        col.collect()
        o1 = col.obs.clone()
        col.roll_over()
        if second is not None:
            env.sensor_noise = G.SensorNoise(second)
        col.collect(1)
        o2 = col.obs[:2].clone()
        torch.cuda.synchronize()
        state = env.get_state()
        assert env.step_count == 5
        env.close()
        return o1.cpu().numpy(), o2.cpu().numpy(), state

    a1, a2, sa = run(None)
    m1, m2, sm = run(sigma_b)
    same(m1, a1, "the rollout before the set keeps the first spec")
    same(m2[0], a1[4], "the row stored before the set")
    inside(a2[1].T, sa, kind, ids, 5, "without a set: the first spec", sigma=SIGMA)
    inside(m2[1].T, sm, kind, ids, 5, "the first row behind the set has the second spec", sigma=sigma_b)
    with pytest.raises(AssertionError):
        inside(m2[1].T, sm, kind, ids, 5, "... and not the first", sigma=SIGMA)


def test_the_actors_without_variant_kernels_are_refused(G):
    """The three actors a disturbance runs run sensor noise; the fp32 vector-ALU and bf16 actors are refused with a message that names the
    feature - by the collector, and by the library."""
    import torch

    from gym_reinmav_amd.ppo import FusedPolicyCollector, MlpPolicy, RolloutCollector

    env = make(G, "quad3d", 65)
    torch.manual_seed(0)
    policy = MlpPolicy(env.nS, env.nA).cuda()
    for kw in (dict(f32_mfma=False), dict(bf16_mfma=True)):
        with pytest.raises(ValueError, match="sensor-noise"):
            FusedPolicyCollector(env, policy, 2, **kw)
        plain = make(G, "quad3d", 65, None)
        col = FusedPolicyCollector(plain, policy, 2, **kw)
        plain.sensor_noise = G.SensorNoise(SIGMA)    # behind the collector's back: the library refuses
        with pytest.raises(G.RmavError, match="sensor noise"):
            col.collect()
        assert plain.step_count == 0
        plain.sensor_noise = None
        col.collect()
        assert plain.step_count == 2
        plain.close()
    with pytest.raises(ValueError, match="sensor_noise"):
        RolloutCollector(env, policy, 2, graph=True)   # (a replayed graph would repeat one noise pattern)
    ro = RolloutCollector(env, policy, 2)
    same(ro.obs[0], env.observe(layout="soa"), "the per-step collector starts from observe()")
    ro.collect()
    torch.cuda.synchronize()
    same(ro.obs[2], env.observe(layout="soa"), "... and stores what step() emits")
    env.close()


# ---- 7. moments on the device -----------------------------------------------------------------------------------------------------------------
def test_moments_on_the_device(G):
    env = make(G, "quad3d", R.MOMENT_N, base=0, seed=R.MOMENT_SEED)
    env.step_count = 5
    z = (env.observe().astype(np.float64) - env.get_state().astype(np.float64)) / SIGMA
    assert (np.abs(z.mean(0)) <= R.MEAN_CAP).all(), z.mean(0)
    assert (np.abs(z.std(0) - 1.0) <= R.STD_CAP).all(), z.std(0)
    env.close()


# ---- 8. API and keywords ------------------------------------------------------------------------------------------------------------------------
def test_round_trip_and_refusals(G):
    import ctypes as C

    A = G._abi
    env = make(G, "quad2d", 3, None)
    assert env.sensor_noise is None
    same(env.observe(), env.get_state(), "observe() on a plain handle")
    same(env.observe(layout="soa", device_out=True), env.get_state(layout="soa", device_out=True), "... on the device")
    env.sensor_noise = G.SensorNoise((0.5, 0.0, 0.25, 0.125, 1.0))
    assert env.sensor_noise.sigma == (0.5, 0.0, 0.25, 0.125, 1.0)
    lib, h = A.lib(), env._h
    for c, v in ((0, -0.5), (1, float("nan")), (2, float("inf")), (5, 0.1), (15, 1e-30)):
        bad = A.SensorNoiseSpec()
        bad.sigma[c] = v
        assert lib.rmav_set_sensor_noise(h, C.byref(bad)) == A.ERR_INVALID, (c, v)
        assert env.sensor_noise.sigma == (0.5, 0.0, 0.25, 0.125, 1.0), "the spec in force stays"
    for bad in (0.25, "0.25", (0.1,) * 4):
        with pytest.raises((TypeError, ValueError)):
            env.sensor_noise = bad
        assert env.sensor_noise.sigma == (0.5, 0.0, 0.25, 0.125, 1.0)
    spec, on = A.SensorNoiseSpec(), C.c_int32(-1)
    assert lib.rmav_get_sensor_noise(h, None, C.byref(on)) == 0 and on.value == 1
    assert lib.rmav_get_sensor_noise(h, C.byref(spec), None) == 0 and list(spec.sigma)[:5] == [0.5, 0.0, 0.25, 0.125, 1.0]
    env.sensor_noise = None
    assert lib.rmav_get_sensor_noise(h, C.byref(spec), C.byref(on)) == 0 and on.value == 0 and spec.sigma[0] == 0.5
    assert lib.rmav_observe(h, None, A.HOST, A.AOS) == A.ERR_INVALID
    env.close()
    with pytest.raises(ValueError):
        G.SensorNoise(0.1).spec(A.REINMAV)


def test_reinmav_takes_no_spec(G):
    import ctypes as C

    A = G._abi
    lib, h = A.lib(), C.c_void_p()
    p = A.default_params(A.REINMAV, None)
    A.check(lib.rmav_create(C.byref(h), A.REINMAV, 2, 0, 1, 0, 0, C.byref(p), None))
    spec = A.SensorNoiseSpec()
    assert lib.rmav_set_sensor_noise(h, C.byref(spec)) == A.ERR_INVALID
    assert lib.rmav_set_sensor_noise(h, None) == 0
    lib.rmav_destroy(h)


def test_the_keyword_reaches_every_constructor(G):
    import torch

    from gym_reinmav_amd.distributed import make_sharded

    sn = G.SensorNoise(SIGMA)
    shard = make_sharded("quad3d", 130, 1, 2, device=0, seed=SEED, sensor_noise=sn)
    assert shard.sensor_noise.sigma == (SIGMA,) * 10
    shard.close()
    single = G.make("quadrotor3d-v0", seed=SEED, sensor_noise=sn)
    o = single.reset()
    same(o.astype(F32), single._batch.observe()[0], "a native env's reset")
    o = single.step(single.control())[0]
    same(o.astype(F32), single._batch.observe()[0], "a native env's step")
    assert np.abs(o - single._batch.get_state()[0]).max() > 0
    single.close()
    n = 65
    for numpy_io in (True, False):
        noisy = G.QuadrotorVecEnv("quad2d", n, seed=SEED, env_id_base=BASE, max_episode_steps=H, terminal_observation=True, numpy_io=numpy_io,
                                  sensor_noise=sn)
        twin = G.QuadrotorVecEnv("quad2d", n, seed=SEED, env_id_base=BASE, max_episode_steps=H, terminal_observation=True, numpy_io=numpy_io)
        same(noisy.reset(), noisy.env.observe(), "vec-env reset")
        twin.reset()
        acts = D.parity_actions("quad2d", n)
        seen = 0
        for t in range(H + 1):
            a = acts[t] if numpy_io else torch.from_numpy(acts[t]).cuda()
            o, r, d, infos = noisy.step(a)
            o2, r2, d2, infos2 = twin.step(a)
            same(o, noisy.env.observe(), "vec-env step")
            same(r, r2, "rewards")
            same(d, d2, "done")
            for i in np.flatnonzero(host(d)):
                fo, fs = host(infos[int(i)]["terminal_observation"]), host(infos2[int(i)]["terminal_observation"])
                inside(fo[None], fs[None], "quad2d", np.array([BASE + int(i)]), t + 1, "terminal_observation")
                assert np.abs(fo - fs).max() > 0
                seen += 1
        assert seen >= n
        noisy.close()
        twin.close()

"""Observation normalisation on the GPU: the statistics kernels against a NumPy float64 restatement of baselines' RunningMeanStd
(tests/test_obs_norm_host.py), rmav_rollout_policy_norm against rmav_rollout_policy / _boot (identity statistics: the same bits),
against the oracle and the torch policy (non-trivial statistics, with and without a binding clip), and the Python layers on top."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from test_obs_norm_host import RefRunningMeanStd, check_against_ref
from util import KINDS, NA, NS, near_threshold

pytestmark = pytest.mark.gpu

ACTORS = ("f32m", "f16", "f16_shared")
# the project's tolerances for the same actors without normalisation (tests/test_gpu_ppo.py:170-175,250; tests/test_gpu_bootstrap.py:16)
VALUE_TOL = {"f32m": 2e-5, "f16": 4e-3, "f16_shared": 4e-3}
LOGP_TOL = 2e-3
INF = float("inf")


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import gym_reinmav_amd as g

    return g


def _norm(env, **kw):
    from gym_reinmav_amd.obs_norm import RunningObsNorm

    return RunningObsNorm(env.nS, f"cuda:{env.device}", **kw)


def _rows(obs_soa):
    """[T, nS, N] device tensor -> [T * N, nS] host rows"""
    return obs_soa.permute(0, 2, 1).reshape(-1, obs_soa.shape[1]).cpu().numpy()


def _moments(G, env, obs, layout, n_rows, pitch):
    import torch

    out = torch.full((33,), float("nan"), dtype=torch.float64, device=obs.device)
    G._abi.check(G._abi.lib().rmav_obs_moments(env._h, C.c_void_p(obs.data_ptr()), layout, n_rows, pitch, C.c_void_p(out.data_ptr())))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_moments(rec, x, ns):
    """rec = (count, mean[16], m2[16]) against two-pass float64 moments of the fp32 rows x [B, ns]; the bound of the host test"""
    x = x.astype(np.float64)
    n = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    tol = 4.0 * n * 2.0 ** -53
    assert rec[0] == n
    e_mean = np.abs(rec[1:1 + ns] - mean) / np.maximum(np.abs(mean), np.sqrt(var))
    e_var = np.abs(rec[17:17 + ns] / n - var) / var
    print(f"moments n={n}: mean err {e_mean.max():.3e} var err {e_var.max():.3e} bound {tol:.3e}")
    assert e_mean.max() <= tol and e_var.max() <= tol
    assert (rec[1 + ns:17] == 0).all() and (rec[17 + ns:] == 0).all()


# ---- 5. batch moments ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_moments_of_a_real_rollout(G, kind):
    import torch

    A = G._abi
    N, T, ns = 4096, 32, NS[kind]
    env = G.BatchedQuadrotor(kind, N, seed=5)
    obs = env.rollout(T, mode="random", layout="soa", device_out=True, want=("obs",))["obs"]
    x = _rows(obs)
    rec = _moments(G, env, obs, A.SOA, T, 0)
    _check_moments(rec, x, ns)
    assert np.array_equal(rec, _moments(G, env, obs, A.SOA, T, 0)), "two calls, two results: not deterministic"
    assert np.array_equal(rec, _moments(G, env, obs, A.SOA, T, N))
    P = N + 64                                                    # a larger pitch; the padding must not be read
    big = torch.full((T, ns, P), float("nan"), device=obs.device)
    big[..., :N] = obs
    _check_moments(_moments(G, env, big, A.SOA, T, P), x, ns)
    odd = torch.full((T * ns * (N + 3) + 1,), float("nan"), device=obs.device)[1:].view(T, ns, N + 3)   # misaligned base, odd pitch
    odd[..., :N] = obs
    _check_moments(_moments(G, env, odd, A.SOA, T, N + 3), x, ns)
    aos = obs[T - 1].t().contiguous()                             # one step, [N, nS]: what rmav_step writes
    _check_moments(_moments(G, env, aos, A.AOS, 1, 0), aos.cpu().numpy(), ns)
    rec0 = _moments(G, env, obs, A.SOA, 0, 0)                     # no rows: an empty record
    assert rec0[0] == 0 and np.isfinite(rec0).all()
    env.close()


def test_moments_of_a_ragged_batch(G):
    """N not a multiple of 4 (masked tail of the 16-byte loads) and smaller than a block"""
    A = G._abi
    for kind, N, T in (("quad3d", 4099, 5), ("quad2d", 131, 3), ("quad3d_sl", 1, 7)):
        env = G.BatchedQuadrotor(kind, N, seed=6)
        obs = env.rollout(T, mode="random", layout="soa", device_out=True, want=("obs",))["obs"]
        if N > 1:
            _check_moments(_moments(G, env, obs, A.SOA, T, 0), _rows(obs), NS[kind])
        else:
            assert _moments(G, env, obs, A.SOA, T, 0)[0] == T
        env.close()


# ---- 6. successive updates, the tables -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_ten_updates_match_the_restatement_and_the_tables_follow(G, kind):
    import torch

    N, T, ns = 2048, 8, NS[kind]
    env = G.BatchedQuadrotor(kind, N, seed=7)
    norm, ref, seen = _norm(env), RefRunningMeanStd(ns), 0
    for it in range(10):
        obs = env.rollout(T, mode="random", layout="soa", device_out=True, want=("obs",))["obs"]
        if it % 3 == 2:   # the VecEnv shape now and then
            aos = obs[0].t().contiguous()
            norm.update(aos, layout="aos", env=env)
            ref.update(aos.cpu().numpy())
            seen += N
        else:
            norm.update(obs, layout="soa", env=env)
            ref.update(_rows(obs))
            seen += T * N
        torch.cuda.synchronize()
        check_against_ref(norm.mean, norm.var, norm.count, ref, seen)
        mean_f, rstd_f = norm.mean_f.cpu().numpy(), norm.rstd_f.cpu().numpy()
        assert np.array_equal(mean_f, norm.mean.astype(np.float32))
        want = (1.0 / np.sqrt(norm.var + norm.eps)).astype(np.float32)
        assert (np.abs(rstd_f - want) <= np.spacing(want)).all()
        assert float(norm.clip_f) == 10.0
        full = norm.buf.cpu().numpy()
        assert (full[288 + 4 * ns:352].view(np.float32) == 0).all() and (full[352 + 4 * ns:416].view(np.float32) == 1).all()
    norm.freeze = True
    before = norm.buf.clone()
    norm.update(obs, layout="soa", env=env)
    torch.cuda.synchronize()
    assert torch.equal(before, norm.buf)
    env.close()


def _stats_from_a_rollout(G, env, clip=10.0, seed_steps=32):
    """statistics far from identity: absorbed from a random-action rollout of a twin handle"""
    twin = G.BatchedQuadrotor(env.kind, 2048, seed=99)
    norm = _norm(env, clip=clip)
    obs = twin.rollout(seed_steps, mode="random", layout="soa", device_out=True, want=("obs",))["obs"]
    # (the moments kernel takes the batch shape from the handle: use the twin's)
    norm.update(obs, layout="soa", env=twin)
    twin.sync()
    twin.close()
    return norm


# ---- 7. elementwise normalisation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("clip", [10.0, 1.0, INF])
def test_normalize_kernel_equals_the_torch_expression(G, kind, clip):
    import torch

    N, T, ns = 2048, 6, NS[kind]
    env = G.BatchedQuadrotor(kind, N, seed=8)
    norm = _stats_from_a_rollout(G, env, clip=clip)
    obs = env.rollout(T, mode="random", layout="soa", device_out=True, want=("obs",))["obs"]
    m, r = norm.mean_f, norm.rstd_f
    want = torch.clamp((obs - m[:, None]) * r[:, None], -clip, clip)
    got = norm.normalize(obs, layout="soa", env=env)
    assert got.data_ptr() != obs.data_ptr() and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(norm.normalize(obs, layout="soa").view(torch.int32), want.view(torch.int32))   # the torch path of the same method
    aos = obs.permute(0, 2, 1).contiguous()
    want_a = want.permute(0, 2, 1).contiguous()
    assert torch.equal(norm.normalize(aos, layout="aos", env=env).view(torch.int32), want_a.view(torch.int32))
    P = N + 64
    big = torch.zeros((T, ns, P), device=obs.device)
    big[..., :N] = obs
    view = big[..., :N]
    norm.normalize(view, out=view, layout="soa", env=env)        # pitched, in place
    assert torch.equal(view.view(torch.int32), want.view(torch.int32)) and (big[..., N:] == 0).all()
    inplace = obs.clone()
    assert norm.normalize(inplace, out=inplace, layout="soa", env=env) is inplace
    assert torch.equal(inplace.view(torch.int32), want.view(torch.int32))
    # against the float64 restatement: three roundings
    mean, var = norm.mean, norm.var
    x = _rows(obs).astype(np.float64)
    rstd = 1.0 / np.sqrt(var + norm.eps)
    zr = np.clip((x - mean) * rstd, -clip, clip)
    bound = 4 * 2.0 ** -24 * (np.abs(zr) + (np.abs(x) + np.abs(mean)) * rstd)
    err = np.abs(_rows(got) - zr)
    print(f"normalize vs float64: worst err / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
    if clip == 1.0:
        share = float((got.abs() == 1.0).float().mean())
        assert 0.1 < share < 0.9, share
    env.close()


# ---- 8. identity statistics: the old bits --------------------------------------------------------------------------------------------
def _policy(env, actor, scaled, obs_norm=None, seed=0):
    import torch
    from gym_reinmav_amd.ppo import MlpPolicy

    torch.manual_seed(seed)
    pol = MlpPolicy(env.nS, env.nA, init_logstd=0.0, value_network=("shared" if actor == "f16_shared" else "copy"), obs_norm=obs_norm).cuda()
    if scaled:   # until actions matter (tests/test_gpu_ppo.py: the default init has gain 0.01 on the action head)
        with torch.no_grad():
            for net in (pol.pi, pol.vf):
                net[-1].weight.mul_(20.0 if net is pol.pi else 1.0)
                for lin in net:
                    lin.bias.uniform_(-0.3, 0.3)
            pol.logstd.copy_(torch.linspace(-0.5, 0.3, env.nA))
    return pol


def _collector(env, pol, T, actor, boot):
    from gym_reinmav_amd.ppo import FusedPolicyCollector

    return FusedPolicyCollector(env, pol, T, f16_mfma=actor.startswith("f16"), bootstrap_truncated=boot)


def _snapshot(env):
    eb = env.episode_buffers()
    return dict(state=env.get_state(), sbd=env.get_sbd(), rc=env.get_reset_counts(), ll=eb["last_length"], cl=eb["cur_length"],
                lr=eb["last_return"], cr=eb["cur_return"], tot=env.episode_totals())


@pytest.mark.parametrize("limit", [None, 16])
@pytest.mark.parametrize("actor", ACTORS)
@pytest.mark.parametrize("kind", KINDS)
def test_identity_statistics_give_the_old_bits(G, kind, actor, limit):
    import torch

    N, T, seed = 4096 + 77, 40, 12
    a = G.BatchedQuadrotor(kind, N, seed=seed, max_episode_steps=limit)
    b = G.BatchedQuadrotor(kind, N, seed=seed, max_episode_steps=limit)
    norm = _norm(a, clip=INF)
    plain = _policy(a, actor, True)
    normed = _policy(a, actor, True, obs_norm=norm)
    normed.load_state_dict(plain.state_dict())
    ca, cb = _collector(a, normed, T, actor, bool(limit)), _collector(b, plain, T, actor, bool(limit))
    assert ca._call[0] is G._abi.lib().rmav_rollout_policy_norm and cb._call[0] is not ca._call[0]
    for it in range(2):
        ca.collect()
        cb.collect()
        torch.cuda.synchronize()
        for key in ("obs", "act", "rew", "done", "logp", "val") + (("boot", "trunc") if limit else ()):
            x, y = getattr(ca, key), getattr(cb, key)
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), \
                (kind, actor, limit, it, key)
        sa, sb = _snapshot(a), _snapshot(b)
        for k in sa:
            assert (sa[k] == sb[k]) if k == "tot" else np.array_equal(sa[k], sb[k]), k
        ca.roll_over()
        cb.roll_over()
    assert int((ca.done != 0).sum()) > 0 and (not limit or int((ca.trunc != 0).sum()) > 0)
    a.close()
    b.close()


# ---- 9. / 10. non-trivial statistics, with and without a binding clip ----------------------------------------------------------------
@pytest.mark.parametrize("clip", [10.0, 1.0])
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("actor", ACTORS)
@pytest.mark.parametrize("kind", KINDS)
def test_normalised_rollout_matches_torch_policy_and_oracle(G, kind, actor, scaled, clip):
    """Teacher-forced, as test_fused_policy_rollout_matches_torch_policy_and_oracle: the dynamics from the recorded (obs, action) against
    the oracle, values / implied noise / logp against the torch fp32 MlpPolicy(obs_norm=...) on the stored RAW obs, at the tolerances
    the same actor has without normalisation."""
    import torch
    from test_gpu_ppo import _check_rollout, _predicted_noise

    N, T, seed, base = 512 + 13, 12, 21, 1000
    env = G.BatchedQuadrotor(kind, N, seed=seed, env_id_base=base)
    norm = _stats_from_a_rollout(G, env, clip=clip)
    assert np.abs(norm.mean).max() > 0.01 and np.abs(norm.var - 1.0).max() > 0.1, "statistics too close to identity to test anything"
    pol = _policy(env, actor, scaled, obs_norm=norm, seed=2)
    ro = _collector(env, pol, T, actor, False)
    rc = env.get_reset_counts()
    t0 = env.step_count
    tol = VALUE_TOL[actor]
    for it in range(2):
        ro.collect()
        rc = _check_rollout(kind, seed, ro, rc, base)
        with torch.no_grad():
            obs = ro.obs[:T].permute(1, 0, 2).reshape(env.nS, -1)
            z_in = norm.normalize(obs)
            share = float((z_in.abs() == clip).float().mean())
            if clip == 1.0:
                assert 0.1 < share < 0.9, share      # the clip binds: this case cannot pass vacuously
            mean, val = pol(obs)
            mean, val = mean.reshape(env.nA, T, N), val.reshape(T, N)
            v_last = pol(ro.obs[T])[1]
            std = torch.exp(pol.logstd)[:, None, None]
        scale_v, scale_m = max(1.0, float(val.abs().max())), max(1.0, float(mean.abs().max()))
        e_v = max(float((ro.val[:T] - val).abs().max()), float((ro.val[T] - v_last).abs().max()))
        z = (ro.act.permute(1, 0, 2) - mean) / std
        logp_ref = -0.5 * (z * z).sum(0) - pol.logstd.detach().sum() - 0.5 * env.nA * np.log(2 * np.pi)
        e_lp = float((ro.logp - logp_ref).abs().max())
        zc = z.cpu().numpy()
        ids = np.arange(0, N, 37)
        e_z = max(np.abs(zc[:, t, ids].T - _predicted_noise(seed, base + ids, t0 + it * T + t)[:, :env.nA]).max() for t in (0, T - 1))
        z_tol = (2e-4 * 30) if actor == "f32m" else tol * scale_m / float(std.min())
        print(f"{kind} {actor} scaled={scaled} clip={clip}: value err {e_v:.3g} (bound {tol * scale_v:.3g}), logp err {e_lp:.3g}, "
              f"implied-noise err {e_z:.3g} (bound {z_tol:.3g}), clipped share {share:.2f}")
        assert e_v < tol * scale_v
        assert e_z < z_tol
        if actor == "f32m":
            assert e_lp < LOGP_TOL
        else:   # (the f16 actors' logp is the noise's own: compared with the predicted noise, as test_bf16_mfma_actor_matches_fp32_policy)
            zp = _predicted_noise(seed, base + np.arange(N), t0 + it * T)[:, :env.nA]
            lp = -0.5 * torch.from_numpy(zp ** 2).sum(1) - float(pol.logstd.detach().sum()) - 0.5 * env.nA * np.log(2 * np.pi)
            assert (ro.logp[0].cpu() - lp).abs().max() < 1e-3
        assert np.array_equal(env.get_state(layout="soa"), ro.obs[T].cpu().numpy())
        ro.roll_over()
    env.close()


# ---- 11. the bootstrap term under normalisation ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("actor", ACTORS)
@pytest.mark.parametrize("kind", ["quad3d", "quad2d_sl"])
def test_boot_is_the_value_net_on_the_normalised_terminal_state(G, kind, actor):
    import torch

    N, H, T, seed = 4096, 16, 64, 21
    env = G.BatchedQuadrotor(kind, N, seed=seed, max_episode_steps=H)
    norm = _stats_from_a_rollout(G, env, clip=2.0)
    pol = _policy(env, actor, True, obs_norm=norm)
    ro = _collector(env, pol, T, actor, True)
    ro.collect()
    torch.cuda.synchronize()
    trunc = ro.trunc != 0
    assert torch.equal(trunc, (ro.done != 0) & (ro.rew < 0))
    assert (ro.boot[~trunc] == 0).all()
    assert int(trunc.sum()) >= N * (T // H) // 4, int(trunc.sum())
    tt, ii = torch.nonzero(trunc, as_tuple=True)
    s_prev = ro.obs[:T].permute(0, 2, 1)[tt, ii].cpu().numpy().astype(np.float64)
    act = ro.act.permute(0, 2, 1)[tt, ii].cpu().numpy().astype(np.float64)
    s_fin, _, d, _ = O.batch_step(kind, s_prev, act, np.full(len(s_prev), -1, np.int32))
    assert not d[~near_threshold(kind, s_fin)].any()
    with torch.no_grad():
        fin = torch.from_numpy(s_fin.astype(np.float32).T.copy()).cuda()
        v = pol(fin)[1]
        norm.freeze = True
        raw_pol = _policy(env, actor, True)
        raw_pol.load_state_dict(pol.state_dict())
        v_raw = raw_pol(fin)[1]
    err, bound = float((ro.boot[tt, ii] - v).abs().max()), VALUE_TOL[actor] * max(1.0, float(v.abs().max()))
    print(f"{kind} {actor}: boot vs torch value of the normalised s_final: {err:.3g} (bound {bound:.3g}); vs the raw state {float((ro.boot[tt, ii] - v_raw).abs().max()):.3g}")
    assert err < bound
    assert float((ro.boot[tt, ii] - v_raw).abs().max()) > 10 * bound, "normalisation made no difference: the test shows nothing"
    env.close()


# ---- 12. a PPO loop ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("collector", ["fused", "eager", "graph"])
def test_ppo_loop_freezes_then_absorbs(G, collector):
    import torch
    from gym_reinmav_amd.ppo import PPO, FusedPolicyCollector, RolloutCollector

    torch.manual_seed(0)
    kind, N, T, seed = "quad3d", 4096, 16, 4
    env = G.BatchedQuadrotor(kind, N, seed=seed)
    norm, ref = _norm(env), RefRunningMeanStd(env.nS)
    pol = _policy(env, "f32m", False, obs_norm=norm)
    ro = FusedPolicyCollector(env, pol, T) if collector == "fused" else RolloutCollector(env, pol, T, graph=(collector == "graph"))
    ppo = PPO(pol, epochs=2, minibatches=4)
    first_ratio = []
    orig_loss = ppo.loss

    def loss(*a):
        out = orig_loss(*a)
        if not first_ratio or first_ratio[-1] is None:
            first_ratio[-1:] = [out[3].detach().clone()]
        return out

    ppo.loss = loss
    tol = VALUE_TOL["f32m"]
    sd_old = None
    for i in range(1, 4):
        ro.collect()
        with torch.no_grad():
            obs = ro.obs[:T].permute(1, 0, 2).reshape(env.nS, -1)
            v_now = pol(obs)[1].reshape(T, N)
            scale = max(1.0, float(v_now.abs().max()))
            e_now = float((ro.val[:T] - v_now).abs().max())
            assert e_now < tol * scale, (collector, i, e_now)       # the collector used the CURRENT statistics (a replay after an update too)
            if sd_old is not None:
                sd_new = norm.state_dict()
                norm.load_state_dict(sd_old)
                e_old = float((ro.val[:T] - pol(obs)[1].reshape(T, N)).abs().max())
                norm.load_state_dict(sd_new)
                print(f"{collector} iteration {i}: values vs torch with the new statistics {e_now:.3g}, with the old ones {e_old:.3g}")
                assert e_old > 10 * tol * scale, "the statistics did not change what the collector computes"
        sd_old = norm.state_dict()
        first_ratio.append(None)
        stats = ppo.update(ro)
        assert np.isfinite(list(stats.values())).all()
        torch.cuda.synchronize()
        ref.update(_rows(ro.obs[:T]))
        assert norm.count == 1e-4 + i * T * N
        check_against_ref(norm.mean, norm.var, norm.count, ref, i * T * N)
        lr = float(first_ratio[-1].log().abs().max())
        print(f"{collector} iteration {i}: |log ratio| on the first minibatch {lr:.3g}")
        if collector == "fused":
            assert lr < LOGP_TOL      # the learner sees the actor's normalisation
        ro.roll_over()
    env.close()


# ---- 13. VecNormalize ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numpy_io", [False, True])
def test_vec_normalize_keeps_baselines_order(G, numpy_io):
    import torch

    n, steps, seed, kind = 1024, 50, 17, "quadrotor3d-v0"
    venv = G.VecNormalize(G.QuadrotorVecEnv(kind, n, seed=seed, numpy_io=numpy_io, max_episode_steps=20, terminal_observation=True))
    raw = G.QuadrotorVecEnv(kind, n, seed=seed, numpy_io=numpy_io, max_episode_steps=20, terminal_observation=True)
    ns = raw.env.nS
    ref = RefRunningMeanStd(ns)
    host = (lambda x: np.asarray(x)) if numpy_io else (lambda x: x.cpu().numpy())

    def check(got, x):
        ref.update(x)                                   # update first, then normalise
        zr = ref.normalise(x)
        rstd = 1.0 / np.sqrt(ref.var + 1e-8)
        bound = 4 * 2.0 ** -24 * (np.abs(zr) + (np.abs(x.astype(np.float64)) + np.abs(ref.mean)) * rstd)
        assert got.dtype == np.float32 and (np.abs(got - zr) <= bound).all(), float((np.abs(got - zr) / bound).max())
        return rstd

    check(host(venv.reset()), host(raw.reset()))
    rng = np.random.RandomState(3)
    finished = 0
    for k in range(steps):
        act = rng.standard_normal((n, raw.env.nA)).astype(np.float32)
        a = act if numpy_io else torch.from_numpy(act).cuda()
        o1, r1, d1, i1 = venv.step(a)
        o0, r0, d0, i0 = raw.step(a)
        assert type(o1) is type(o0) and o1.shape == o0.shape
        check(host(o1), host(o0))
        assert np.array_equal(host(r1), host(r0)) and np.array_equal(host(d1), host(d0))
        m = venv.obs_norm.mean_f.cpu().numpy()
        r = venv.obs_norm.rstd_f.cpu().numpy()
        for j in np.nonzero(host(d0))[0]:
            e1, e0 = i1[j], i0[j]
            assert e1["episode"]["r"] == e0["episode"]["r"] and e1["episode"]["l"] == e0["episode"]["l"]
            assert e1["TimeLimit.truncated"] == e0["TimeLimit.truncated"]
            want = np.clip((e0["terminal_observation"] - m) * r, np.float32(-10), np.float32(10))
            assert np.array_equal(e1["terminal_observation"], want)
            finished += 1
        assert all(i1[j] == {} for j in np.nonzero(~host(d0).astype(bool))[0][:8])
    assert finished > n
    assert venv.obs_norm.count == ref.count and abs(ref.count - (steps + 1) * n - 1e-4) < 1e-9   # (51 sequential additions)
    with pytest.raises(ValueError, match="ret"):
        G.VecNormalize(raw, ret=True)
    venv.close()
    raw.close()


# ---- 14. boundaries ------------------------------------------------------------------------------------------------------------------
def test_boundaries(G):
    import torch
    from gym_reinmav_amd.ppo import FusedPolicyCollector, MlpPolicy

    A, L = G._abi, G._abi.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    N, T = 256, 4
    env = G.BatchedQuadrotor("quad3d", N, seed=1)
    lim = G.BatchedQuadrotor("quad3d", N, seed=1, max_episode_steps=8)
    rm = G.BatchedQuadrotor("reinmav", 64, seed=1)
    dev = torch.device("cuda", env.device)
    stats = torch.zeros(432 + 16, dtype=torch.uint8, device=dev)
    good, bad = stats[:432], stats[4:436]
    assert good.data_ptr() % 16 == 0 and bad.data_ptr() % 16 != 0
    obs = torch.zeros((T, env.nS, N), device=dev)
    rec = torch.zeros(33, dtype=torch.float64, device=dev)

    def invalid(rc, word):
        assert rc == A.ERR_INVALID and word in L.rmav_last_error(), (rc, L.rmav_last_error())

    assert L.rmav_obs_norm_init(env._h, p(good), 10.0, 1e-8, 1e-4) == A.OK
    invalid(L.rmav_obs_norm_init(env._h, None, 10.0, 1e-8, 1e-4), b"stats")
    invalid(L.rmav_obs_norm_init(env._h, p(bad), 10.0, 1e-8, 1e-4), b"aligned")
    invalid(L.rmav_obs_norm_init(env._h, p(good), 0.0, 1e-8, 1e-4), b"clip")
    invalid(L.rmav_obs_norm_init(env._h, p(good), 10.0, 1e-8, 0.0), b"count0")
    invalid(L.rmav_obs_norm_init(rm._h, p(good), 10.0, 1e-8, 1e-4), b"RMAV_REINMAV")
    torch.cuda.synchronize()
    # rmav_obs_norm_init writes what RunningObsNorm writes from the host
    from gym_reinmav_amd.obs_norm import RunningObsNorm

    assert torch.equal(good, RunningObsNorm(env.nS, dev).buf)
    # n_rows == 0: OK, nothing changes
    before = good.clone()
    assert L.rmav_obs_moments(env._h, p(obs), A.SOA, 0, 0, p(rec)) == A.OK
    assert L.rmav_obs_norm_merge(env._h, p(good), p(rec), 1) == A.OK
    assert L.rmav_obs_norm_merge(env._h, p(good), p(rec), 0) == A.OK
    assert L.rmav_obs_normalize(env._h, p(good), p(obs), p(obs), A.SOA, 0, 0) == A.OK
    torch.cuda.synchronize()
    assert torch.equal(before, good)
    invalid(L.rmav_obs_moments(env._h, None, A.SOA, T, 0, p(rec)), b"obs")
    invalid(L.rmav_obs_moments(env._h, p(obs), A.SOA, -1, 0, p(rec)), b"n_rows")
    invalid(L.rmav_obs_moments(env._h, p(obs), A.SOA, T, N - 1, p(rec)), b"pitch")
    invalid(L.rmav_obs_moments(env._h, p(obs), A.AOS, T, N, p(rec)), b"pitch")
    invalid(L.rmav_obs_moments(env._h, p(obs), 7, T, 0, p(rec)), b"layout")
    invalid(L.rmav_obs_moments(rm._h, p(obs), A.SOA, 1, 0, p(rec)), b"RMAV_REINMAV")
    invalid(L.rmav_obs_norm_merge(env._h, p(bad), p(rec), 1), b"aligned")
    invalid(L.rmav_obs_norm_merge(env._h, None, p(rec), 1), b"stats")
    invalid(L.rmav_obs_norm_merge(env._h, p(good), None, 1), b"batch")
    invalid(L.rmav_obs_norm_merge(rm._h, p(good), p(rec), 1), b"RMAV_REINMAV")
    invalid(L.rmav_obs_normalize(env._h, p(bad), p(obs), p(obs), A.SOA, T, 0), b"aligned")
    invalid(L.rmav_obs_normalize(env._h, p(good), None, p(obs), A.SOA, T, 0), b"in and out")
    invalid(L.rmav_obs_normalize(rm._h, p(good), p(obs), p(obs), A.SOA, 1, 0), b"RMAV_REINMAV")
    # the rollout
    w = torch.zeros(int(L.rmav_policy_weight_count_f32_mfma()), device=dev)
    act, rew = torch.zeros((T, env.nA, N), device=dev), torch.zeros((T, N), device=dev)
    done, val = torch.zeros((T, N), dtype=torch.uint8, device=dev), torch.zeros((T + 1, N), device=dev)
    logp, boot = torch.zeros((T, N), device=dev), torch.zeros((T, N), device=dev)

    def roll(h, st, prec, b=None, tr=None, lp=logp):
        return L.rmav_rollout_policy_norm(h, T, p(w), p(st), p(act), p(obs), p(rew), p(done), p(lp), p(val), p(b), p(tr), prec)

    assert roll(env._h, good, A.POLICY_FP32_MFMA) == A.OK
    assert roll(lim._h, good, A.POLICY_FP32_MFMA, boot, done.clone()) == A.OK
    assert roll(lim._h, good, A.POLICY_FP32_MFMA, boot) == A.OK          # trunc_out stays optional
    invalid(roll(env._h, None, A.POLICY_FP32_MFMA), b"stats")
    invalid(roll(env._h, bad, A.POLICY_FP32_MFMA), b"aligned")
    invalid(roll(env._h, good, A.POLICY_FP32_MFMA, boot), b"time limit")
    invalid(roll(env._h, good, A.POLICY_FP32_MFMA, None, done), b"time limit")
    invalid(roll(lim._h, good, A.POLICY_FP32_MFMA), b"boot_out")
    invalid(roll(env._h, good, A.POLICY_FP32_MFMA, lp=None), b"logp_out")
    for prec in (A.POLICY_FP32, A.POLICY_BF16_MFMA, 9):
        invalid(roll(env._h, good, prec), b"RMAV_POLICY_F16_MFMA")
    invalid(roll(rm._h, good, A.POLICY_FP32_MFMA), b"RMAV_REINMAV")
    torch.cuda.synchronize()
    # Python: the two actors without a normalised kernel, a time limit without the bootstrap buffers, a closed env
    norm = RunningObsNorm(env.nS, dev)
    pol = MlpPolicy(env.nS, env.nA, obs_norm=norm).cuda()
    for kw in (dict(bf16_mfma=True), dict(f32_mfma=False)):
        with pytest.raises(ValueError, match="obs_norm"):
            FusedPolicyCollector(env, pol, T, **kw)
    with pytest.raises(ValueError, match="bootstrap_truncated"):
        FusedPolicyCollector(lim, pol, T)
    with pytest.raises(ValueError, match="env="):
        norm.update(obs)
    col = FusedPolicyCollector(env, pol, T)
    col.collect()
    env.close()
    with pytest.raises(A.RmavError):
        col.collect()
    lim.close()
    rm.close()

"""Terminal observations and the bootstrap term of truncated steps: rmav_step_final, rmav_rollout_policy_boot, rmav_gae_boot and
what the Python layers build on them, against the oracle, twin handles and the torch policy."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from test_bootstrap_host import hand_placed, ref_f64
from util import KINDS, NA, NS, TOL, near_threshold, scaled_err

pytestmark = pytest.mark.gpu

N = 4096
ACTORS = (("f32m", False), ("f16", False), ("f16", True))   # (actor, shared trunk): as tests/test_gpu_time_limit.py
VALUE_TOL = {"f32m": 2e-5, "f16": 4e-3}                      # tests/test_gpu_ppo.py: fp32 values 2e-5, ACTOR_TOL["f16"] / ["f16_shared"] 4e-3
SENTINEL = np.float32(-12345.0)


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import gym_reinmav_amd as g

    return g


def _snapshot(env):
    eb = env.episode_buffers()
    return dict(state=env.get_state(), sbd=env.get_sbd(), rc=env.get_reset_counts(), trunc=env.episode_truncated(),
                ll=eb["last_length"], cl=eb["cur_length"], lr=eb["last_return"], cr=eb["cur_return"], tot=env.episode_totals())


def _same_bits(a, b):
    for k in a:
        if k == "tot":
            assert a[k] == b[k], (a[k], b[k])
        else:
            assert np.array_equal(a[k], b[k]), k


# ---- 4. single step -------------------------------------------------------------------------------------------------------------
def _run_step_final(G, kind, H, auto_reset, layout, device, n, steps=100, seed=21):
    """`steps` steps of N(0, 1) actions through rmav_step_final on one handle, through rmav_step on a twin with the same flags, and
    through rmav_step on a twin without auto-reset.  Returns the number of finished episodes whose final_obs was compared."""
    import torch

    nS, nA = NS[kind], NA[kind]
    mk = lambda ar: G.BatchedQuadrotor(kind, n, seed=seed, auto_reset=ar, max_episode_steps=H)  # noqa: E731
    env, ref, nores = mk(auto_reset), mk(auto_reset), mk(False)
    rng = np.random.RandomState(7)
    aos = layout == "aos"
    host = (lambda x: x.cpu().numpy()) if device else (lambda x: np.asarray(x))
    rows = (lambda x: host(x)) if aos else (lambda x: host(x).T)     # -> [N, dim]
    shared = np.ones(n, bool)      # envs that have not finished an episode yet: env and nores still share their state
    compared = 0
    for k in range(steps):
        prev = env.get_state().astype(np.float64)
        sbd = env.get_sbd()
        act = rng.normal(size=(n, nA)).astype(np.float32)
        a_in = np.ascontiguousarray(act if aos else act.T)
        fin0 = np.full((n, nS) if aos else (nS, n), SENTINEL, np.float32)
        if device:
            a_in = torch.from_numpy(a_in).cuda()
            out = (torch.empty(fin0.shape, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda"),
                   torch.from_numpy(fin0).cuda(), torch.empty(n, dtype=torch.uint8, device="cuda"))
        else:
            out = (np.empty(fin0.shape, np.float32), np.empty(n, np.float32), np.empty(n, np.uint8), fin0.copy(), np.empty(n, np.uint8))
        obs, rew, done, fin, trunc = env.step_final(a_in, layout=layout, out=out)
        o_r, r_r, d_r = ref.step(a_in, layout=layout)
        o_n, _, _ = nores.step(a_in, layout=layout)
        if device:
            torch.cuda.synchronize()
        obs, fin, o_r, o_n = rows(obs), rows(fin), rows(o_r), rows(o_n)
        rew, r_r = host(rew), host(r_r)
        done, trunc, d_r = host(done).astype(bool), host(trunc).astype(bool), host(d_r).astype(bool)
        # everything rmav_step reports: bit-equal
        assert np.array_equal(obs, o_r) and np.array_equal(rew, r_r) and np.array_equal(done, d_r), (kind, H, k)
        # the oracle, from the pre-step state
        s2, _, d, _ = O.batch_step(kind, prev, act.astype(np.float64), sbd)
        sure = ~near_threshold(kind, s2)
        assert np.array_equal(trunc[sure], (done & ~d)[sure]), (kind, H, k)
        if H is None:
            assert not trunc.any()
        cmp_ = done & sure & np.isfinite(s2).all(axis=1)
        assert scaled_err(fin[cmp_], s2[cmp_]).max(initial=0.0) <= TOL, (kind, H, k)
        compared += int(cmp_.sum())
        # envs that did not finish keep the sentinel
        assert (fin[~done] == SENTINEL).all(), (kind, H, k)
        # up to and including its first finished episode an env shares its state with the twin that never resets
        first = done & shared
        assert np.array_equal(fin[first], o_n[first]), (kind, H, k)
        if not auto_reset:
            assert np.array_equal(fin[done], obs[done])
        shared &= ~done
    _same_bits(_snapshot(env), _snapshot(ref))
    for e in (env, ref, nores):
        e.close()
    return compared


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H", [None, 16, 80])
def test_step_final_vs_oracle_and_twins(G, kind, H):
    for auto_reset in (True, False):
        for layout in ("aos", "soa"):
            for device in (False, True):
                got = _run_step_final(G, kind, H, auto_reset, layout, device, N)
                assert got >= N // 2, (kind, H, auto_reset, layout, device, got)


@pytest.mark.parametrize("kind", KINDS)
def test_step_final_on_a_one_wavefront_handle(G, kind):
    """<= 64 envs with host arrays: the pinned completion-word path the gym-shaped single env uses"""
    for H in (None, 16):
        for layout in ("aos", "soa"):
            got = _run_step_final(G, kind, H, True, layout, False, 64)
            assert got >= 32, (kind, H, layout, got)


# ---- 5. / 6. the fused policy rollouts ------------------------------------------------------------------------------------------
def _policy(G, env, shared):
    import torch
    from gym_reinmav_amd import ppo as P

    torch.manual_seed(0)
    return P.MlpPolicy(env.nS, env.nA, init_logstd=0.0, value_network="shared" if shared else "copy").cuda()   # N(0, 1) exploration


def _collect(G, env, actor, T, shared, boot, pol=None):
    from gym_reinmav_amd import ppo as P

    pol = pol or _policy(G, env, shared)
    col = P.FusedPolicyCollector(env, pol, T, f16_mfma=(actor == "f16"), bootstrap_truncated=boot)
    col.collect()
    return col, pol


@pytest.mark.parametrize("actor,shared", ACTORS)
def test_boot_is_the_value_net_on_the_terminal_state(G, actor, shared):
    """A handle with H = 16 and an unlimited twin, both rolled T = H steps from creation: where the twin runs on, the limited handle is
    truncated at step H - 1 and its boot is the twin's value of the state after H steps - the same device function on the same state,
    bit for bit.  (Compared on the envs the twin did not terminate in ANY of the H steps: an env that terminated earlier was reset
    in both and is not at its limit at step H - 1.)"""
    import torch

    H, kind, seed = 16, "quad3d", 21
    lim = G.BatchedQuadrotor(kind, N, seed=seed, max_episode_steps=H)
    twin = G.BatchedQuadrotor(kind, N, seed=seed)
    cl, pol = _collect(G, lim, actor, H, shared, True)
    ct, _ = _collect(G, twin, actor, H, shared, False, pol)
    torch.cuda.synchronize()
    keep = ~(ct.done != 0).any(dim=0)
    assert int(keep.sum()) >= N // 2, int(keep.sum())
    assert (cl.trunc[H - 1][keep] == 1).all()
    diff = (cl.boot[H - 1][keep] - ct.val[H][keep]).abs().max()
    print(f"boot vs twin value_out[H] ({actor}, shared={shared}): max |diff| = {float(diff):.3g} over {int(keep.sum())} envs")
    assert torch.equal(cl.boot[H - 1][keep], ct.val[H][keep])
    assert (cl.boot[cl.trunc == 0] == 0).all()
    assert torch.equal(cl.trunc[:H - 1], torch.zeros_like(cl.trunc[:H - 1]))
    lim.close()
    twin.close()


@pytest.mark.parametrize("actor,shared", ACTORS)
def test_several_truncations_per_rollout(G, actor, shared):
    import torch

    H, T, kind, seed = 16, 64, "quad3d", 21
    a, b = G.BatchedQuadrotor(kind, N, seed=seed, max_episode_steps=H), G.BatchedQuadrotor(kind, N, seed=seed, max_episode_steps=H)
    ca, pol = _collect(G, a, actor, T, shared, True)
    cb, _ = _collect(G, b, actor, T, shared, False, pol)
    torch.cuda.synchronize()
    # everything but boot / trunc: rmav_rollout_policy's bits
    for key in ("obs", "act", "rew", "done", "logp", "val"):
        assert torch.equal(getattr(ca, key), getattr(cb, key)), (actor, shared, key)
    _same_bits(_snapshot(a), _snapshot(b))
    trunc = ca.trunc != 0
    assert torch.equal(trunc, (ca.done != 0) & (ca.rew < 0))
    assert (ca.boot[~trunc] == 0).all()
    assert int(trunc.sum()) >= N * (T // H) // 2, int(trunc.sum())
    # boot = the torch policy's value of s_final, rebuilt by the oracle from the kernel's own obs[t] and act[t]
    tt, ii = torch.nonzero(trunc, as_tuple=True)
    s_prev = ca.obs[:T].permute(0, 2, 1)[tt, ii].cpu().numpy().astype(np.float64)     # [M, nS]
    act = ca.act.permute(0, 2, 1)[tt, ii].cpu().numpy().astype(np.float64)
    s_fin, _, d, _ = O.batch_step(kind, s_prev, act, np.full(len(s_prev), -1, np.int32))
    assert not d[~near_threshold(kind, s_fin)].any()                                  # truncated, not terminated
    with torch.no_grad():
        v = pol(torch.from_numpy(s_fin.astype(np.float32).T.copy()).cuda())[1]
    err = (ca.boot[tt, ii] - v).abs().max()
    bound = VALUE_TOL[actor] * max(1.0, float(v.abs().max()))
    print(f"boot vs torch value of the oracle's s_final ({actor}, shared={shared}): max |err| = {float(err):.3g}, bound {bound:.3g}, "
          f"{len(tt)} truncated samples")
    assert err < bound
    a.close()
    b.close()


# ---- 7. GAE kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,T", [(1, 1), (63, 7), (64, 8), (1000, 17), (20037, 33), (65536, 32), (4096, 257)])
def test_gae_boot_matches_float64_recursion(G, n, T):
    import torch

    gamma, lam, scale = 0.99, 0.95, 0.5
    if n >= 5:
        rew, val, done, boot, trunc = hand_placed(T, n, n + T)
    else:
        rng = np.random.RandomState(n + T)
        rew, val = rng.normal(size=(T, n)).astype(np.float32), rng.normal(size=(T + 1, n)).astype(np.float32)
        done, boot = np.ones((T, n), np.uint8), rng.normal(size=(T, n)).astype(np.float32)
    env = G.BatchedQuadrotor("quad3d", n, track_episodes=False)
    r, v, d, b = (torch.from_numpy(x).cuda() for x in (rew, val, done, boot))
    sums = torch.zeros(2, dtype=torch.float64, device="cuda")
    adv, ret = env.gae(r, d, v, gamma, lam, reward_scale=scale, sums=sums, boot=b)
    exp_a, exp_r = ref_f64(rew, val, done, boot, gamma, lam, scale)
    tol = 1e-5 * max(1.0, np.abs(exp_a).max())
    assert np.abs(adv.cpu().numpy() - exp_a).max() < tol and np.abs(ret.cpu().numpy() - exp_r).max() < tol
    s = sums.cpu().numpy()
    assert abs(s[0] - exp_a.sum()) < 1e-4 * max(1.0, np.abs(exp_a).sum())
    assert abs(s[1] - (exp_a ** 2).sum()) < 1e-4 * max(1.0, (exp_a ** 2).sum())
    # boot = 0: rmav_gae's bits
    s0, s1 = torch.zeros_like(sums), torch.zeros_like(sums)
    a0, r0 = env.gae(r, d, v, gamma, lam, reward_scale=scale, sums=s0)
    a1, r1 = env.gae(r, d, v, gamma, lam, reward_scale=scale, sums=s1, boot=torch.zeros_like(r))
    assert torch.equal(a0, a1) and torch.equal(r0, r1) and torch.equal(s0, s1)
    env.close()


# ---- 8. the bias is gone, end to end --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("actor,shared", ACTORS)
def test_truncated_steps_target_r_plus_gamma_v(G, actor, shared):
    """V = c (all weights zero, last bias c), gamma = 0.99, lam = 1: on a truncated step the return target is r + gamma c with the
    bootstrap, r alone without it"""
    import torch
    from gym_reinmav_amd import ppo as P

    c, gamma, H, T = 2.5, 0.99, 16, 64
    for flag in (True, False):
        env = G.BatchedQuadrotor("quad3d", N, seed=21, max_episode_steps=H)
        pol = _policy(G, env, shared)
        with torch.no_grad():
            for prm in pol.parameters():
                prm.zero_()
            pol.vf[-1].bias.fill_(c)
        ro = P.FusedPolicyCollector(env, pol, T, f16_mfma=(actor == "f16"), bootstrap_truncated=flag).collect()
        ppo = P.PPO(pol, gamma=gamma, lam=1.0)
        # the GAE call of PPO.update
        _, ret = ro.env.gae(ro.rew, ro.done, ro.val, ppo.gamma, ppo.lam, ppo.reward_scale, boot=getattr(ro, "boot", None))
        torch.cuda.synchronize()
        trunc = (ro.done != 0) & (ro.rew < 0)
        assert int(trunc.sum()) >= N * (T // H) // 2
        want = ro.rew[trunc] + (gamma * c if flag else 0.0)
        err = ((ret[trunc] - want).abs() / want.abs().clamp(min=1.0)).max()
        assert err <= 1e-5, (flag, float(err))
        st = ppo.update(ro)                       # and the learner runs on such a rollout
        assert np.isfinite(st["vf_loss"])
        env.close()


# ---- 9. VecEnv and the per-step collector ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dict_infos,n", [(True, 256), (False, 8192)])
def test_vec_env_terminal_observation(G, dict_infos, n):
    import torch

    H = 5
    for flag in (True, False):
        venv = G.QuadrotorVecEnv("quadrotor3d-v0", n, seed=6, dict_infos=dict_infos, max_episode_steps=H, terminal_observation=flag)
        twin = G.BatchedQuadrotor("quad3d", n, seed=6, max_episode_steps=H)
        venv.reset()
        twin.reset()
        seen = 0
        for k in range(2 * H + 2):
            act = venv.env.control(layout="aos", device_out=True)
            if k % 2:   # push some envs out of the box: terminations between the truncations
                act[::7] = 10.0
            _, rew, done, infos = venv.step(act)
            _, _, d2, fin, tr2 = twin.step_final(act, layout="aos")
            d = done.cpu().numpy()
            fin, tr2 = fin.cpu().numpy(), tr2.cpu().numpy()
            assert np.array_equal(d, d2.cpu().numpy().astype(bool))
            for i in range(n):
                info = infos[i]
                if not d[i]:
                    assert info == {}
                    continue
                assert "episode" in info and info["TimeLimit.truncated"] == bool(tr2[i])
                if flag:
                    t = info["terminal_observation"]
                    assert t.dtype == np.float32 and t.shape == (venv.env.nS,) and np.array_equal(t, fin[i])
                    seen += 1
                else:
                    assert set(info) == {"episode", "TimeLimit.truncated"}
        if flag:
            assert seen >= n
            if not dict_infos:   # LazyInfos' staleness rule covers the terminal observations: the buffer has moved on
                venv.step(act)
                _, _, _, unread = venv.step(act)
                venv.step(act)
                with pytest.raises(RuntimeError):
                    unread[0]
        venv.close()
        twin.close()
    # numpy_io: the same key from host arrays
    venv = G.QuadrotorVecEnv("quadrotor3d-v0", 64, seed=6, numpy_io=True, max_episode_steps=H, terminal_observation=True)
    twin = G.BatchedQuadrotor("quad3d", 64, seed=6, max_episode_steps=H)
    venv.reset()
    twin.reset()
    for k in range(H):
        act = venv.env.control(layout="aos")
        _, _, done, infos = venv.step(act)
        _, _, d2, fin, _ = twin.step_final(act, layout="aos")
        assert np.array_equal(done, d2)
        for i in np.nonzero(done)[0]:
            assert np.array_equal(infos[i]["terminal_observation"], fin[i])
    assert done.sum() >= 32
    venv.close()
    twin.close()


@pytest.mark.parametrize("graph", [False, True])
def test_rollout_collector_bootstraps_truncated_steps(G, graph):
    """RolloutCollector(bootstrap_truncated=True): boot = the torch value net on rmav_step_final's final_obs where the step was
    truncated, checked against the torch value of the oracle's s_final; and it still captures into a graph."""
    import torch
    from gym_reinmav_amd import ppo as P

    H, T, kind = 8, 24, "quad3d"
    env = G.BatchedQuadrotor(kind, N, seed=21, max_episode_steps=H)
    pol = _policy(G, env, False)
    ro = P.RolloutCollector(env, pol, T, graph=graph, bootstrap_truncated=True)
    for it in range(2):
        ro.collect()
        torch.cuda.synchronize()
        trunc = ro.trunc != 0
        assert torch.equal(trunc, (ro.done != 0) & (ro.rew < 0)) and (ro.boot[~trunc] == 0).all()
        assert int(trunc.sum()) >= N * (T // H) // 2
        tt, ii = torch.nonzero(trunc, as_tuple=True)
        s_prev = ro.obs[:T].permute(0, 2, 1)[tt, ii].cpu().numpy().astype(np.float64)
        act = ro.act.permute(0, 2, 1)[tt, ii].cpu().numpy().astype(np.float64)
        s_fin, _, _, _ = O.batch_step(kind, s_prev, act, np.full(len(s_prev), -1, np.int32))
        with torch.no_grad():
            v = pol(torch.from_numpy(s_fin.astype(np.float32).T.copy()).cuda())[1]
        assert (ro.boot[tt, ii] - v).abs().max() < VALUE_TOL["f32m"] * max(1.0, float(v.abs().max()))
        st = P.PPO(pol).update(ro)
        assert np.isfinite(st["vf_loss"])
        ro.roll_over()
    nolim = G.BatchedQuadrotor(kind, 64)
    with pytest.raises(ValueError):
        P.RolloutCollector(nolim, pol, 4, bootstrap_truncated=True)
    nolim.close()
    env.close()


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(G):
    import torch
    from gym_reinmav_amd import ppo as P

    A = G._abi
    L = A.lib()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    T = 8
    w = torch.zeros(max(L.rmav_policy_weight_count(A.QUAD3D), L.rmav_policy_weight_count_bf16(), L.rmav_policy_weight_count_f32_mfma()), device="cuda")
    lp, v, bo = torch.empty((T, N), device="cuda"), torch.empty((T + 1, N), device="cuda"), torch.empty((T, N), device="cuda")

    def boot(env, prec, boot_out=bo):
        return L.rmav_rollout_policy_boot(env._h, T, p(w), None, None, None, None, p(lp), p(v), None if boot_out is None else p(boot_out), None, prec)

    nolim = G.BatchedQuadrotor("quad3d", N)
    assert boot(nolim, A.POLICY_FP32_MFMA) == A.ERR_INVALID and b"time limit" in L.rmav_last_error()
    with pytest.raises(ValueError):
        P.FusedPolicyCollector(nolim, P.MlpPolicy(nolim.nS, nolim.nA).cuda(), T, bootstrap_truncated=True)
    nolim.close()
    lim = G.BatchedQuadrotor("quad3d", N, max_episode_steps=16)
    for prec in (A.POLICY_FP32, A.POLICY_BF16_MFMA):
        assert boot(lim, prec) == A.ERR_INVALID and b"RMAV_POLICY_F16_MFMA" in L.rmav_last_error()
    assert boot(lim, A.POLICY_FP32_MFMA, None) == A.ERR_INVALID and b"boot_out" in L.rmav_last_error()
    assert lim.step_count == 0                       # a refused call runs nothing
    lim.close()
    rm = G.BatchedQuadrotor("reinmav", 64)
    a4, o13 = torch.zeros((64, 4), device="cuda"), torch.zeros((64, 13), device="cuda")
    r1, d1 = torch.zeros(64, device="cuda"), torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert L.rmav_step_final(rm._h, p(a4), p(o13), p(r1), p(d1), p(o13), p(d1), A.DEVICE, A.AOS) == A.ERR_INVALID
    assert len(L.rmav_last_error()) > 0
    assert boot(rm, A.POLICY_FP32_MFMA) == A.ERR_INVALID and len(L.rmav_last_error()) > 0
    rw, vv = torch.zeros((T, 64), device="cuda"), torch.zeros((T + 1, 64), device="cuda")
    dd = torch.zeros((T, 64), dtype=torch.uint8, device="cuda")
    assert L.rmav_gae_boot(rm._h, T, p(rw), p(dd), p(vv), p(rw), 0.99, 0.95, 1.0, p(rw.clone()), p(rw.clone()), None) == A.ERR_INVALID
    assert len(L.rmav_last_error()) > 0
    rm.close()

"""Return normalisation on the GPU: rmav_ret_moments / rmav_ret_norm_merge / rmav_ret_normalize / rmav_gae_norm, RunningReturnNorm,
PPO(ret_norm=...) and VecNormalize(norm_reward=True) against the float64 NumPy restatement of baselines' rule in
test_ret_norm_host.py (RefReturnNorm) - never against the code under test."""
import ctypes as C

import numpy as np
import pytest

from test_ret_norm_host import N, RefReturnNorm, T, synth

pytestmark = pytest.mark.gpu

INF = float("inf")
GAMMA = 0.99
U = 2.0 ** -24   # unit roundoff of fp32


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import gym_reinmav_amd as g

    return g


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _state(buf):
    """(count, mean, m2) of a statistics buffer (synchronises)"""
    return buf.cpu().numpy()[:24].view(np.float64).copy()


def _table(buf):
    """(rstd_f, clip_f) bits of a statistics buffer"""
    return buf.cpu().numpy()[48:56].view(np.float32).copy()


def _new_stats(G, env, clip=10.0, eps=1e-8, count0=1e-4):
    import torch

    buf = torch.zeros(64, dtype=torch.uint8, device=torch.device("cuda", env.device))
    G._abi.check(G._abi.lib().rmav_ret_norm_init(env._h, p(buf), clip, eps, count0))
    return buf


def _moments(G, env, rew, done, scale, carry, n_steps=None):
    import torch

    out = torch.full((3,), float("nan"), dtype=torch.float64, device=carry.device)
    G._abi.check(G._abi.lib().rmav_ret_moments(env._h, rew.shape[0] if n_steps is None else n_steps, p(rew), p(done), scale, GAMMA, p(carry), p(out)))
    return out


def error_model(rew, done, scale, S0=None, E0=None):
    """The derived bound on the fp32 recurrence R = fmaf(gamma, R, s r) against exact arithmetic, run in float64 beside the data:
        S_t = gamma S_{t-1} + |s r_t|            (a bound on |R_t|)
        E_t = gamma E_{t-1} + 2^-24 (|s r_t| + S_t)    (one rounding of the product s r, one of the fma; the error of step t-1 decays by gamma)
    both reset at done.  The assertions carry a factor 2 for the product rounding order (and the fp32 roundings of s and gamma themselves, each
    <= 2^-24 relative, which enter as 2^-24 |s r_t| and 2^-25 S_t).  -> E [T, N], S_T, E_T"""
    Tn, Nn = rew.shape
    S = np.zeros(Nn) if S0 is None else S0.copy()
    E = np.zeros(Nn) if E0 is None else E0.copy()
    out = np.empty((Tn, Nn))
    for t in range(Tn):
        a = np.abs(scale * rew[t].astype(np.float64))
        S = GAMMA * S + a
        E = GAMMA * E + U * (a + S)
        out[t] = E
        S[done[t] != 0] = 0.0
        E[done[t] != 0] = 0.0
    return out, S, E


def check_record(rec, R64, E, label=""):
    """a (count, mean, m2) record against the float64 returns R64, with the bounds of error_model"""
    mean64 = R64.mean()
    m2_64 = ((R64 - mean64) ** 2).sum()
    e_mean, b_mean = abs(rec[1] - mean64), 2 * E.mean() + 1e-12 * abs(mean64)
    e_sd, b_sd = abs(np.sqrt(rec[2]) - np.sqrt(m2_64)), 2 * np.sqrt((E ** 2).sum()) + 1e-12 * np.sqrt(m2_64)
    print(f"{label} count {rec[0]:.0f} mean err {e_mean:.3e} (bound {b_mean:.3e})  sqrt(m2) err {e_sd:.3e} (bound {b_sd:.3e})")
    assert rec[0] == R64.size
    assert e_mean <= b_mean and e_sd <= b_sd, (e_mean, b_mean, e_sd, b_sd)


def ref_merge(state, rec):
    """baselines' update_from_moments on (count, mean, m2) triples, float64; empty records are skipped"""
    count, mean, m2 = state
    bc, bm, bm2 = rec
    if not bc > 0:
        return state
    tot = count + bc
    d = bm - mean
    var = (m2 / count * count + bm2 / bc * bc + d * d * count * bc / tot) / tot
    return np.array([tot, mean + d * bc / tot, var * tot])


def _arbitrary_stats(G, env, clip, rec=(5000.0, 1.5, 5000.0 * 7.3)):
    """statistics far from identity: one record merged into a fresh buffer"""
    import torch

    buf = _new_stats(G, env, clip=clip)
    r = torch.tensor(rec, dtype=torch.float64, device=buf.device)
    G._abi.check(G._abi.lib().rmav_ret_norm_merge(env._h, p(buf), p(r), 1))
    return buf


# ---- 1. rmav_ret_normalize: the torch expression, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 0.05])
@pytest.mark.parametrize("clip", [INF, 0.25])
def test_normalize_is_the_torch_expression(G, scale, clip):
    import torch

    env = G.BatchedQuadrotor("quad3d", N, seed=1)
    rew, done = synth(1)
    # statistics of these very returns, so that z has the spread a user sees
    ref = RefReturnNorm(N)
    R64 = ref.returns(rew.astype(np.float64) * scale, done)
    buf = _arbitrary_stats(G, env, clip, rec=(float(R64.size), float(R64.mean()), float(R64.var() * R64.size)))
    x = _dev(rew)
    out = torch.empty_like(x)
    G._abi.check(G._abi.lib().rmav_ret_normalize(env._h, p(buf), p(x), p(out), x.numel(), scale))
    tab = buf[48:56].view(torch.float32)
    want = torch.clamp((x * scale) * tab[0], -tab[1], tab[1])
    assert torch.equal(out, want)
    assert float(tab[1]) == clip
    # against the restatement: one rounding of the table, two products
    st = _state(buf)
    z64 = np.clip(rew.astype(np.float64) * scale / np.sqrt(st[2] / st[0] + 1e-8), -clip, clip)
    assert np.abs(out.cpu().numpy() - z64).max() <= 4 * U * np.abs(z64).max()
    share = float((np.abs(rew.astype(np.float64) * scale / np.sqrt(st[2] / st[0] + 1e-8)) > clip).mean())
    print(f"clip {clip}: the restatement clips {share:.3f} of the samples")
    if clip != INF:
        assert 0.05 <= share <= 0.5, share
    # in place
    G._abi.check(G._abi.lib().rmav_ret_normalize(env._h, p(buf), p(x), p(x), x.numel(), scale))
    assert torch.equal(x, want)
    env.close()


# ---- 2. rmav_ret_moments against the restatement, with a derived bound --------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 0.05])
def test_moments_against_the_restatement(G, scale):
    import torch

    env = G.BatchedQuadrotor("quad3d", N, seed=1)
    dev = torch.device("cuda", env.device)
    rew, done = synth(2)
    ref = RefReturnNorm(N)
    R64 = ref.returns(rew.astype(np.float64) * scale, done)
    E, _, E_T = error_model(rew, done, scale)
    x, d = _dev(rew), _dev(done)
    carry = torch.zeros(N, dtype=torch.float32, device=dev)
    rec = _moments(G, env, x, d, scale, carry)
    check_record(rec.cpu().numpy(), R64, E, f"scale {scale}")
    c = carry.cpu().numpy().astype(np.float64)
    print(f"carry err / bound max {(np.abs(c - ref.R) / np.maximum(2 * E_T, 1e-300))[E_T > 0].max():.3f}")
    assert (np.abs(c - ref.R) <= 2 * E_T).all()
    assert (c[done[-1] != 0] == 0).all()
    # the same input gives the same bits
    carry2 = torch.zeros_like(carry)
    rec2 = _moments(G, env, x, d, scale, carry2)
    assert torch.equal(rec.view(torch.int64), rec2.view(torch.int64)) and torch.equal(carry, carry2)
    # n_steps = 0: an empty record, carry untouched
    before = carry.clone()
    rec0 = _moments(G, env, x, d, scale, carry, n_steps=0)
    assert rec0.cpu().tolist() == [0.0, 0.0, 0.0] and torch.equal(carry, before)
    # T at once = T1 then T2: the carry bit for bit, the merged statistics to 1e-12
    for T1 in (1, 13, 32):
        ca = torch.zeros_like(carry)
        ra = _moments(G, env, x[:T1].contiguous(), d[:T1].contiguous(), scale, ca)
        rb = _moments(G, env, x[T1:].contiguous(), d[T1:].contiguous(), scale, ca)
        assert torch.equal(ca, carry2), T1
        one, two = _new_stats(G, env), _new_stats(G, env)
        G._abi.check(G._abi.lib().rmav_ret_norm_merge(env._h, p(one), p(rec), 1))
        G._abi.check(G._abi.lib().rmav_ret_norm_merge(env._h, p(two), p(torch.stack([ra, rb])), 2))
        s1, s2 = _state(one), _state(two)
        assert s1[0] == 1e-4 + T * N and s2[0] == (1e-4 + T1 * N) + (T - T1) * N   # (two additions round differently from one)
        assert abs(s1[1] - s2[1]) <= 1e-12 * abs(s1[1]) and abs(s1[2] - s2[2]) <= 1e-12 * s1[2], (T1, s1, s2)
    env.close()


# ---- 3. merge --------------------------------------------------------------------------------------------------------------------------
def test_merge_against_the_restatement(G):
    import torch

    env = G.BatchedQuadrotor("quad3d", 256, seed=1)
    buf = _new_stats(G, env)
    st = _state(buf)
    assert st.tolist() == [1e-4, 0.0, 1e-4] and _table(buf).tolist() == [np.float32(1.0 / np.sqrt(1.0 + 1e-8)), 10.0]
    rng = np.random.default_rng(4)
    ref = st.copy()
    for n_batches in (1, 4, 3):   # world-size-n behaviour: n records in one launch, merged in order
        recs = np.zeros((n_batches, 3))
        for b in range(n_batches):
            cnt = float(rng.integers(1, 40000))
            recs[b] = (cnt, rng.normal() * 20.0, cnt * rng.uniform(0.1, 400.0))
        if n_batches == 4:
            recs[2] = 0.0   # an empty record is skipped
        G._abi.check(G._abi.lib().rmav_ret_norm_merge(env._h, p(buf), p(_dev(recs)), n_batches))
        for r in recs:
            ref = ref_merge(ref, r)
        st = _state(buf)
        assert st[0] == ref[0]
        assert abs(st[1] - ref[1]) <= 1e-12 * max(abs(ref[1]), np.sqrt(ref[2] / ref[0])) and abs(st[2] - ref[2]) <= 1e-12 * ref[2], (st, ref)
        tab = _table(buf)
        assert tab[0] == np.float32(1.0 / np.sqrt(st[2] / st[0] + 1e-8)) and tab[1] == np.float32(10.0)
    G._abi.check(G._abi.lib().rmav_ret_norm_merge(env._h, p(buf), None, 0))   # nothing to merge
    assert np.array_equal(_state(buf), st)
    env.close()


# ---- 4. rmav_gae_norm -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_boot", [False, True])
@pytest.mark.parametrize("scale", [1.0, 0.05])
def test_gae_norm_is_gae_on_normalised_rewards(G, with_boot, scale):
    import torch

    env = G.BatchedQuadrotor("quad3d", N, seed=1)
    dev = torch.device("cuda", env.device)
    L, chk = G._abi.lib(), G._abi.check
    rew, done = synth(5)
    rng = np.random.default_rng(6)
    x, d = _dev(rew), _dev(done)
    val = _dev(rng.standard_normal((T + 1, N)).astype(np.float32))
    boot = _dev((rng.standard_normal((T, N)) * (rng.random((T, N)) < 0.03) * done).astype(np.float32)) if with_boot else None
    new = lambda: (torch.empty_like(x), torch.empty_like(x), torch.full((2,), float("nan"), dtype=torch.float64, device=dev))  # noqa: E731

    def plain(r, s):
        a, q, sm = new()
        if with_boot:
            chk(L.rmav_gae_boot(env._h, T, p(r), p(d), p(val), p(boot), GAMMA, 0.95, s, p(a), p(q), p(sm)))
        else:
            chk(L.rmav_gae(env._h, T, p(r), p(d), p(val), GAMMA, 0.95, s, p(a), p(q), p(sm)))
        return a, q, sm

    def normed(buf, s):
        a, q, sm = new()
        chk(L.rmav_gae_norm(env._h, T, p(x), p(d), p(val), p(boot), p(buf), GAMMA, 0.95, s, p(a), p(q), p(sm)))
        return a, q, sm

    def same(u, v):
        return all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int64),
                               b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int64)) for a, b in zip(u, v))

    for clip in (INF, 0.25, 10.0):
        buf = _arbitrary_stats(G, env, clip, rec=(5000.0, 1.5, 5000.0 * 130.0 * scale * scale))
        z = torch.empty_like(x)
        chk(L.rmav_ret_normalize(env._h, p(buf), p(x), p(z), x.numel(), scale))
        if clip == 0.25:
            share = float((z.abs() == 0.25).float().mean())
            assert 0.05 <= share <= 0.5, share
        assert same(normed(buf, scale), plain(z, 1.0)), clip
        # without sums_out as well
        a, q, _ = new()
        chk(L.rmav_gae_norm(env._h, T, p(x), p(d), p(val), p(boot), p(buf), GAMMA, 0.95, scale, p(a), p(q), None))
        assert same((a, q), plain(z, 1.0)[:2])
    if scale == 1.0:   # identity statistics: the bits of rmav_gae / rmav_gae_boot on the raw rewards
        ident = _new_stats(G, env, clip=INF)
        assert _table(ident).tolist() == [1.0, INF]
        assert same(normed(ident, 1.0), plain(x, 1.0))
    env.close()


# ---- 5. end to end: collector -> PPO(ret_norm) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("actor,scale", [("f32m", 1.0), ("f16_shared", 0.05)])
def test_ppo_update_with_ret_norm_end_to_end(G, actor, scale):
    import torch
    from gym_reinmav_amd.ppo import PPO, FusedPolicyCollector, MlpPolicy
    from gym_reinmav_amd.ret_norm import RunningReturnNorm

    n, steps, H = 4096, 32, 20
    env = G.BatchedQuadrotor("quad3d", n, seed=11, max_episode_steps=H)
    torch.manual_seed(0)
    pol = MlpPolicy(env.nS, env.nA, value_network=("shared" if actor == "f16_shared" else "copy")).cuda()
    with torch.no_grad():
        pol.pi[2].bias[0] = 9.8
    col = FusedPolicyCollector(env, pol, steps, f16_mfma=(actor == "f16_shared"), bootstrap_truncated=True)
    norm = RunningReturnNorm(f"cuda:{env.device}")
    ppo = PPO(pol, epochs=1, minibatches=2, reward_scale=scale, ret_norm=norm)
    ref, ref_state = RefReturnNorm(n), np.array([1e-4, 0.0, 1e-4])
    R_all, E_all, S, E = [], [], None, None
    gae_orig = env.gae

    def gae_then_allow_syncs(*a, **k):
        out = gae_orig(*a, **k)
        torch.cuda.set_sync_debug_mode("default")   # everything up to and including the GAE launch was enqueued without a synchronisation
        return out

    env.gae = gae_then_allow_syncs
    for k in range(3):
        col.collect()
        torch.cuda.synchronize()
        raw = col.rew.clone()
        torch.cuda.set_sync_debug_mode("error")
        try:
            ppo.update(col)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(col.rew, raw), "ro.rew must stay raw"
        # the advantages the learner used = env.gae on torch-normalised rewards (statistics that already include this rollout)
        z = torch.clamp((col.rew * scale) * norm.rstd_f, -norm.clip_f, norm.clip_f)
        adv, ret = gae_orig(z, col.done, col.val, ppo.gamma, ppo.lam, 1.0, boot=col.boot)
        assert torch.equal(ppo.adv, adv) and torch.equal(ppo.ret, ret)
        # replay through the restatement
        rew, done = col.rew.cpu().numpy(), col.done.cpu().numpy()
        assert done.any() and not done.all()
        R64 = ref.returns(rew.astype(np.float64) * scale, done)
        Ek, S, E = error_model(rew, done, scale, S, E)
        R_all.append(R64)
        E_all.append(Ek)
        ref_state = ref_merge(ref_state, (R64.size, R64.mean(), R64.var() * R64.size))
        Rc, Ec = np.concatenate(R_all).ravel(), np.concatenate(E_all).ravel()
        c = norm.carry(env).cpu().numpy().astype(np.float64)
        assert (np.abs(c - ref.R) <= 2 * E).all()
        b_mean = 2 * Ec.mean() + 1e-12 * abs(ref_state[1])
        b_sd = 2 * np.sqrt((Ec ** 2).sum()) + 1e-12 * np.sqrt(ref_state[2])
        mean, var, count = norm.mean, norm.var, norm.count   # the only read-back of the statistics, last
        e_mean, e_sd = abs(mean - ref_state[1]), abs(np.sqrt(var * count) - np.sqrt(ref_state[2]))
        print(f"{actor} round {k}: count {count:.4f} mean {mean:.4f} std {np.sqrt(var):.4f} rstd_f {float(norm.rstd_f):.6f}  "
              f"mean err {e_mean:.3e} (bound {b_mean:.3e}) sqrt(m2) err {e_sd:.3e} (bound {b_sd:.3e})")
        assert count == ref_state[0] and abs(count - (1e-4 + (k + 1) * steps * n)) <= 1e-9   # (count0 plus the batch sizes, batch by batch)
        assert e_mean <= b_mean and e_sd <= b_sd
        assert np.float32(float(norm.rstd_f)) == np.float32(1.0 / np.sqrt(var + 1e-8))
        col.roll_over()
    env.gae = gae_orig
    env.close()


# ---- 6. VecNormalize(norm_reward=True): baselines' per-step order ---------------------------------------------------------------------------
@pytest.mark.parametrize("numpy_io", [False, True])
def test_vec_normalize_norm_reward(G, numpy_io):
    import torch

    n, steps, seed, kind, H = 1024, 50, 17, "quadrotor3d-v0", 20
    venv = G.VecNormalize(G.QuadrotorVecEnv(kind, n, seed=seed, numpy_io=numpy_io, max_episode_steps=H), norm_reward=True)
    twin = G.VecNormalize(G.QuadrotorVecEnv(kind, n, seed=seed, numpy_io=numpy_io, max_episode_steps=H))   # norm_reward=False: raw rewards
    assert twin.ret_norm is None and venv.ret_norm is not None and venv.ret_norm.gamma == GAMMA and venv.ret_norm.clip == 10.0
    host = (lambda x: np.asarray(x)) if numpy_io else (lambda x: x.cpu().numpy())
    ref = RefReturnNorm(n)
    S, E, sumE2 = np.zeros(n), np.zeros(n), 0.0
    carry = lambda: venv.ret_norm.carry(venv.venv.env).cpu().numpy()  # noqa: E731

    assert np.array_equal(host(venv.reset()), host(twin.reset()))
    assert (carry() == 0).all()
    rng = np.random.RandomState(3)
    finished = 0
    for k in range(steps):
        act = rng.standard_normal((n, venv.venv.env.nA)).astype(np.float32)
        a = act if numpy_io else torch.from_numpy(act).cuda()
        o1, r1, d1, i1 = venv.step(a)
        o0, r0, d0, i0 = twin.step(a)
        raw, done = host(r0).astype(np.float64), host(d0).astype(bool)
        # observations, dones and infos are those of norm_reward=False
        assert type(r1) is type(r0) and r1.shape == r0.shape and host(r1).dtype == np.float32
        assert np.array_equal(host(o1), host(o0)) and np.array_equal(host(d1), host(d0))
        for j in np.nonzero(done)[0]:
            assert i1[j]["episode"] == {**i0[j]["episode"], "t": i1[j]["episode"]["t"]} and i1[j]["TimeLimit.truncated"] == i0[j]["TimeLimit.truncated"]
            finished += 1
        assert all(i1[j] == {} for j in np.nonzero(~done)[0][:8])
        # the restatement, step by step: update with this step's returns, then normalise this step's rewards
        zr = ref.step(raw, done)
        Ek, S, E = error_model(raw[None].astype(np.float32), done[None], 1.0, S, E)
        sumE2 += float((Ek ** 2).sum())
        m2_64 = ref.var * ref.count
        rel_stat = (2 * np.sqrt(sumE2) + 1e-12 * np.sqrt(m2_64)) / np.sqrt(m2_64)   # relative error bound of sqrt(var), test 2's bound
        bound = 4 * U * np.abs(zr) + np.abs(zr) * rel_stat
        got = host(r1).astype(np.float64)
        assert (np.abs(got - zr) <= bound).all(), (k, float((np.abs(got - zr) / np.maximum(bound, 1e-300)).max()))
        c = carry().astype(np.float64)
        assert (c[done] == 0).all() and (np.abs(c - ref.R) <= 2 * E).all()
    assert finished > n
    assert venv.ret_norm.count == ref.count and abs(ref.count - (1e-4 + steps * n)) <= 1e-9   # (50 sequential additions)
    venv.reset()
    assert (carry() == 0).all()
    with pytest.raises(ValueError, match="ret"):
        G.VecNormalize(twin.venv, ret=True)
    venv.close()
    twin.close()


# ---- 7. boundaries -----------------------------------------------------------------------------------------------------------------------
def test_boundaries(G):
    import torch

    A, L = G._abi, G._abi.lib()
    n, steps = 256, 4
    env = G.BatchedQuadrotor("quad3d", n, seed=1)
    rm = G.BatchedQuadrotor("reinmav", n, seed=1)
    dev = torch.device("cuda", env.device)
    stats = torch.zeros(64 + 16, dtype=torch.uint8, device=dev)
    good, bad = stats[:64], stats[4:68]
    assert good.data_ptr() % 16 == 0 and bad.data_ptr() % 16 != 0
    rew, val = torch.zeros((steps, n), device=dev), torch.zeros((steps + 1, n), device=dev)
    done = torch.zeros((steps, n), dtype=torch.uint8, device=dev)
    adv, ret, carry = torch.empty_like(rew), torch.empty_like(rew), torch.zeros(n, device=dev)
    rec = torch.zeros(3, dtype=torch.float64, device=dev)

    def invalid(rc, word):
        assert rc == A.ERR_INVALID and word in L.rmav_last_error(), (rc, L.rmav_last_error())

    assert L.rmav_ret_norm_init(env._h, p(good), 10.0, 1e-8, 1e-4) == A.OK
    invalid(L.rmav_ret_norm_init(env._h, None, 10.0, 1e-8, 1e-4), b"stats")
    invalid(L.rmav_ret_norm_init(env._h, p(bad), 10.0, 1e-8, 1e-4), b"aligned")
    invalid(L.rmav_ret_norm_init(env._h, p(good), 0.0, 1e-8, 1e-4), b"clip")
    invalid(L.rmav_ret_norm_init(env._h, p(good), -1.0, 1e-8, 1e-4), b"clip")
    invalid(L.rmav_ret_norm_init(env._h, p(good), 10.0, -1e-8, 1e-4), b"eps")
    invalid(L.rmav_ret_norm_init(env._h, p(good), 10.0, 1e-8, 0.0), b"count0")
    invalid(L.rmav_ret_moments(env._h, -1, p(rew), p(done), 1.0, GAMMA, p(carry), p(rec)), b"n_steps")
    invalid(L.rmav_ret_moments(env._h, steps, p(rew), p(done), 1.0, GAMMA, None, p(rec)), b"carry")
    invalid(L.rmav_ret_moments(env._h, steps, p(rew), p(done), 1.0, GAMMA, p(carry), None), b"batch_out")
    invalid(L.rmav_ret_norm_merge(env._h, None, p(rec), 1), b"stats")
    invalid(L.rmav_ret_norm_merge(env._h, p(bad), p(rec), 1), b"aligned")
    invalid(L.rmav_ret_norm_merge(env._h, p(good), p(rec), -1), b"n_batches")
    invalid(L.rmav_ret_norm_merge(env._h, p(good), None, 1), b"batch")
    invalid(L.rmav_ret_normalize(env._h, None, p(rew), p(rew), rew.numel(), 1.0), b"stats")
    invalid(L.rmav_ret_normalize(env._h, p(bad), p(rew), p(rew), rew.numel(), 1.0), b"aligned")
    invalid(L.rmav_ret_normalize(env._h, p(good), p(rew), p(rew), -1, 1.0), b"count")
    assert L.rmav_ret_normalize(env._h, p(good), None, None, 0, 1.0) == A.OK
    g = lambda h, n_steps, boot, st: L.rmav_gae_norm(h, n_steps, p(rew), p(done), p(val), boot, st, GAMMA, 0.95, 1.0, p(adv), p(ret), None)  # noqa: E731
    assert g(env._h, steps, None, p(good)) == A.OK and g(env._h, steps, p(rew), p(good)) == A.OK
    invalid(g(env._h, steps, None, None), b"stats")
    invalid(g(env._h, steps, None, p(bad)), b"aligned")
    invalid(g(env._h, -1, None, p(good)), b"n_steps")
    invalid(g(env._h, 0, None, p(good)), b"n_steps")
    # RMAV_REINMAV: every call but the bootstrap form
    assert g(rm._h, steps, None, p(good)) == A.OK
    invalid(g(rm._h, steps, p(rew), p(good)), b"ReinmavEnv")
    assert L.rmav_ret_moments(rm._h, steps, p(rew), p(done), 1.0, GAMMA, p(carry), p(rec)) == A.OK
    torch.cuda.synchronize()
    assert rec.cpu().tolist() == [float(steps * n), 0.0, 0.0]
    env.close()
    rm.close()

"""The launches around the fused learner on the GPU (rmav_adv_moments, rmav_ppo_adam, PPO(fused_learner=True, fused_optimizer=True)):
every output against the fp64 restatement of tests/optim_ref.py under ITS bound (derived there from the roundings of the documented
expression; tests/test_optim_host.py shows on the CPU that eleven wrong expressions leave it by more than a decade on these inputs),
determinism, the refusals and the PPO integration.
Measured (MI355X, every case): error / asserted bound at most 0.25 (the parameters: the one rounding of p - u), 0.21 for the moments;
the table is in profiles/r26/optimizer.md.

B = 33 025 is the batch at which a lane adds two samples AND several workgroups write partials: 130 tiles of 256 on 128 workgroups,
workgroups 0 and 1 walk two tiles each (the second tile of workgroup 1 holds one sample)."""
import copy
import ctypes as C

import numpy as np
import pytest

import optim_ref as R

pytestmark = pytest.mark.gpu
BATCHES = (1, 2, 63, 64, 65, 256, 257, 2125, 33025)


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available()
    import gym_reinmav_amd as g

    return g


@pytest.fixture(scope="module")
def envs(G):
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = G.BatchedQuadrotor(kind, 64, seed=0)
        return made[kind]

    yield get
    for e in made.values():
        e.close()


def _bits(t):
    import torch

    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    import torch

    return torch.equal(_bits(a), _bits(b))


# ---- rmav_adv_moments ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
def test_adv_moments_against_the_restatement(envs, B):
    import torch

    assert -(-33025 // 256) == 130 and 33025 % 256 == 1
    env = envs("quad3d")
    for which in R.ADV_INPUTS:
        x = R.adv_input(which, B)
        adv = torch.from_numpy(x).cuda()
        out = env.adv_moments(adv).clone()
        again = env.adv_moments(adv).clone()
        ref, bound = R.adv_moments(x)
        got = out.double().cpu().numpy()
        print(f"adv-moments B={B} {which}: got {got} ref {ref} excess {R.excess(got, ref, bound):.3g}")
        assert R.excess(got, ref, bound) <= 1.0, (which, got, ref, bound)
        assert _same_bits(out, again), "two runs must give the same bits"
        if B == 1:
            assert got[0] == float(x[0]) and np.isnan(got[1])
        # through idx: positions drawn WITH repeats from a longer array
        M = B + 37
        rng = np.random.default_rng([R.SEED, B, 7])
        long = torch.from_numpy(R.adv_input(which, M)).cuda()
        idx = torch.from_numpy(rng.integers(0, M, B)).cuda()
        gathered = long[idx].contiguous()
        via_idx = env.adv_moments(long, idx).clone()
        via_gather = env.adv_moments(gathered).clone()
        assert _same_bits(via_idx, via_gather), "the idx route must give the bits of the gathered route"
        assert _same_bits(via_idx, env.adv_moments(long, idx))
        ref, bound = R.adv_moments(gathered.cpu().numpy())
        assert R.excess(via_idx.double().cpu().numpy(), ref, bound) <= 1.0, (which, "idx")
        supplied = torch.zeros(2, device="cuda")
        assert env.adv_moments(long, idx, out=supplied) is supplied and _same_bits(supplied, via_idx)


# ---- rmav_ppo_adam ------------------------------------------------------------------------------------------------------------------------
def _adam_call(env, kind, shared, c):
    """one rmav_ppo_adam on fresh device copies of the case -> (p, m, v as flat CUDA tensors, stats, grad after the call)"""
    import torch

    ps = [torch.from_numpy(a.copy()).cuda() for a in R.split(c["p"], kind, shared)]   # separate allocations, as a policy's tensors are
    grad, m, v = (torch.from_numpy(c[k].copy()).cuda() for k in ("grad", "m", "v"))
    stats = torch.zeros(2, device="cuda")
    ret = env.ppo_adam(ps, grad, m, v, c["step"], lr=R.LR, beta1=R.BETA1, beta2=R.BETA2, eps=R.EPS, max_grad_norm=c["max_grad_norm"],
                       grad_scale=c["grad_scale"], shared=shared, stats=stats)
    assert ret is stats
    return torch.cat([p.reshape(-1) for p in ps]), m, v, stats, grad


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("kind", sorted(R.KINDS))
def test_adam_against_the_restatement(envs, kind, shared):
    import torch

    env = envs(kind)
    assert sum(R.tensor_sizes(kind, shared)) == (env._lib.rmav_ppo_grad_shared_param_count if shared else env._lib.rmav_ppo_grad_param_count)(env.kind)
    for scenario in R.SCENARIOS:
        c = R.adam_case(kind, shared, scenario)
        p, m, v, stats, grad = _adam_call(env, kind, shared, c)
        ref = R.adam(c["grad"], c["p"], c["m"], c["v"], c["step"], max_grad_norm=c["max_grad_norm"], grad_scale=c["grad_scale"])
        got = dict(p=p, m=m, v=v, norm=stats[0], coef=stats[1])
        worst = {k: R.excess(t.double().cpu().numpy(), ref[k], ref["bound_" + k]) for k, t in got.items()}
        print(f"ppo-adam {kind} shared={int(shared)} {scenario}: norm {float(stats[0]):.6g} coef {float(stats[1]):.6g} excess "
              + " ".join(f"{k}={x:.3g}" for k, x in worst.items()))
        assert max(worst.values()) <= 1.0, (scenario, worst)
        assert _same_bits(grad, torch.from_numpy(c["grad"])), "grad is read only"
        p2, m2, v2, stats2, _ = _adam_call(env, kind, shared, c)
        assert _same_bits(p, p2) and _same_bits(m, m2) and _same_bits(v, v2) and _same_bits(stats, stats2), "two runs must give the same bits"
        if scenario == "one_nan":
            assert torch.isnan(p).all() and torch.isnan(m).all() and torch.isnan(v).all() and torch.isnan(stats).all()
        elif scenario == "huge_no_clip":   # g^2 overflows: v infinite, the step 0
            assert torch.isinf(v).all() and _same_bits(p, torch.from_numpy(c["p"])) and float(stats[1]) == 1.0
        elif scenario == "zero_grad":
            assert float(stats[0]) == 0.0 and float(stats[1]) == 1.0 and not _same_bits(p, torch.from_numpy(c["p"]))
        elif scenario.startswith("active"):
            assert float(stats[1]) < 0.2
        elif scenario == "first_step_inactive":
            assert float(stats[1]) == 1.0
    # stats_out is optional, and the env keeps a buffer of its own when the caller supplies none
    c = R.adam_case(kind, shared, "active_half")
    ps = [torch.from_numpy(a.copy()).cuda() for a in R.split(c["p"], kind, shared)]
    grad, m, v = (torch.from_numpy(c[k].copy()).cuda() for k in ("grad", "m", "v"))
    own = env.ppo_adam(ps, grad, m, v, c["step"], lr=R.LR, beta1=R.BETA1, beta2=R.BETA2, eps=R.EPS, max_grad_norm=c["max_grad_norm"],
                       grad_scale=c["grad_scale"], shared=shared)
    assert own is env.ppo_adam(ps, grad, m, v, c["step"] + 1, shared=shared)


def test_refusals_name_the_argument(G, envs):
    import torch

    A = G._abi
    kind, shared = "quad3d", False
    env = envs(kind)
    c = R.adam_case(kind, shared, "active_half")
    ps = [torch.from_numpy(a.copy()).cuda() for a in R.split(c["p"], kind, shared)]
    t = {k: torch.from_numpy(c[k].copy()).cuda() for k in ("grad", "m", "v")}
    names = {"grad": "grad", "m": "exp_avg", "v": "exp_avg_sq"}

    def adam(step=1, sh=0, null=(), null_param=None, reserved=(0, 0), n_ptrs=13, **hyper):
        h = dict(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5, max_grad_norm=0.5, grad_scale=1.0)
        h.update(hyper)
        spec = A.PpoAdamSpec(h["lr"], h["beta1"], h["beta2"], h["eps"], h["max_grad_norm"], h["grad_scale"], reserved)
        ptrs = (C.c_void_p * n_ptrs)(*[None if k == null_param else q.data_ptr() for k, q in enumerate(ps[:n_ptrs])])
        arg = {names[k]: (None if names[k] in null else C.c_void_p(x.data_ptr())) for k, x in t.items()}
        A.check(A.lib().rmav_ppo_adam(env._h, sh, arg["grad"], None if "params" in null else ptrs, arg["exp_avg"], arg["exp_avg_sq"], step,
                                      None if "spec" in null else C.byref(spec), None))

    adam()   # the arguments as they are pass (stats_out NULL is allowed)
    torch.cuda.synchronize()
    for name in ("grad", "params", "exp_avg", "exp_avg_sq", "spec"):
        with pytest.raises(A.RmavError, match=rf"\b{name} is NULL"):
            adam(null=(name,))
    for k in range(13):
        with pytest.raises(A.RmavError, match=rf"params\[{k}\] is NULL"):
            adam(null_param=k)
    with pytest.raises(A.RmavError, match=r"params\[8\] is NULL"):
        adam(sh=1, null_param=8, n_ptrs=9)
    with pytest.raises(A.RmavError, match="shared must be 0 or 1"):
        adam(sh=2)
    for bad in (0, -3):
        with pytest.raises(A.RmavError, match="step must be >= 1"):
            adam(step=bad)
    inf, nan = float("inf"), float("nan")
    for field, values in (("lr", (nan, inf, -1e-3)), ("beta1", (-0.1, 1.0, nan)), ("beta2", (-0.1, 1.0, 1.5, nan)), ("eps", (nan, inf, -1e-5)),
                          ("max_grad_norm", (nan, 0.0, -0.5)), ("grad_scale", (nan, inf, 0.0, -1.0))):
        for value in values:
            with pytest.raises(A.RmavError, match=rf"\b{field} must be"):
                adam(**{field: value})
    adam(max_grad_norm=inf, lr=0.0, eps=0.0, beta1=0.0, beta2=0.0)   # all allowed
    for reserved in ((1, 0), (0, -1)):
        with pytest.raises(A.RmavError, match="_reserved must be 0"):
            adam(reserved=reserved)
    # rmav_adv_moments
    adv = torch.randn(100, device="cuda")
    ws = torch.empty(A.lib().rmav_adv_moments_workspace_bytes(100) + 8, dtype=torch.uint8, device="cuda")
    out = torch.zeros(2, device="cuda")
    vp = lambda x, off=0: C.c_void_p(x.data_ptr() + off)  # noqa: E731

    def moments(batch=100, adv_p=vp(adv), ws_p=vp(ws), out_p=vp(out)):
        A.check(A.lib().rmav_adv_moments(env._h, batch, None, adv_p, ws_p, out_p))

    moments()
    for bad in (0, -2):
        with pytest.raises(A.RmavError, match="batch must be >= 1"):
            moments(batch=bad)
    for name, kw in (("adv", dict(adv_p=None)), ("workspace", dict(ws_p=None)), ("adv_norm_out", dict(out_p=None))):
        with pytest.raises(A.RmavError, match=rf"\b{name} is NULL"):
            moments(**kw)
    with pytest.raises(A.RmavError, match="workspace must be 8-byte aligned"):
        moments(ws_p=vp(ws, 4))
    torch.cuda.synchronize()


# ---- PPO(fused_learner=True, fused_optimizer=True) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("value_network", ["shared", "copy"])
def test_ppo_fused_optimizer_matches_the_restatement_call_by_call(G, value_network):
    """130 quadrotor3d envs x 8 steps, 2 epochs x 2 minibatches: every one of the 4 optimiser calls against the restatement on its own
    recorded inputs, every adv_norm against fp64 on adv[idx]; then the optimiser's state_dict round-trips and the torch-optimiser
    path carries on from the same moments."""
    import torch
    from gym_reinmav_amd.ppo import PPO, FusedPolicyCollector, MlpPolicy

    torch.manual_seed(3)
    shared = value_network == "shared"
    env = G.BatchedQuadrotor("quad3d", 130, seed=4)
    pol = MlpPolicy(env.nS, env.nA, value_network=value_network).cuda()
    ro = FusedPolicyCollector(env, pol, 8).collect()
    ppo = PPO(pol, epochs=2, minibatches=2, fused_learner=True, fused_optimizer=True)
    adam_calls, moment_calls = [], []
    real_adam, real_moments = env.ppo_adam, env.adv_moments

    def rec_adam(params, grad, exp_avg, exp_avg_sq, step, **kw):
        before = dict(p=torch.cat([p.detach().reshape(-1) for p in params]).clone(), grad=grad.clone(), m=exp_avg.clone(), v=exp_avg_sq.clone())
        stats = real_adam(params, grad, exp_avg, exp_avg_sq, step, **kw)
        after = dict(p=torch.cat([p.detach().reshape(-1) for p in params]).clone(), m=exp_avg.clone(), v=exp_avg_sq.clone(),
                     norm=stats[0].clone(), coef=stats[1].clone(), grad=grad.clone())
        adam_calls.append((before, after, step, kw))
        return stats

    def rec_moments(adv, idx=None, out=None):
        res = real_moments(adv, idx, out=out)
        moment_calls.append((adv[idx].clone(), res.clone()))
        return res

    env.ppo_adam, env.adv_moments = rec_adam, rec_moments
    try:
        st = ppo.update(ro)
    finally:
        del env.ppo_adam, env.adv_moments
    assert set(st) == {"pg_loss", "vf_loss", "ratio_max", "grad_norm", "explained_variance"} and np.isfinite(list(st.values())).all()
    assert len(adam_calls) == 4 and len(moment_calls) == 4
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    for k, (before, after, step, kw) in enumerate(adam_calls):
        assert step == k + 1 and kw["shared"] == shared and kw["grad_scale"] == 1.0 and kw["max_grad_norm"] == 0.5
        b = {n: t.cpu().numpy() for n, t in before.items()}
        ref = R.adam(b["grad"], b["p"], b["m"], b["v"], step, lr=f32(kw["lr"]), beta1=f32(kw["beta1"]), beta2=f32(kw["beta2"]),
                     eps=f32(kw["eps"]), max_grad_norm=kw["max_grad_norm"])
        worst = {n: R.excess(after[n].double().cpu().numpy(), ref[n], ref["bound_" + n]) for n in ("p", "m", "v", "norm", "coef")}
        print(f"ppo-fused-optimizer {value_network} call {k}: norm {float(after['norm']):.4g} coef {float(after['coef']):.4g} excess {worst}")
        assert max(worst.values()) <= 1.0, (k, worst)
        assert _same_bits(after["grad"], before["grad"])
        if k:
            assert _same_bits(before["p"], adam_calls[k - 1][1]["p"]) and _same_bits(before["m"], adam_calls[k - 1][1]["m"])
    assert st["grad_norm"] == float(adam_calls[-1][1]["norm"])
    for x, res in moment_calls:
        assert x.numel() == 130 * 8 // 2
        ref, bound = R.adv_moments(x.cpu().numpy())
        assert R.excess(res.double().cpu().numpy(), ref, bound) <= 1.0
    # the kernel's state IS the torch optimiser's: views of the flat buffers, step on the host
    ps = ppo._fused[0]
    m_flat, v_flat = ppo._fused_opt.exp_avg, ppo._fused_opt.exp_avg_sq
    assert all(int(ppo.opt.state[p]["step"]) == 4 for p in ps)
    assert torch.equal(torch.cat([ppo.opt.state[p]["exp_avg"].reshape(-1) for p in ps]), m_flat) and m_flat.abs().max() > 0
    assert _same_bits(m_flat, adam_calls[-1][1]["m"]) and _same_bits(v_flat, adam_calls[-1][1]["v"])
    # state_dict round trip: the loaded tensors are new ones; the next fused step copies them in and steps from them
    sd = copy.deepcopy(ppo.opt.state_dict())
    ppo.opt.load_state_dict(sd)
    assert ppo.opt.state[ps[0]]["exp_avg"].data_ptr() != m_flat.data_ptr()
    ppo.epochs = ppo.minibatches = 1
    env.ppo_adam = rec_adam
    try:
        ppo.update(ro)
    finally:
        del env.ppo_adam
    before, after, step, _ = adam_calls[-1]
    assert step == 5 and _same_bits(before["m"], adam_calls[-2][1]["m"]) and _same_bits(before["v"], adam_calls[-2][1]["v"])
    assert ppo.opt.state[ps[0]]["exp_avg"].data_ptr() == m_flat.data_ptr()
    sd2 = ppo.opt.state_dict()
    assert [int(s["step"]) for s in sd2["state"].values()] == [5] * len(ps)
    # ... and an update on the torch-optimiser path starts from the same exp_avg values
    ppo.fused_optimizer = False
    seen = []
    real_step = ppo.opt.step

    def rec_step(*a, **k):
        seen.append(torch.cat([ppo.opt.state[p]["exp_avg"].reshape(-1) for p in ps]).clone())
        return real_step(*a, **k)

    ppo.opt.step = rec_step
    try:
        st = ppo.update(ro)
    finally:
        ppo.opt.step = real_step
    assert len(seen) == 1 and _same_bits(seen[0], after["m"]) and all(int(ppo.opt.state[p]["step"]) == 6 for p in ps)
    assert "grad_norm" not in st and not _same_bits(m_flat, after["m"]), "torch's Adam stepped on the shared state"
    env.close()



def test_data_parallel_step_all_reduces_the_flat_gradient_once(G, monkeypatch):
    """A two-rank world whose SUM all-reduce doubles the buffer (both ranks hold the same gradient): one all_reduce per minibatch, on the
    flat gradient itself, grad_scale = 1 / 2 - and, 2 g / 2 being exact, the bits of the single-process update."""
    import torch
    import gym_reinmav_amd.ppo as P

    env = G.BatchedQuadrotor("quad3d", 130, seed=4)
    torch.manual_seed(3)
    pol = P.MlpPolicy(env.nS, env.nA, value_network="shared").cuda()
    ro = P.FusedPolicyCollector(env, pol, 8).collect()
    start = torch.cat([q.detach().reshape(-1) for q in P.PPO(pol, fused_learner=True)._fused_params()]).clone()
    finals, reduced, scales = {}, [], []
    real_adam = env.ppo_adam

    def rec_adam(*a, **kw):
        scales.append(kw["grad_scale"])
        return real_adam(*a, **kw)

    env.ppo_adam = rec_adam
    try:
        for world in (1, 2):
            p = copy.deepcopy(pol)
            ppo = P.PPO(p, epochs=1, minibatches=2, fused_learner=True, fused_optimizer=True)
            if world == 2:
                monkeypatch.setattr(P.dist, "is_initialized", lambda: True)
                monkeypatch.setattr(P.dist, "get_world_size", lambda *a: 2)
                monkeypatch.setattr(P.dist, "all_reduce", lambda t, op=None: (reduced.append(t.data_ptr()), t.mul_(2.0))[1])
            torch.manual_seed(17)
            ppo.update(ro)
            finals[world] = torch.cat([q.detach().reshape(-1) for q in ppo._fused[0]]).clone()
            flat_ptr = ppo._fused[1].data_ptr()
    finally:
        del env.ppo_adam
        monkeypatch.undo()
    assert scales == [1.0, 1.0, 0.5, 0.5] and reduced == [flat_ptr, flat_ptr]
    assert _same_bits(finals[1], finals[2]) and not _same_bits(finals[1], start), "both stepped, to the same bits"
    env.close()

"""The shared-trunk fused learner on the fp32 matrix cores, on the GPU (rmav_ppo_grad_shared_mfma, PPO(fused_learner=True,
matrix_learner=True)): gradients and statistics against the fp64 oracle with the torch fp32 learner as the yardstick, at the edges of
the wavefront tile (32 samples) and the workgroup step (128) and on walks of several tiles per wavefront; the exact zeros of the clipped
branches, determinism, the pitches, the workspace, the refusals and the PPO integration.

Tolerance (learner_mfma_ref.margin_mfma, learner_ref.FLOOR; derived in profiles/r29/learner_mfma.md): per parameter tensor,
err = max|g - g64| / max|g64|,
    err(kernel) <= margin_mfma(B) * max(err(torch fp32 learner on the same GPU, same inputs), FLOOR),
margin_mfma(B) = 10 at every B of BATCHES, 18.5 / 19.1 / 18.6 at the three WALKS.  The measured errors are in the profile."""
import copy
import ctypes as C

import numpy as np
import pytest

import learner_mfma_ref as M
from learner_mfma_ref import R

pytestmark = pytest.mark.gpu
SEED = R.SEED


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


def _params(pol):
    named = dict(pol.named_parameters())
    return [named[n] for n in R.NAMES]


def _spread(case, pitch, seed):
    """the case's samples scattered over arrays of `pitch` columns -> (arrays, idx int64 [B]): column idx[j] holds sample j, the other
    columns hold finite filler the launch must not read"""
    import torch

    B = case["adv"].numel()
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(pitch, generator=g)[:B]
    out = {}
    for k, v in case.items():
        full = torch.randn(v.shape[:-1] + (pitch,), generator=g) * 3.0
        full[..., idx] = v
        out[k] = full
    return out, idx


def _run(env, pol, case, idx=None, norm_buf=None, ent_coef=0.0, clip=R.CLIP, vf_coef=R.VF_COEF):
    """rmav_ppo_grad_shared_mfma on CUDA copies of the case -> (grad, stats) CUDA tensors (clones)"""
    import torch

    c = {k: v.cuda() for k, v in case.items()}
    adv_mb = c["adv"] if idx is None else c["adv"][idx]
    adv_norm = torch.stack(R.adv_moments(adv_mb))
    grad, stats = env.ppo_grad_shared_mfma(_params(pol), c["obs"], c["act"], c["logp_old"], c["val_old"], c["adv"], c["ret"], adv_norm,
                                           clip=clip, vf_coef=vf_coef, ent_coef=ent_coef, idx=idx, obs_norm=norm_buf)
    return grad.clone(), stats.clone()


def _check(kind, B, tag, g, s, g64, s64, gy, sy):
    """one kernel result against the oracle under the yardstick's rule; prints the case's learner-mfma-err line first"""
    ey = R.tensor_errors(kind, gy, g64)
    ek = R.tensor_errors(kind, g.double().cpu().numpy(), g64)
    s = s.double().cpu().numpy()
    m = M.margin_mfma(B)
    at = max(ek, key=lambda n: ek[n] / max(ey[n], M.FLOOR))
    print(f"learner-mfma-err kind={kind} B={B} {tag} kernel={max(ek.values()):.3e} torch={max(ey.values()):.3e} "
          f"ratio={ek[at] / max(ey[at], M.FLOOR):.2f} at={at} ({ek[at]:.2e} / {ey[at]:.2e}) margin={m:.1f}")
    assert np.isfinite(g.cpu().numpy()).all()
    for n in ek:
        assert ek[n] <= m * max(ey[n], M.FLOOR), (n, ek[n], ey[n], tag)
    for k in range(4):
        scale = max(1.0, abs(s64[k]))
        assert abs(s[k] - s64[k]) <= m * max(abs(sy[k] - s64[k]), M.FLOOR * scale), (k, s[k], sy[k], s64[k])


@pytest.mark.parametrize("B", M.BATCHES)
@pytest.mark.parametrize("kind", sorted(R.KINDS))
def test_gradients_and_statistics_against_the_fp64_oracle(envs, kind, B):
    """B = 33: wavefront 1 has a single live lane, wavefronts 2 and 3 none; B = 129: the same in a second workgroup."""
    import torch

    env = envs(kind)
    for with_norm in (False, True):
        norm = R.make_norm(kind, SEED) if with_norm else None
        case = R.make_case(kind, B, SEED, norm)
        norm_buf = norm.buffer("cuda") if with_norm else None
        spread, idx = _spread(case, B + 37, 11 + B)
        pol = R.trained_policy(kind, SEED).cuda()
        for ent in (0.0, 0.01):
            g64, s64, clear = R.oracle(kind, SEED, case, norm, ent_coef=ent)
            assert min(clear.values()) >= R.CLEAR, clear
            # the yardstick: PPO.loss + backward in fp32 on the GPU
            ypol = R.trained_policy(kind, SEED, norm.to(device="cuda") if with_norm else None).cuda()
            gy, sy = R.torch_learner(ypol, case, ent_coef=ent)
            for use_idx in (False, True):
                if use_idx:
                    g, s = _run(env, pol, spread, idx.cuda(), norm_buf, ent)
                else:
                    g, s = _run(env, pol, case, None, norm_buf, ent)
                _check(kind, B, f"norm={int(with_norm)} ent={ent} idx={int(use_idx)}", g, s, g64, s64, gy, sy)
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind,B,with_norm,use_idx,ent", M.WALKS)
def test_several_tiles_per_wavefront_against_the_fp64_oracle(envs, kind, B, with_norm, use_idx, ent):
    """More steps than workgroups: the 128 accumulator registers carried from tile to tile, the LDS tiles overwritten by every tile.
    B = G 128 + 1: workgroup 0 walks a second step that is a one-sample tail; B = 2 G 128 + 129: workgroup 0 walks three steps,
    workgroup 1's third is a one-sample tail; quad3d_sl at 3 G 128: three full steps per workgroup at nS = 16, contiguous."""
    env = envs(kind)
    st = M.steps(B)
    assert st > M.GROUPS and B % M.STEP in (0, 1)
    assert (st, B % M.STEP) in ((M.GROUPS + 1, 1), (2 * M.GROUPS + 2, 1), (3 * M.GROUPS, 0))
    norm = R.make_norm(kind, SEED) if with_norm else None
    case = R.make_case(kind, B, SEED, norm)
    g64, s64, clear = R.oracle(kind, SEED, case, norm, ent_coef=ent)
    assert min(clear.values()) >= R.CLEAR, clear
    gy, sy = R.torch_learner(R.trained_policy(kind, SEED, norm.to(device="cuda") if with_norm else None).cuda(), case, ent_coef=ent)
    pol, buf = R.trained_policy(kind, SEED).cuda(), (norm.buffer("cuda") if with_norm else None)
    if use_idx:
        spread, idx = _spread(case, B + 37, 11 + B)
        g, s = _run(env, pol, spread, idx.cuda(), buf, ent)
    else:
        g, s = _run(env, pol, case, None, buf, ent)
    _check(kind, B, f"norm={int(with_norm)} ent={ent} idx={int(use_idx)}", g, s, g64, s64, gy, sy)


@pytest.mark.parametrize("kind", ["quad2d_sl", "quad3d"])
def test_clipped_branches_give_exact_zeros(envs, kind):
    """the exact-zero cases of the vector-ALU shared learner's test, B = 130: a step and a two-sample tail"""
    import torch

    env, sl = envs(kind), R.slices(kind)
    pol = R.trained_policy(kind, SEED).cuda()
    trunk, logstd = slice(0, sl["pi.2.weight"].start), sl["logstd"]
    n_ls = logstd.stop - logstd.start

    def zero(g, name):
        return torch.equal(g[sl[name]], torch.zeros(sl[name].stop - sl[name].start))

    # every sample's clipped surrogate branch strictly active: nothing reaches the mean head, logstd keeps the entropy term alone; the
    # trunk still learns from the value head
    g, _ = _run(env, pol, R.make_case(kind, 130, SEED, mode="pg_clipped"), ent_coef=0.01)
    g = g.cpu()
    assert zero(g, "pi.2.weight") and zero(g, "pi.2.bias"), "the mean head's gradient must be bitwise zero"
    assert torch.equal(g[logstd], torch.full((n_ls,), -0.01)), g[logstd]   # 0 - ent_coef: one exact rounding
    assert g[trunk].abs().max() > 0 and g[sl["vf.0.weight"]].abs().max() > 0
    # v_clip's branch active everywhere with |v - val_old| > clip: nothing reaches the value head; the trunk learns from the mean head
    g, _ = _run(env, pol, R.make_case(kind, 130, SEED, mode="vf_clipped"))
    g = g.cpu()
    assert zero(g, "vf.0.weight") and zero(g, "vf.0.bias"), "the value head's gradient must be bitwise zero"
    assert g[trunk].abs().max() > 0 and g[sl["pi.2.weight"]].abs().max() > 0 and g[logstd].abs().max() > 0
    # both: every tensor but logstd
    g, _ = _run(env, pol, R.make_case(kind, 130, SEED, mode="both_clipped"), ent_coef=0.01)
    g = g.cpu()
    assert torch.equal(g[:logstd.start], torch.zeros(logstd.start)), "the whole net's gradient must be bitwise zero"
    assert torch.equal(g[logstd], torch.full((n_ls,), -0.01)), g[logstd]


@pytest.mark.parametrize("B", [2125, M.WALKS[0][1]])
def test_same_inputs_same_bits_and_idx_equals_gathered(envs, B):
    import torch

    kind = "quad3d"
    env = envs(kind)
    pol = R.trained_policy(kind, SEED).cuda()
    norm = R.make_norm(kind, SEED)
    case = R.make_case(kind, B, SEED, norm)
    buf = norm.buffer("cuda")
    g1, s1 = _run(env, pol, case, None, buf, 0.01)
    g2, s2 = _run(env, pol, case, None, buf, 0.01)
    assert torch.equal(g1, g2) and torch.equal(s1, s2)
    spread, idx = _spread(case, B + 101, 3)
    g3, s3 = _run(env, pol, spread, idx.cuda(), buf, 0.01)
    assert torch.equal(g1, g3) and torch.equal(s1, s3), "the idx route must give the bits of the gathered-contiguous route"
    assert g1.abs().max() > 0 and torch.isfinite(g1).all()


@pytest.mark.parametrize("use_idx", (False, True))
def test_unequal_pitches_give_the_bits_of_the_contiguous_call(envs, use_idx):
    """obs rows M + 37 apart, act rows M + 101 apart, the 1-D arrays of length M: the bits of the contiguous call"""
    import torch

    kind, B, ent = "quad3d", 130, 0.01
    env = envs(kind)
    pol = R.trained_policy(kind, SEED).cuda()
    norm = R.make_norm(kind, SEED)
    buf = norm.buffer("cuda")
    case, idx = R.make_case(kind, B, SEED, norm), None
    if use_idx:
        case, idx = _spread(case, B + 37, 11 + B)
        idx = idx.cuda()
    n_col = case["adv"].numel()
    g1, s1 = _run(env, pol, case, idx, buf, ent)
    wide = {k: v.cuda() for k, v in case.items()}
    gen = torch.Generator().manual_seed(5)
    for key, extra in (("obs", 37), ("act", 101)):   # finite filler behind every row, which the launch must not read
        full = (torch.randn(case[key].shape[0], n_col + extra, generator=gen) * 3.0).cuda()
        full[:, :n_col] = wide[key]
        wide[key] = full[:, :n_col]
        assert wide[key].stride() == (n_col + extra, 1) and not wide[key].is_contiguous()
    g2, s2 = _run(env, pol, wide, idx, buf, ent)
    assert torch.equal(g1, g2) and torch.equal(s1, s2)
    assert g1.abs().max() > 0 and torch.isfinite(g1).all()


def test_a_grown_workspace_is_reused_by_smaller_and_larger_batches(G):
    """B = 2 125 (17 workgroups), then 129 (2), then 2 125 on ONE handle, each result the bits of the same call on a fresh handle: a
    smaller batch must not fold partials a larger one left behind.  The vector-ALU shared learner on the same handle keeps a workspace
    of its own."""
    import torch

    kind, ent = "quad3d", 0.01
    pol = R.trained_policy(kind, SEED).cuda()
    norm = R.make_norm(kind, SEED)
    buf = norm.buffer("cuda")
    one = G.BatchedQuadrotor(kind, 64, seed=0)
    for B in (2125, 129, 2125):
        case = R.make_case(kind, B, SEED, norm)
        fresh = G.BatchedQuadrotor(kind, 64, seed=0)
        g0, s0 = _run(fresh, pol, case, None, buf, ent)
        g1, s1 = _run(one, pol, case, None, buf, ent)
        torch.cuda.synchronize()
        fresh.close()
        assert torch.equal(g0, g1) and torch.equal(s0, s1), B
        assert g0.abs().max() > 0 and torch.isfinite(g0).all()
    assert one._ppo_grad_shared_mfma_cache["ws"].numel() == G._abi.lib().rmav_ppo_grad_shared_mfma_workspace_bytes(one.kind, 2125)
    assert "_ppo_grad_shared_cache" not in one.__dict__
    one.close()


def _ppo_case(env, ro, ppo, T):
    case = dict(obs=ro.obs[:T].permute(1, 0, 2).reshape(env.nS, -1), act=ro.act.permute(1, 0, 2).reshape(env.nA, -1),
                logp_old=ro.logp.reshape(-1), val_old=ro.val[:T].reshape(-1), adv=ppo.adv.reshape(-1), ret=ppo.ret.reshape(-1))
    return {k: v.detach().cpu().clone() for k, v in case.items()}


def test_ppo_matrix_learner_leaves_the_torch_paths_gradients(G):
    """One epoch x one minibatch of 130 envs x 8 steps (8 full steps and a 16-sample tail), deep-copied shared-trunk policies, the
    same torch seed: the post-clip p.grad update() leaves behind against the fp64 oracle on that rollout."""
    import torch
    from gym_reinmav_amd.ppo import PPO, FusedPolicyCollector, MlpPolicy

    torch.manual_seed(3)
    T = 8
    env = G.BatchedQuadrotor("quad3d", 130, seed=4)
    pol_t = MlpPolicy(env.nS, env.nA, value_network="shared").cuda()
    with torch.no_grad():   # (the default init's 0.01 gain would hide the mean head)
        pol_t.pi[2].weight.mul_(30.0)
    pol_m = copy.deepcopy(pol_t)
    ro = FusedPolicyCollector(env, pol_t, T).collect()
    grads = {}
    for name, pol, kw in (("torch", pol_t, {}), ("matrix", pol_m, dict(fused_learner=True, matrix_learner=True))):
        ppo = PPO(pol, epochs=1, minibatches=1, ent_coef=0.01, **kw)
        assert ppo.matrix_learner is (name == "matrix")
        torch.manual_seed(17)
        before = [p.detach().clone() for p in pol.parameters()]
        st = ppo.update(ro)
        assert set(st) == {"pg_loss", "vf_loss", "ratio_max", "explained_variance"} and np.isfinite(list(st.values())).all()
        assert any(not torch.equal(a, p.detach()) for a, p in zip(before, pol.parameters())), "the optimiser stepped"
        grads[name] = torch.cat([g.reshape(-1) for g in (p.grad for p in _params(pol))]).double().cpu().numpy()
        if name == "torch":
            case, start = _ppo_case(env, ro, ppo, T), before
    # the fp64 oracle on the rollout, from the parameters both started with, clipped as clip_grad_norm_ does
    pol64 = MlpPolicy(env.nS, env.nA, value_network="shared").double()
    with torch.no_grad():
        for p, b in zip(pol64.parameters(), start):
            p.copy_(b.double().cpu())
    g64, _ = R.torch_learner(pol64, case, ent_coef=0.01)
    g64 = g64 * min(1.0, 0.5 / (np.linalg.norm(g64) + 1e-6))
    et, em = R.tensor_errors("quad3d", grads["torch"], g64), R.tensor_errors("quad3d", grads["matrix"], g64)
    m = M.margin_mfma(130 * T)
    for n in et:
        print(f"ppo-mfma-grad {n}: matrix {em[n]:.3e} torch {et[n]:.3e}")
        assert em[n] <= m * max(et[n], M.FLOOR), (n, em[n], et[n])
    env.close()


def test_ppo_matrix_learner_runs_and_fits_values(G):
    """12 iterations of 4 epochs x 4 minibatches at 4096 envs x 32 steps with the fused optimiser on: finite statistics with update's
    keys, and the value head picks the returns up - what test_ppo_fused_learner_runs_and_fits_values asks of the vector path."""
    import torch
    from gym_reinmav_amd.ppo import PPO, FusedPolicyCollector, MlpPolicy

    torch.manual_seed(0)
    env = G.BatchedQuadrotor("quad3d", 4096, seed=0)
    pol = MlpPolicy(env.nS, env.nA, value_network="shared").cuda()
    ro = FusedPolicyCollector(env, pol, 32)
    ppo = PPO(pol, fused_learner=True, fused_optimizer=True, matrix_learner=True)
    hist = []
    for it in range(12):
        ro.collect()
        hist.append(ppo.update(ro))
        ro.roll_over()
    print("ppo-mfma-ev", [round(h["explained_variance"], 4) for h in hist])
    assert all(set(h) == {"pg_loss", "vf_loss", "ratio_max", "explained_variance", "grad_norm"} for h in hist)
    assert all(np.isfinite(list(h.values())).all() for h in hist)
    assert all(h["ratio_max"] < 5.0 for h in hist)
    assert hist[-1]["explained_variance"] > max(0.02, hist[0]["explained_variance"])
    env.close()


def test_refusals_name_the_argument(G, envs):
    import torch

    A = G._abi
    kind = "quad3d"
    env = envs(kind)
    pol = R.trained_policy(kind, SEED).cuda()
    c = {k: v.cuda() for k, v in R.make_case(kind, 33, SEED).items()}
    adv_norm = torch.stack(R.adv_moments(c["adv"]))
    n_par = A.lib().rmav_ppo_grad_shared_param_count(env.kind)
    ws = torch.empty(A.lib().rmav_ppo_grad_shared_mfma_workspace_bytes(env.kind, 33), dtype=torch.uint8, device="cuda")
    grad, stats = torch.zeros(n_par, device="cuda"), torch.zeros(4, device="cuda")
    ptrs = (C.c_void_p * 9)(*[p.data_ptr() for p in _params(pol)])

    def call(batch=33, hyper=(0.2, 0.5, 0.0), null_param=None, obs_pitch=33, act_pitch=33, ws_off=0, **nulls):
        a = dict(obs=c["obs"], act=c["act"], logp_old=c["logp_old"], val_old=c["val_old"], adv=c["adv"], ret=c["ret"], adv_norm=adv_norm,
                 workspace=ws, grad_out=grad, stats_out=stats)
        p = {k: (None if k in nulls else C.c_void_p(v.data_ptr() + (ws_off if k == "workspace" else 0))) for k, v in a.items()}
        sp = None if "spec" in nulls else C.byref(A.PpoGradSpec(*hyper, 0))
        pp = ptrs
        if "params" in nulls:
            pp = None
        elif null_param is not None:
            pp = (C.c_void_p * 9)(*[None if k == null_param else q.data_ptr() for k, q in enumerate(_params(pol))])
        A.check(A.lib().rmav_ppo_grad_shared_mfma(env._h, batch, None, p["obs"], obs_pitch, p["act"], act_pitch, p["logp_old"], p["val_old"],
                                                  p["adv"], p["ret"], p["adv_norm"], pp, None, sp, p["workspace"], p["grad_out"],
                                                  p["stats_out"]))

    call()   # the arguments as they are pass
    torch.cuda.synchronize()
    assert stats.abs().max() > 0
    for name in ("obs", "act", "logp_old", "val_old", "adv", "ret", "adv_norm", "params", "spec", "workspace", "grad_out", "stats_out"):
        with pytest.raises(A.RmavError, match=rf"\b{name} is NULL"):
            call(**{name: True})
    for k in range(9):
        with pytest.raises(A.RmavError, match=rf"params\[{k}\] is NULL"):
            call(null_param=k)
    for bad in (0, -5):
        with pytest.raises(A.RmavError, match="batch must be"):
            call(batch=bad)
    with pytest.raises(A.RmavError, match="obs_pitch must be"):
        call(obs_pitch=32)
    with pytest.raises(A.RmavError, match="act_pitch must be"):
        call(act_pitch=32)
    for hyper, name in (((float("nan"), 0.5, 0.0), "clip"), ((-0.1, 0.5, 0.0), "clip"), ((float("inf"), 0.5, 0.0), "clip"),
                       ((0.2, float("inf"), 0.0), "vf_coef"), ((0.2, 0.5, float("nan")), "ent_coef")):
        with pytest.raises(A.RmavError, match=rf"\b{name} must be finite"):
            call(hyper=hyper)
    with pytest.raises(A.RmavError, match="workspace must be 16-byte aligned"):
        call(ws_off=4)

"""tests/optim_ref.py without a GPU: the restatement agrees with torch's own float64 arithmetic (torch.std_mean; clip_grad_norm_ +
torch.optim.Adam(eps=1e-5) over three consecutive steps), an fp32 NumPy walk through the header's lines sits inside its bound, every
arithmetic mutant leaves the bound by more than a decade on the inputs tests/test_gpu_optim.py launches, and PPO refuses
fused_optimizer without fused_learner.

Agreement with torch in float64 is asserted to 1024 fp64 roundings (1024 * 2^-53 = 1.1e-13) relative to the quantity's own scale: an
element's chain is about 16 operations, and the norm is a sum of ~10^4 squares that torch adds in another order (per tensor, then over
the tensors), a random walk of ~100 roundings; for the moments the scale is max |x|^2 / std, the conditioning of a variance."""
import numpy as np
import pytest

import optim_ref as R

TOL64 = 1024 * R.E


def test_moments_agree_with_torch_std_mean():
    import torch

    for which in ("normal", "offset"):
        for B in (2, 63, 257, 2125):
            x = R.adv_input(which, B).astype(np.float64)
            out, _ = R.adv_moments(x)
            std, mean = torch.std_mean(torch.from_numpy(x))
            want = 1.0 / (float(std) + R.EPS8)
            scale = np.abs(x).max()
            assert abs(out[0] - float(mean)) <= TOL64 * scale
            assert abs(out[1] - want) <= TOL64 * (scale ** 2 / float(std) ** 2) * want, (which, B)
    out, bound = R.adv_moments(R.adv_input("normal", 1))
    assert out[0] == float(R.adv_input("normal", 1)[0]) and np.isnan(out[1]) and bound[1] == 0.0
    out, _ = R.adv_moments(R.adv_input("constant", 257))
    assert out[0] == float(np.float32(0.37)) and out[1] == 1.0 / R.EPS8


@pytest.mark.parametrize("shared", [False, True])
def test_adam_agrees_with_torch_float64_over_three_steps(shared):
    import torch

    kind = "quad3d"
    sizes = R.tensor_sizes(kind, shared)
    rng = np.random.default_rng(5)
    ps = [torch.nn.Parameter(torch.from_numpy(0.3 * rng.standard_normal(s))) for s in sizes]
    opt = torch.optim.Adam(ps, lr=R.LR, betas=(R.BETA1, R.BETA2), eps=R.EPS)
    p = np.concatenate([q.detach().numpy() for q in ps])
    m, v = np.zeros_like(p), np.zeros_like(p)
    for step, (gnorm, max_norm) in enumerate(((0.05, 0.5), (5.0, 0.5), (2.0, 0.5)), start=1):   # clip inactive, active, active
        g = rng.standard_normal(p.size)
        g *= gnorm / np.linalg.norm(g)
        for q, gq in zip(ps, R.split(g, kind, shared)):
            q.grad = torch.from_numpy(gq.copy())
        total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
        got = R.adam(g, p, m, v, step, max_grad_norm=max_norm, exact=True)
        assert abs(got["norm"] - float(total)) <= TOL64 * gnorm
        assert (got["coef"] < 1.0) == (gnorm > max_norm)
        want_p = np.concatenate([q.detach().numpy() for q in ps])
        want_m = np.concatenate([opt.state[q]["exp_avg"].numpy() for q in ps])
        want_v = np.concatenate([opt.state[q]["exp_avg_sq"].numpy() for q in ps])
        for name, want in (("p", want_p), ("m", want_m), ("v", want_v)):
            err = np.abs(got[name] - want).max()
            assert err <= TOL64 * np.abs(want).max(), (step, name, err)
        p, m, v = got["p"], got["m"], got["v"]
    assert int(opt.state[ps[0]]["step"]) == 3


def _walk_f32(c, lr=R.LR, beta1=R.BETA1, beta2=R.BETA2, eps=R.EPS):
    """include/rmav_ppo.h's lines in NumPy fp32 (every NumPy fp32 operation, sqrt and divide included, is correctly rounded)"""
    f = np.float32
    g = c["grad"] * f(c["grad_scale"])
    norm = f(np.sqrt((g.astype(np.float64) ** 2).sum()))
    ratio = f(c["max_grad_norm"]) / (norm + f(1e-6))
    coef = f(1.0) if ratio >= 1.0 else ratio
    gh = g * coef
    m = c["m"] + (f(1.0) - f(beta1)) * (gh - c["m"])
    v = f(beta2) * c["v"] + (f(1.0) - f(beta2)) * (gh * gh)
    step_size = f(lr / (1.0 - beta1 ** c["step"]))
    bc2_sqrt = f(np.sqrt(1.0 - beta2 ** c["step"]))
    p = c["p"] - step_size * (m / (np.sqrt(v) / bc2_sqrt + f(eps)))
    return dict(p=p, m=m, v=v, norm=norm, coef=coef)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("kind", sorted(R.KINDS))
def test_an_fp32_walk_through_the_lines_sits_inside_the_bound(kind, shared):
    for scenario in R.SCENARIOS:
        c = R.adam_case(kind, shared, scenario)
        with np.errstate(all="ignore"):
            got = _walk_f32(c)
        ref = R.adam(c["grad"], c["p"], c["m"], c["v"], c["step"], max_grad_norm=c["max_grad_norm"], grad_scale=c["grad_scale"])
        for name in ("p", "m", "v", "norm", "coef"):
            x = R.excess(got[name], ref[name], ref["bound_" + name])
            assert x <= 1.0, (scenario, name, x)
        if scenario == "one_nan":
            assert all(np.isnan(ref[name]).all() for name in ("p", "m", "v", "norm", "coef"))
        if scenario == "huge_no_clip":
            assert np.isinf(ref["v"]).all() and np.array_equal(ref["p"], c["p"].astype(np.float64))
    for which in R.ADV_INPUTS:
        for B in (2, 257, 2125):
            x = R.adv_input(which, B)
            ref, bound = R.adv_moments(x)
            std = np.float32(np.std(x.astype(np.float64), ddof=1))
            got = [np.float32(x.astype(np.float64).mean()), np.float32(1.0) / (std + np.float32(1e-8))]
            assert R.excess(got, ref, bound) <= 1.0, (which, B)


def _worst_excess(mutant, seed):
    """the largest excess of the mutant's outputs over the asserted bound, over the inputs of test_gpu_optim.py"""
    worst = 0.0
    if mutant in R.MOMENT_MUTANTS:
        for which in R.ADV_INPUTS:
            for B in (2, 63, 2125):
                x = R.adv_input(which, B, seed)
                ref, bound = R.adv_moments(x)
                bad, _ = R.adv_moments(x, mutant=mutant)
                worst = max(worst, R.excess(bad, ref, bound))
        return worst
    for shared in (False, True):
        for scenario in R.FINITE_SCENARIOS:
            c = R.adam_case("quad3d", shared, scenario, seed)
            kw = dict(max_grad_norm=c["max_grad_norm"], grad_scale=c["grad_scale"])
            ref = R.adam(c["grad"], c["p"], c["m"], c["v"], c["step"], **kw)
            bad = R.adam(c["grad"], c["p"], c["m"], c["v"], c["step"], mutant=mutant, **kw)
            for name in ("p", "m", "v", "norm", "coef"):
                worst = max(worst, R.excess(bad[name], ref[name], ref["bound_" + name]))
    return worst


def test_every_mutant_leaves_the_bound():
    """R.SEED = 0 is the first seed tried: every mutant clears 10 x there."""
    assert len(R.MUTANTS) >= 10
    got = {mutant: _worst_excess(mutant, R.SEED) for mutant in R.MUTANTS}
    print("optim-mutants", {k: f"{v:.3g}" for k, v in got.items()})
    assert all(v >= 10.0 for v in got.values()), got


def test_fused_optimizer_needs_the_fused_learner():
    from gym_reinmav_amd.ppo import PPO, MlpPolicy

    pol = MlpPolicy(10, 4)
    with pytest.raises(ValueError, match="fused_optimizer=True needs fused_learner=True"):
        PPO(pol, fused_optimizer=True)
    assert PPO(pol).fused_optimizer is False

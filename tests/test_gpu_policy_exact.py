"""The in-kernel policy actors against the quantisation-exact fp64 restatement (oracle/policy_ref.py): every mean row and the value of
every env inside the reference's own per-output bound - fp32 accumulation error plus activations that may round either way - with no
global scale factor.  The inputs (policies, start states) are those of tests/test_policy_ref_host.py, which proves on them that six
arithmetic mutants leave this bound; launches of T = 2 steps and at most 300 envs.

Each case prints a line `EXACT actor kind n case t=.. ratio=.. undecided=.. acc=..`: the largest |kernel - ref| / bound, the share of
envs with undecided activations and, where every operand of the output layer is exact (no undecided activation, no f16-subnormal
operand), the largest |kernel - ref| / (2^-24 (sum |a||x| + |b|)) - the accumulation constant the hardware showed, against the
worst-case C = 132 the bound uses (profiles/r13/policy_exactness.md records them)."""
import copy
import math

import numpy as np
import pytest

import policy_ref as R
from test_policy_ref_host import ACTORS, SHAPES, case_inputs, cases_of, family, huge_envs, reference

pytestmark = pytest.mark.gpu

T = 2
# fp32 / bf16 actors have no deterministic launch: logstd = -60 instead, |act - mean| <= 6.5 e^-60 (Box-Muller on 24-bit uniforms: |z| < 6.5)
NOISE = 6.5 * math.exp(-60.0)


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available()
    import gym_reinmav_amd as g

    return g


def _launch(G, actor, kind, n, case):
    """One T-step launch of the case: (obs [T + 1, nS, n], mean [T, nA, n], val [T + 1, n], normaliser tables or None, slack on the mean)."""
    import torch
    from gym_reinmav_amd.obs_norm import RunningObsNorm
    from gym_reinmav_amd.ppo import FusedPolicyCollector

    cpu_pol, _, s0, _ = case_inputs(family(actor), kind, n, case)
    # the action rule (deterministic=True) runs the fp32 matrix-core and the f16 actors of the four quadrotor kinds
    det = actor in ("fp32_mfma", "f16", "f16_shared") and kind != "reinmav"
    pol = copy.deepcopy(cpu_pol).cuda()
    if not det:
        with torch.no_grad():
            pol.logstd.fill_(-60.0)
    env = G.BatchedQuadrotor(kind, n, seed=33)
    if actor == "bf16_1w":
        env.set_tuning(policy_pair=0)
    env.set_state(s0)
    tables = None
    if case == "norm":   # statistics far from the identity, clip = 2: as _policy(..., variant="obs_norm") of test_gpu_action_rule.py
        torch.manual_seed(2)
        on = RunningObsNorm(env.nS, f"cuda:{env.device}", clip=2.0)
        on.update(torch.randn(64, env.nS, n, device="cuda") * 1.7 + 0.4, env=env)
        pol.obs_norm = on
    col = FusedPolicyCollector(env, pol, T, f32_mfma=(False if actor == "fp32" else None), bf16_mfma=actor.startswith("bf16"),
                               f16_mfma=(actor == "f16"), deterministic=det)
    assert col.actor == ("bf16" if actor == "bf16_1w" else actor)
    col.collect()
    torch.cuda.synchronize()
    if case == "norm":
        tables = (on.mean_f.cpu().numpy(), on.rstd_f.cpu().numpy(), float(on.clip_f.cpu().reshape(-1)[0]))
        assert tables[2] == 2.0 and (tables[1] != 1.0).all()
    out = col.obs.cpu().numpy(), col.act.cpu().numpy(), col.val.cpu().numpy()
    env.close()
    assert np.array_equal(out[0][0], s0.T)   # the stored first observation IS the state that was set
    return out + (tables, 0.0 if det else NOISE)


CONFIGS = [(a, k, n, c) for a in ACTORS for k, n in SHAPES for c in cases_of(a, k)]


@pytest.mark.parametrize("actor,kind,n,case", CONFIGS)
def test_actor_within_the_reference_bound(G, actor, kind, n, case):
    """|kernel - reference| <= bound for every env and every output row: the means and the value at t = 0, in the dense and the
    normalised cases also at t = 1 and the value of the last observation.  huge: the envs with a 3e4 and a 1e30 component give finite
    outputs inside their bound (f16: the input saturates at 65504), and every other env of the launch stays inside its ordinary one."""
    fam = family(actor)
    _, nets, _, _ = case_inputs(fam, kind, n, case)
    obs, mean, val, tables, slack = _launch(G, actor, kind, n, case)
    nA = mean.shape[1]
    steps = (0, 1, 2) if case in ("dense", "dense_wide", "norm") else (0,)
    failures = []
    for t in steps:
        res = reference(fam, kind, n, case) if (t == 0 and tables is None) else R.ACTORS[fam](nets, obs[t], norm=tables)
        cols = slice(0, nA + 1) if t < T else slice(nA, nA + 1)           # val[T]: the value of the last observation only
        y = np.concatenate([mean[min(t, T - 1)].T, val[t][:, None]], axis=1).astype(np.float64)[:, cols]
        ref, bound = res.y[:, cols], res.bound[:, cols].copy()
        bound[:, :-1] += slack
        diff = np.abs(y - ref)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(np.isfinite(bound), diff / bound, 0.0)
            exact = (res.undecided[:, cols] == 0) & (res.subnormal[:, cols] == 0) & np.isfinite(diff)
            acc = diff / (R.U * res.scale[:, cols])
        print(f"EXACT {actor} {kind} {n} {case} t={t} ratio={np.nanmax(ratio):.4f} undecided={float((res.undecided.max(1) > 0).mean()):.3f} "
              f"acc={(acc[exact].max() if exact.any() else float('nan')):.3f} exact_outputs={int(exact.sum())} max_bound={np.nanmax(bound):.3g} "
              f"max_abs_y={np.abs(ref[np.isfinite(ref)]).max():.3g}")
        bad = ~(diff <= bound)
        if t == 0 and case == "huge":
            h = huge_envs(n)
            assert np.isfinite(y[h]).all() and np.isfinite(ref[h]).all(), "a huge state must saturate, not turn the outputs into inf / NaN"
        for e, r in zip(*np.nonzero(bad)):
            failures.append(f"t={t} env {e} row {r}: kernel {y[e, r]:.9g} ref {ref[e, r]:.9g} |d| {diff[e, r]:.3g} > bound {bound[e, r]:.3g}")
    assert not failures, f"{len(failures)} outputs outside the bound, e.g. " + "; ".join(failures[:6])

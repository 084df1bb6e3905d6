"""The sampling half of the in-kernel policy against its fp64 restatement (oracle/sample_ref.py): the stored action fma(std, z, mean) and
the log-probability of EVERY env, step and component inside the reference's own bound - 4 x the first-order propagation of the documented
ulp errors of logf / sqrtf / sincospif / expf, plus policy_ref's bound of the mean - for every actor, kind, variant kernel, counter
width and end of the 24-bit uniforms.  The inputs are those of tests/test_sample_ref_host.py, which proves on them that the listed
arithmetic mutants land more than a decade outside this bound.  Launches of T = 5 steps and at most 300 envs.

A zero-head policy (zero action-head weight, bias B3) makes the mean B3 whatever the observation, so the comparison holds at every
step, through resets, without a reference of the dynamics.

Each case prints `SAMPLE actor kind n variant ratio_act=.. ratio_logp=.. max|z|=..`: the worst |kernel - ref| / bound of the launch
(profiles/r18/policy_sampling.md records them)."""
import copy

import numpy as np
import pytest

import noise_edges as E
import sample_ref as S
from test_policy_ref_host import SHAPES, case_inputs, family, reference
from test_sample_ref_host import (ACTORS, B3, BASE, LATE_T0, SEED, T, WIDE_BASE, dims, edge_launch, exact_zero_components, logstd_of, mean_reference,
                                  noise_grid, plain_cases, zero_head_policy)
from util import random_cases

pytestmark = pytest.mark.gpu

H = 2                      # the time limit of the tl / tl_boot variants: every env ends at least two episodes inside T = 5 steps
CLIP = (-0.05, 0.05)       # binds on most components (|B3| >= 0.09, std >= 0.3)
# the actuator of the `al` / `all8` variants, per action count: one time constant per component (one of them: no lag)
UPPER = {"ds": ("disturbance",), "sn": ("sensor_noise",), "al": ("actuator",), "ss": ("start_state",), "tc": ("termination",),
         "all8": ("disturbance", "sensor_noise", "actuator", "start_state", "termination", "reward")}
UPPER_TAUS = {2: (0.01, 0.02), 4: (0.01, 0.02, 0.015, 0.0)}
UPPER_INIT = {2: (1.5, -0.25), 4: (1.5, -0.25, 0.125, 0.0)}


@pytest.fixture(scope="module")
def G(built):
    import torch

    assert torch.cuda.is_available()
    import gym_reinmav_amd as g

    return g


def _launch(G, actor, kind, n, variant="plain", group=None, base=BASE, t0=0, steps=T):
    """One launch of `steps` steps: (act [steps, n, nA], logp [steps, n]) as fp32 host arrays."""
    import torch
    from gym_reinmav_amd.obs_norm import RunningObsNorm
    from gym_reinmav_amd.ppo import FusedPolicyCollector

    kw = {}
    if variant in ("tl", "tl_boot", "all8"):
        kw["max_episode_steps"] = H
    if variant in ("ranged", "all8"):
        kw["randomize"] = {"mass": (0.8, 1.25)}
    if variant in ("skip3", "all8"):
        kw["frame_skip"] = 3
    if variant in ("reward", "all8"):
        kw["reward"] = G.TrackingReward(alive=1.0, w_pos=1.0, w_vel=0.1, w_act=0.01, terminal=-10.0)
    # the five upper rungs of the feature ladder, one at a time and (all8) on top of each other and of the four lower features
    if variant in ("ds", "all8"):
        kw["disturbance"] = G.Disturbance(wind=((-1.0, 1.0), (-0.5, 0.75), (0.0, 0.5)), gust=(0.5, 0.25, 0.125), hold=3)
    if variant in ("sn", "all8"):
        kw["sensor_noise"] = G.SensorNoise(0.25)
    if variant in ("al", "all8"):
        kw["actuator"] = G.Actuator(UPPER_TAUS[dims(kind)[1]], init=UPPER_INIT[dims(kind)[1]])
    if variant in ("ss", "all8"):
        kw["start_state"] = G.StartState(-0.75, 0.75)
    if variant in ("tc", "all8"):
        d = 2 if kind.startswith("quad2d") else 3
        kw["termination"] = G.Termination(pos_lo=(-0.97,) * d, pos_hi=(0.97,) * d, max_tilt=0.5 if d == 2 else 1.6)
    env = G.BatchedQuadrotor(kind, n, seed=SEED, env_id_base=base, **kw)
    if t0:
        env.step_count = t0
    assert env.step_count == t0
    if actor == "bf16_1w":
        env.set_tuning(policy_pair=0)
    if group is not None:
        env.set_tuning(pair_group=group)
    pol = copy.deepcopy(zero_head_policy(family(actor), kind)).cuda()
    if kind == "reinmav":   # spread the envs out (they all start from the same init state)
        env.set_state(env.get_state() + np.random.RandomState(0).normal(scale=0.1, size=(n, 13)).astype(np.float32))
    else:
        env.set_state(random_cases(kind, n, seed=5)[0])
    for feature in UPPER.get(variant, ()):
        assert getattr(env, feature) is not None, (variant, feature)
    if variant == "norm":
        torch.manual_seed(2)
        on = RunningObsNorm(env.nS, f"cuda:{env.device}", clip=2.0)
        on.update(torch.randn(64, env.nS, n, device="cuda") * 1.7 + 0.4, env=env)
        pol.obs_norm = on
    col = FusedPolicyCollector(env, pol, steps, f32_mfma=(False if actor == "fp32" else None), bf16_mfma=actor.startswith("bf16"),
                               f16_mfma=(actor == "f16"), bootstrap_truncated=(variant in ("tl_boot", "all8")), clip_actions=(CLIP if variant == "clip" else False))
    assert col.actor == ("bf16" if actor == "bf16_1w" else actor)
    col.collect()
    torch.cuda.synchronize()
    assert env.step_count == t0 + steps     # frame skip: the counter advances per agent step
    act, logp, done = col.act.cpu().numpy().transpose(0, 2, 1), col.logp.cpu().numpy(), col.done.cpu().numpy()
    if variant in ("tl", "tl_boot", "all8"):
        assert (done.sum(0) >= 2).all()   # the comparison runs through two resets of every env (terminated, or truncated after H steps)
    env.close()
    return act, logp


def _check(label, act, logp, smp, z):
    """Every (t, env, component) inside the bound; prints the SAMPLE line.  Returns the failures as text."""
    assert act.shape == smp.act.shape and logp.shape == smp.logp.shape, (act.shape, smp.act.shape)
    da, dl = np.abs(act.astype(np.float64) - smp.act), np.abs(logp.astype(np.float64) - smp.logp)
    with np.errstate(invalid="ignore", divide="ignore"):
        ra = np.where(smp.bound_act > 0, da / smp.bound_act, np.where(da == 0, 0.0, np.inf))
        rl = dl / smp.bound_logp
    nA = act.shape[-1]
    print(f"SAMPLE {label} ratio_act={np.nanmax(ra):.4f} ratio_logp={np.nanmax(rl):.4f} max|z|={np.abs(z[..., :nA]).max():.3f}")
    assert np.isfinite(act).all() and np.isfinite(logp).all(), label
    bad = [f"act t={t} env {e} c={c}: {act[t, e, c]:.9g} ref {smp.act[t, e, c]:.9g} |d| {da[t, e, c]:.3g} > {smp.bound_act[t, e, c]:.3g}"
           for t, e, c in zip(*np.nonzero(~(da <= smp.bound_act)))]
    bad += [f"logp t={t} env {e}: {logp[t, e]:.9g} ref {smp.logp[t, e]:.9g} |d| {dl[t, e]:.3g} > {smp.bound_logp[t, e]:.3g}"
            for t, e in zip(*np.nonzero(~(dl <= smp.bound_logp)))]
    return bad


def _reference(actor, kind, n, base=BASE, t0=0):
    nA = dims(kind)[1]
    mean, mb = mean_reference(family(actor), kind)
    z, _, bz = noise_grid(base, n, t0)
    return S.sample(mean, mb, logstd_of(nA), 1.0, z, bz, nA), z


# ---- a. every draw of every actor and variant -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("actor,kind,n,variant,group", plain_cases())
def test_every_draw_is_inside_the_bound(G, actor, kind, n, variant, group):
    """clip: the stored action stays unclipped and logp is that of the unclipped one (the reference knows no clip); skip3: the noise
    counter advances per agent step; tl / tl_boot: through two resets of every env."""
    act, logp = _launch(G, actor, kind, n, variant, group)
    smp, z = _reference(actor, kind, n)
    if variant == "clip":
        assert ((act < CLIP[0]) | (act > CLIP[1])).mean() > 0.5
    bad = _check(f"{actor} {kind} {n} {variant}{'' if group is None else f'/g{group}'}", act, logp, smp, z)
    assert not bad, f"{len(bad)} outside the bound, e.g. " + "; ".join(bad[:6])


# ---- b. counter width -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("actor", ["fp32_mfma", "bf16", "f16_shared"])
@pytest.mark.parametrize("base,t0", [(WIDE_BASE, 0), (BASE, LATE_T0[0]), (BASE, LATE_T0[1])])
def test_wide_counters(G, actor, base, t0):
    """env ids above 2^40; a step counter that crosses 2^32 inside the launch (bits 32..47 of t reach the counter word c3); one that
    crosses 2^48 (c3 holds bits 32..47 of t: the draw continues with those bits back at zero)."""
    kind, n = "quad3d", 65
    act, logp = _launch(G, actor, kind, n, base=base, t0=t0)
    smp, z = _reference(actor, kind, n, base, t0)
    bad = _check(f"{actor} {kind} {n} base={base},t0={t0}", act, logp, smp, z)
    assert not bad, f"{len(bad)} outside the bound, e.g. " + "; ".join(bad[:6])


# ---- c. the ends of the 24-bit uniforms -------------------------------------------------------------------------------------------------
EDGE_GROUPS = sorted({en[0] for en in E.EDGES}) + ["wide_env", "late_t"]


def _entries(group):
    if group == "wide_env":
        return list(enumerate(E.EDGES_WIDE_ENV))
    if group == "late_t":
        return list(enumerate(E.EDGES_LATE_T))
    return [(i, en) for i, en in enumerate(E.EDGES) if en[0] == group]


@pytest.mark.parametrize("actor", ["fp32", "fp32_mfma", "bf16", "f16", "f16_shared"])
@pytest.mark.parametrize("group", EDGE_GROUPS)
def test_edges_of_the_uniforms(G, actor, group):
    """One 65-env launch per edge entry (and kind: quadrotor3d always, quadrotor2d as well where the entry is in the first pair of
    words, which is all a 2-action kind stores), the entry at lane j of step s.  Everything finite and inside the bound; a component
    the spec makes exactly zero stores the mean's bits; u1 = 1 on a 2-action kind stores the launch's logp0."""
    failures = []
    for i, entry in _entries(group):
        name, w, _, env_id, t = entry
        base, t0, j, s = edge_launch(i, entry)
        for kind in (("quad3d", "quad2d") if w < 2 else ("quad3d",)):
            nA = dims(kind)[1]
            act, logp = _launch(G, actor, kind, 65, base=base, t0=t0)
            smp, z = _reference(actor, kind, 65, base, t0)
            failures += _check(f"{actor} {kind} 65 edge:{name}/r{w}/lane{j}/step{s}", act, logp, smp, z)
            for c in exact_zero_components(entry):
                assert z[s, j, c] == 0.0
                if c < nA and act[s, j, c].tobytes() != B3[c].tobytes():
                    failures.append(f"{name} r{w} env {env_id} t {t}: component {c} is exactly zero in the spec, stored {act[s, j, c]!r} is not the mean {B3[c]!r}")
            if name == "u1_one" and nA == 2:
                d = abs(float(logp[s, j]) - smp.logp0)
                if not d <= smp.bound_logp0:
                    failures.append(f"{name} r{w} env {env_id} t {t}: logp {logp[s, j]!r} is not logp0 {smp.logp0!r} (|d| {d:.3g} > {smp.bound_logp0:.3g})")
    assert not failures, f"{len(failures)} failures, e.g. " + "; ".join(failures[:6])


# ---- d. dense means, one step -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("actor", ACTORS)
@pytest.mark.parametrize("kind,n", SHAPES)
def test_dense_policy_sample_is_inside_both_bounds(G, actor, kind, n):
    """The `dense` policy of tests/test_policy_ref_host.py (action head x 20, logstd 0) run stochastically from its start states: at
    t = 0 the stored action is inside policy_ref's own bound of the mean plus the noise part of bound_act, per env and component."""
    import torch
    from gym_reinmav_amd.ppo import FusedPolicyCollector

    fam = family(actor)
    cpu_pol, _, s0, _ = case_inputs(fam, kind, n, "dense")
    pol = copy.deepcopy(cpu_pol).cuda()
    nA = dims(kind)[1]
    assert float(pol.logstd.abs().max()) == 0.0
    env = G.BatchedQuadrotor(kind, n, seed=SEED, env_id_base=BASE)
    if actor == "bf16_1w":
        env.set_tuning(policy_pair=0)
    env.set_state(s0)
    col = FusedPolicyCollector(env, pol, 1, f32_mfma=(False if actor == "fp32" else None), bf16_mfma=actor.startswith("bf16"), f16_mfma=(actor == "f16"))
    col.collect()
    torch.cuda.synchronize()
    act, logp = col.act.cpu().numpy().transpose(0, 2, 1), col.logp.cpu().numpy()
    env.close()
    res = reference(fam, kind, n, "dense")
    z, _, bz = noise_grid(BASE, n, 0, 1)
    smp = S.sample(res.mean[None], res.bound[None, :, :nA], np.zeros(nA, np.float32), 1.0, z, bz, nA)
    bad = _check(f"{actor} {kind} {n} dense", act, logp, smp, z)
    assert not bad, f"{len(bad)} outside the bound, e.g. " + "; ".join(bad[:6])


# ---- e. one stream ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["quad3d", "quad2d_sl"])
def test_every_route_stores_the_same_bits(G, kind):
    """Under the zero-head policy the mean is B3 in every actor (a zero weight adds exact zeros) and std = expf(logstd) in every kernel,
    so the stored action and the log-probability are the same statement on the same operands everywhere: the two fp32 actors, the bf16
    pair and one-wavefront routes, the f16 and shared-trunk pairs at 1 and 4 pairs per workgroup, and the time-limited, bootstrap,
    normalised, ranged, frame-skip, tracking-reward and clipped kernels of the three actors that have them store identical bits.  So do
    the kernels of the five upper rungs of the feature ladder (ds: disturbance, sn: sensor noise, al: actuator lag, ss: start-state
    ranges, tc: termination spec - whose noise, lag and resets change every observation but not the zero-head mean) and all8, every
    feature at once under a time limit with the bootstrap term, at the automatic choice and at 1 and 4 pairs per workgroup."""
    n = 130
    ref = _launch(G, "fp32", kind, n)
    routes = [(a, "plain", None) for a in ACTORS[1:]] + [(a, "plain", g) for a in ("bf16", "f16", "f16_shared") for g in (1, 4)]
    routes += [(a, v, None) for a in ("fp32_mfma", "f16", "f16_shared") for v in ("tl", "tl_boot", "norm", "ranged", "skip3", "reward", "clip")]
    upper = ("fp32_mfma", "f16", "f16_shared")
    routes += [(a, v, None) for a in upper for v in ("ds", "sn", "al", "ss", "tc", "all8")] + [(a, "all8", g) for a in upper for g in (1, 4)]
    differ = []
    for actor, variant, group in routes:
        act, logp = _launch(G, actor, kind, n, variant, group)
        if act.tobytes() != ref[0].tobytes() or logp.tobytes() != ref[1].tobytes():
            differ.append(f"{actor}/{variant}/{group}: {int((act != ref[0]).sum())} actions, {int((logp != ref[1]).sum())} log-probabilities differ from the fp32 actor's")
    assert not differ, "; ".join(differ)

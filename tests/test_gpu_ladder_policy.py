"""The policy side of the feature ladder on the GPU: the in-kernel actors (rmav_launch_{policy, sensor_policy, actuator_policy,
start_policy, term_policy}_rollout, three actor kernels each) on handles with EVERY rung up to theirs switched on, where the
per-feature policy tests add one upper feature to test_gpu_disturbance.POLICY_CONFIGS and leave the lower slots of the rung's argument
list empty.  upto(G, kind, n, top) builds such a handle from test_gpu_ladder.all_eight's specs: a time limit, a frame skip, a mass
range and the tracking reward always, then disturbance, sensor noise, actuator lag, start-state ranges and the termination spec up to
and including `top`; upto(.., "term") IS all_eight.  Every collect runs the normalised bootstrap kernels (a RunningObsNorm far from the
identity, bootstrap_truncated=True) with clip_actions=True under max_episode_steps = H.

No CPU twin composes all eight features with an in-kernel policy, so the checks are
  1. replay: the stored actions, clipped on the host, through rollout(mode="buffer") on a twin - every array the dynamics own, bit for bit;
  2. 1, 2 and 4 pairs per workgroup store the same bits (300 envs: two workgroups at 4, the second one ragged);
  3. one T-step launch is T one-step launches, bit for bit in every array and the tail;
  4. the actor read what it stored: val[k] inside oracle/policy_ref.py's own bound of the value of the stored noisy raw obs[k], boot on
     truncated lanes inside the bound of the value at the terminal observation step_final reports on a third twin, and - a second,
     deterministic launch - the stored action inside the bound of the mean.  The bound is the reference's own
     (tests/test_policy_ref_host.py shows that its mutants leave it); nothing is widened.

The policy is test_gpu_disturbance.policy_of(norm=True) with the action head's bias at the kind's hover command and a log standard
deviation per component, and the value head's last layer x 4 (as test_gpu_sensor_noise.policy_of: a value that read the true state
instead of the noisy row must leave the f16 actors' bound too; item 4 prints the share of lanes where it does).  Chosen on the GPU
(profiles/r28/ladder_policy.md has the runs):
  quadrotor2d             bias (0.98, 0), logstd (-3, 2.5):   thrust 0.98 +- 0.05 of 10 g; rates of std 12 rad/s, clipped to the box's
                          +-10: a tilt walk of up to 0.2 rad per agent step against the limit of 0.5 from starts within 0.25
  quadrotor3d_slungload   bias (9.8, 0, 0, 0), logstd (-3, 1.5, 1.5, 0):  term_ref.commands' mean thrust; rates of std 4.5 rad/s.  About
                          every second fresh state (quaternion components in +-0.75) lies beyond the tilt limit of 1.6 rad and ends with
                          its first step whatever the action
Counts observed at top = term in one launch of T x n env-steps (the three actors and every pair group alike: the clipped actions of
a zero-gain head differ between them by roundings that moved no episode end):
  quadrotor2d             n = 65: 72 episode ends, 55 truncations, 17 terminations, largest reset count 4;  n = 300: 332 / 260 / 72 / 4
  quadrotor3d_slungload   n = 65: 158 episode ends, 63 truncations, 95 terminations, largest reset count 6;  n = 300: 785 / 270 / 515 / 9
  item 4, the deterministic launch behind the sampled one (n = 65): quadrotor2d 123 truncations, quadrotor3d_slungload 87 - 178 and 150
  truncated lane-steps for the boot check

The truncation count.  With T = 8 and H = 5 an env is truncated at most once per launch (the second truncation of an env would fall on
step 10 at the earliest), so n is the ceiling of a launch's count, reached only if every env has an episode that starts inside the
first three steps and lasts; of quadrotor3d_slungload's envs one in eight has none (three fresh states in a row beyond the tilt limit).
The condition `at least n truncated lane-steps for the boot check` is therefore asserted where the boot check is, in item 4, over the
two launches it checks boot on (stochastic, then deterministic: 16 steps); every test asserts a truncation, a rule termination and a
reset count of 2 inside its own launch, and prints its counts."""
import numpy as np
import pytest

import disturbance_ref as D
import policy_ref as PR
import test_gpu_disturbance as TD
from test_gpu_actuator import INIT, TAUS, u8
from test_gpu_disturbance import ACTORS, host, policy_of, same
from test_gpu_ladder import HOVER, START, H, N, T, all_eight
from test_gpu_termination import G, make  # noqa: F401  (G: the module fixture)
from test_policy_ref_host import family, nets_of
from util import NA

pytestmark = pytest.mark.gpu

F32 = np.float32
KINDS2 = ("quad2d", "quad3d_sl")     # the smallest and the largest state, as test_gpu_ladder.py
RUNGS = ("disturbance", "sensor", "actuator", "start", "term")
BIAS = {"quad2d": (HOVER["quad2d"], 0.0), "quad3d_sl": (9.8, 0.0, 0.0, 0.0)}      # quad3d_sl: the mean thrust of term_ref.commands
LOGSTD = {"quad2d": (-3.0, 2.5), "quad3d_sl": (-3.0, 1.5, 1.5, 0.0)}
TAIL = ("state", "sbd", "rc", "t")


def upto(G, kind, n, top):
    """A handle with the four lower features and every upper rung up to and including `top`, from all_eight's specs."""
    k = RUNGS.index(top)
    if top == "term":
        return all_eight(G, kind, n)
    kw = dict(max_episode_steps=H, randomize={"mass": (0.8, 1.2)}, frame_skip=2, reward=True, disturbance=TD.dist(G, D.SPEC))
    if k >= 1:
        kw["sensor_noise"] = G.SensorNoise(0.25)
    if k >= 2:
        kw["actuator"] = G.Actuator(TAUS[NA[kind]], init=INIT[NA[kind]])
    if k >= 3:
        kw["start_state"] = G.StartState(-START[kind], START[kind])
    return make(G, kind, n, term=None, **kw)


def switched_on(env, top):
    k = RUNGS.index(top)
    want = [True, k >= 1, k >= 2, k >= 3, k >= 4]
    have = [x is not None for x in (env.disturbance, env.sensor_noise, env.actuator, env.start_state, env.termination)]
    return have == want and env.reward is not None and env.frame_skip == 2 and env.max_episode_steps == H


def ladder_policy(env, actor, kind):
    import torch

    pol = policy_of(env, actor, norm=True)
    with torch.no_grad():
        pol.pi[-1].bias.copy_(torch.tensor(BIAS[kind]))
        pol.logstd.copy_(torch.tensor(LOGSTD[kind]))
        pol.vf[-1].weight.mul_(4.0)
    return pol


def collector(env, pol, actor, steps, deterministic=False):
    from gym_reinmav_amd.ppo import FusedPolicyCollector

    col = FusedPolicyCollector(env, pol, steps, f16_mfma=(actor == "f16"), bootstrap_truncated=True, clip_actions=True, deterministic=deterministic)
    assert col.actor == actor
    return col


def arrays(col):
    import torch

    torch.cuda.synchronize()
    return {key: getattr(col, key).cpu().numpy().copy() for key in ("act", "obs", "rew", "done", "logp", "val", "boot", "trunc")}


def tail(env):
    out = dict(state=env.get_state(), sbd=env.get_sbd(), rc=env.get_reset_counts(), t=np.array([env.step_count]))
    if env.actuator is not None:
        out["m"] = env.actuator_state()
    return out


def launch(G, actor, kind, n, top, group=None):
    """One T-step launch of the ladder policy on a fresh upto handle -> every array the launch leaves and the handle's tail."""
    env = upto(G, kind, n, top)
    assert switched_on(env, top)
    if group is not None:
        env.set_tuning(pair_group=group)
    col = collector(env, ladder_policy(env, actor, kind), actor, T)
    col.collect()
    out = arrays(col)
    out.update(tail(env))
    env.close()
    return out


def clipped(env, act):
    """what clip_actions=True hands the dynamics"""
    return np.ascontiguousarray(np.clip(act, F32(env.params.act_lo), F32(env.params.act_hi)).astype(F32))


def counts(out, what, n, need=True):
    """Prints the episode-end counts of a launch; at top = term and n >= 65 both kinds of end and a second reset fall inside it."""
    done, trunc = u8(out["done"]).astype(bool), u8(out["trunc"]).astype(bool)
    c = dict(ends=int(done.sum()), trunc=int(trunc.sum()), term=int((done & ~trunc).sum()), rc=int(out["rc"].max()))
    print(f"LADDER-POLICY {what}: {c['ends']} episode ends in {done.shape[0]} x {n} env-steps, {c['trunc']} truncations, {c['term']} terminations; "
          f"largest reset count {c['rc']}")
    assert (trunc <= done).all()
    if need:
        assert c["trunc"] >= 1 and c["term"] >= 1 and c["rc"] >= 2, c
    return c


def replay(G, kind, n, top, out, what):
    """The stored actions, clipped on the host, in buffer mode on a twin from the same start: what the dynamics own, bit for bit."""
    twin = upto(G, kind, n, top)
    tr = twin.rollout(T, mode="buffer", actions=clipped(twin, out["act"]), layout="soa", want=("obs", "rew", "done"))
    same(tr["obs"], out["obs"][1:], f"{what}: obs"), same(tr["rew"], out["rew"], f"{what}: rew"), same(u8(tr["done"]), u8(out["done"]), f"{what}: done")
    back = tail(twin)
    twin.close()
    assert set(back) == {k for k in out if k in TAIL + ("m",)} and ("m" in back) == (RUNGS.index(top) >= 2)
    for key in back:
        same(back[key], out[key], f"{what}: {key}")
    done, trunc = u8(out["done"]).astype(bool), u8(out["trunc"]).astype(bool)
    assert not out["boot"][~trunc].any() and (trunc <= done).all(), "boot is exactly 0 wherever the step was not truncated"


# ---- 1. replay, every cumulative rung ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("actor", ACTORS)
@pytest.mark.parametrize("kind", KINDS2)
@pytest.mark.parametrize("top,n", [(top, N) for top in RUNGS] + [("term", 300), ("term", 1)])
def test_policy_rollouts_by_replay_on_cumulative_handles(G, actor, kind, top, n):
    assert N == 65 and T == 8 and H == 5
    out = launch(G, actor, kind, n, top)
    what = f"{actor} {kind} n={n} up to {top}"
    counts(out, what, n, need=(top == "term" and n >= 65))
    replay(G, kind, n, top, out, what)


# ---- 2. pairs per workgroup ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("actor", ("f16", "f16_shared"))
@pytest.mark.parametrize("kind", KINDS2)
def test_pairs_per_workgroup_store_the_same_bits(G, actor, kind):
    n = 300      # 150 pairs: two workgroups at 4 pairs per workgroup, the second one ragged
    outs = {g: launch(G, actor, kind, n, "term", group=g) for g in (1, 2, 4)}
    for g in (1, 2, 4):
        what = f"{actor} {kind} n={n} all eight, pair_group={g}"
        counts(outs[g], what, n)
        replay(G, kind, n, "term", outs[g], what)
        for key in outs[1]:
            same(outs[g][key], outs[1][key], f"{what} against pair_group=1: {key}")


# ---- 3. launch splitting ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("actor", ACTORS)
@pytest.mark.parametrize("kind", KINDS2)
def test_one_launch_equals_one_step_launches(G, actor, kind):
    n = N
    whole = launch(G, actor, kind, n, "term")
    counts(whole, f"{actor} {kind} n={n} all eight, one launch", n)
    env = upto(G, kind, n, "term")
    col = collector(env, ladder_policy(env, actor, kind), actor, 1)
    for k in range(T):
        col.collect()
        rec = arrays(col)
        for key in ("act", "rew", "done", "logp", "boot", "trunc"):
            same(whole[key][k], rec[key][0], f"{key}[{k}]")
        for key in ("obs", "val"):
            same(whole[key][k], rec[key][0], f"{key}[{k}]")
            same(whole[key][k + 1], rec[key][1], f"{key}[{k + 1}] behind step {k}")
        col.roll_over()
    back = tail(env)
    env.close()
    for key in back:
        same(back[key], whole[key], f"tail: {key}")


# ---- 4. the actor read what it stored ----------------------------------------------------------------------------------------------------
def tables_of(pol):
    on = pol.obs_norm
    tab = (on.mean_f.cpu().numpy(), on.rstd_f.cpu().numpy(), float(on.clip_f.cpu().reshape(-1)[0]))
    assert tab[2] == 2.0 and (tab[1] != 1.0).all()
    return tab


def worst(diff, bound, rows):
    """largest |kernel - ref| / bound over the rows; the rows outside the bound"""
    d, b = diff[rows], bound[rows]
    bad = ~(d <= b)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(np.isfinite(b) & (b > 0), d / b, 0.0)
    return (float(ratio.max()) if ratio.size else 0.0), int(bad.sum())


@pytest.mark.parametrize("actor", ACTORS)
@pytest.mark.parametrize("kind", KINDS2)
def test_the_actor_read_what_it_stored(G, actor, kind):
    """Prints `LADDER-EXACT actor kind launch: val=.. boot=.. mean=.. share=.. boot_share=..`: the worst |kernel - ref| / bound of the values,
    the bootstrap terms and (deterministic launch) the means; the share of lanes whose val[k] is OUTSIDE the bound of the value of the true
    pre-step state, and the share of truncated lanes whose boot[k] is outside the bound of the value of the next stored row (the fresh
    episode's observation) - what a net that read the wrong row would store; both shares are above one half."""
    n, fam, nA = N, family(actor), NA[kind]
    env, twin = upto(G, kind, n, "term"), upto(G, kind, n, "term")
    pol = ladder_policy(env, actor, kind)
    nets, tables = nets_of(pol), None
    ref = lambda o: PR.ACTORS[fam](nets, np.ascontiguousarray(o, F32), norm=tables)   # noqa: E731  (o: [nS, n])
    failures, truncated, missed, missed_boot = [], 0, [], []
    for name, det in (("sampled", False), ("deterministic", True)):
        col = collector(env, pol, actor, T, deterministic=det)
        col.collect()
        out = arrays(col)
        out.update(tail(env))
        if tables is None:
            tables = tables_of(pol)
        c = counts(out, f"{actor} {kind} n={n} all eight, {name}", n, need=not det)
        truncated += c["trunc"]
        u = clipped(env, out["act"])
        rv = rb = rm = 0.0
        for k in range(T + 1):
            res = ref(out["obs"][k])
            ratio, bad = worst(np.abs(out["val"][k].astype(np.float64) - res.y[:, nA]), res.bound[:, nA], np.ones(n, bool))
            rv = max(rv, ratio)
            if bad:
                failures.append(f"{name} val[{k}]: {bad} envs outside the bound, worst ratio {ratio:.3g}")
            if k == T:
                break
            if det:   # the stored action is the mean (act and logp stay those of the unclipped action)
                ratio, bad = worst(np.abs(out["act"][k].T.astype(np.float64) - res.y[:, :nA]), res.bound[:, :nA], np.ones(n, bool))
                rm = max(rm, ratio)
                if bad:
                    failures.append(f"{name} act[{k}]: {bad} components outside the bound of the mean, worst ratio {ratio:.3g}")
            # the third twin: the true pre-step state, and the terminal observation of the lanes whose episode ends with step k
            pre = twin.get_state()
            true = ref(pre.T)
            missed.append(~(np.abs(out["val"][k].astype(np.float64) - true.y[:, nA]) <= true.bound[:, nA]))
            o, r, d, fin, tr = twin.step_final(np.ascontiguousarray(u[k].T))
            same(host(o).T, out["obs"][k + 1], f"{name}: the twin's obs[{k + 1}]")
            same(u8(tr), u8(out["trunc"][k]), f"{name}: the twin's trunc[{k}]")
            lanes = u8(tr).astype(bool)
            if lanes.any():
                res = ref(host(fin).T)
                ratio, bad = worst(np.abs(out["boot"][k].astype(np.float64) - res.y[:, nA]), res.bound[:, nA], lanes)
                rb = max(rb, ratio)
                if bad:
                    failures.append(f"{name} boot[{k}]: {bad} of {int(lanes.sum())} truncated lanes outside the bound, worst ratio {ratio:.3g}")
                nxt = ref(out["obs"][k + 1])
                missed_boot.append(~(np.abs(out["boot"][k].astype(np.float64) - nxt.y[:, nA]) <= nxt.bound[:, nA])[lanes])
            assert not out["boot"][k][~lanes].any()
        print(f"LADDER-EXACT {actor} {kind} {name}: val={rv:.4f} boot={rb:.4f} mean={rm:.4f} share={float(np.mean(missed)):.3f} "
              f"boot_share={float(np.concatenate(missed_boot).mean()):.3f}")
    env.close(), twin.close()
    assert truncated >= n, (truncated, "truncated lane-steps for the boot check")
    assert float(np.mean(missed)) > 0.5 and float(np.concatenate(missed_boot).mean()) > 0.5, "the bound tells the stored rows from the others"
    assert not failures, f"{len(failures)} failures, e.g. " + "; ".join(failures[:6])

"""The feature ladder on the GPU, for the one case the per-feature tests do not combine: a handle with ALL eight switches set at once - a
parameter range, a frame skip, a tracking reward, a disturbance, sensor noise, actuator lag, a start-state spec and a termination spec -
under an episode time limit.  Such a handle runs the top rung's kernels (k_rollout_tc, k_step_tc) with every slot of their argument lists
taken from a real spec.  Three twin handles with the same seed are driven with the same action buffer: one fused ACT_BUFFER rollout, 8 single
steps and 8 rmav_step_final calls.  Observations, rewards, done bytes and the final state are bit-equal across the three (the step and the
rollout kernels round identically: DESIGN.md); no array is excluded.

This file drives the handle with buffered actions (mode="buffer" rollouts and single steps).  The policy side - the in-kernel actors of
FusedPolicyCollector on the same handle, and on every cumulative handle below it - is tests/test_gpu_ladder_policy.py, which takes
all_eight, N, T, H and the HOVER / START tables from here; the sampled draw on such handles is test_every_route_stores_the_same_bits of
tests/test_gpu_policy_sample.py (variants ds, sn, al, ss, tc, all8)."""
import disturbance_ref as D
import numpy as np
import pytest

import term_ref as R
import test_gpu_disturbance as TD
from test_gpu_actuator import INIT, TAUS, u8
from test_gpu_disturbance import host, same
from test_gpu_termination import G, make, term_of  # noqa: F401  (G: the module fixture)
from util import NA

pytestmark = pytest.mark.gpu

N, T, H = 65, 8, 5       # one full wavefront and a one-lane tail; a truncation and a reset fall inside the run
# Every second env holds its attitude at hover thrust, so that its episodes reach the time limit; the others turn until the tilt rule ends
# them.  quadrotor2d ends an episode at |v| > 2 m/s (the reference's rule, default reading), which term_ref.commands' thrust - five times
# the weight at that kind's thrust scale of 10 - passes within a few dynamics steps: its held envs get the hover command 0.98 and start
# states near the origin, whose tilt leaves the thrust nearly vertical (0.25 rad: at most 2.4 m/s^2 sideways, 1.2 m/s over the five agent
# steps of ten dynamics steps each; the mass range adds up to 2.5 m/s^2 along the thrust, the wind and the gust up to 1.5 m/s^2).
HOVER = {"quad2d": 0.98, "quad3d_sl": None}     # thrust command of the held envs (None: what term_ref.commands gives)
START = {"quad2d": 0.25, "quad3d_sl": 0.75}     # half-width of the start-state ranges


def all_eight(G, kind, n=N):
    return make(G, kind, n, term="spec", max_episode_steps=H, randomize={"mass": (0.8, 1.2)}, frame_skip=2, reward=True,
                disturbance=TD.dist(G, D.SPEC), sensor_noise=G.SensorNoise(0.25), actuator=G.Actuator(TAUS[NA[kind]], init=INIT[NA[kind]]),
                start_state=G.StartState(-START[kind], START[kind]))


@pytest.mark.parametrize("kind", ("quad2d", "quad3d_sl"))     # the smallest and the largest state
def test_all_eight_switches_rollout_steps_and_step_final_agree(G, kind):
    acts = R.commands(kind, N, T)
    acts[:, 1::2, 1:] = 0.0     # every second env holds its attitude: its episodes reach the time limit, the turning ones end by the rule
    if HOVER[kind] is not None:
        acts[:, 1::2, 0] = HOVER[kind]
    fused, steps, finals = all_eight(G, kind), all_eight(G, kind), all_eight(G, kind)
    for env in (fused, steps, finals):
        assert None not in (env.disturbance, env.sensor_noise, env.actuator, env.start_state, env.termination, env.reward) and env.frame_skip == 2
    same(fused.get_state(), steps.get_state(), "the twins start from the same state")
    tr = fused.rollout(T, mode="buffer", actions=acts, layout="aos", want=("obs", "rew", "done"))      # ONE fused launch
    one = [steps.step(acts[t]) for t in range(T)]
    fin = [finals.step_final(acts[t]) for t in range(T)]
    runs = {"fused": (host(tr["obs"]), host(tr["rew"]), u8(tr["done"]), fused.get_state())}
    for name, env, outs in (("single steps", steps, one), ("step_final", finals, fin)):
        runs[name] = (np.stack([host(x[0]) for x in outs]), np.stack([host(x[1]) for x in outs]), np.stack([u8(x[2]) for x in outs]), env.get_state())
    for name in ("single steps", "step_final"):
        for i, what in enumerate(("obs", "rew", "done", "final state")):
            same(runs[name][i], runs["fused"][i].astype(runs[name][i].dtype), f"{kind}, {name} against the fused rollout: {what}")
    done = runs["fused"][2].astype(bool)
    trunc = np.stack([u8(x[4]) for x in fin]).astype(bool)
    print(f"{kind}: {int(done.sum())} episode ends in {T} x {N} env-steps, {int(trunc.sum())} of them truncations, {int((done & ~trunc).sum())} terminations; "
          f"largest reset count {int(fused.get_reset_counts().max())}")
    assert (trunc <= done).all() and trunc.any(), "a truncation falls inside the run"
    assert (done & ~trunc).any() and fused.get_reset_counts().max() >= 2, "... and so do terminations and their resets"
    same(fused.get_reset_counts(), finals.get_reset_counts(), "reset counts")
    for env in (fused, steps, finals):
        env.close()

#!/usr/bin/env python3
"""Timings behind profiles/r21/start_state.md: what a handle with a start-state spec (rmav_set_start_state) pays for its route - the *_ss
kernels are the lagged bodies with the map behind every draw of a fresh state and a wave-uniform switch around the filter - against the
*_al kernels they are cut from, at 65 536 quadrotor3d envs.  Three handles of the SAME build (tools/isa_compare.py: the *_al kernels have
the parent commit's instruction streams):

  actuator                  actuator lag alone: the *_al kernels
  actuator+start_state      ... with a start spec: the *_ss kernels with the filter                  (against *_al)
  start_state               a start spec alone: the *_ss kernels with the filter switched off        (against *_al)

  (a) rollout   64-step random-action launches, trajectory (actions, obs, reward, done) stored into a cold ring of buffer sets (bench.py's
                method: >= 5 sets, > 1.5 GB)
  (b) step      rmav_step (device pointers, batch-major actions and obs)
  (c) policy    32-step in-kernel policy rollouts (FusedPolicyCollector, trajectory stored) of the three actors

The sides live in one process and alternate launch by launch so that clock and co-tenant drift hit them alike; every launch sits between
two HIP events (5 warm-up launches per side, then `--reps` timed ones per side), and the whole sequence runs `--passes` times; the table
has the median per side and pass, the spread over the passes and the ratios of the medians.

    python tools/start_state_ab.py [--out FILE] [--passes 3] [--reps 30] [--tau 0.05] [--spread 0.25]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reinmav-gym_amd"))
WARM = 5


def alternate(sides, reps):
    """sides {name: fn(i)} -> {name: sorted us per launch}, the sides taking turns"""
    import torch

    for i in range(WARM):
        for fn in sides.values():
            fn(i)
    ts = {name: [] for name in sides}
    for i in range(reps):
        for name, fn in sides.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(WARM + i)
            b.record()
            b.synchronize()
            ts[name].append(a.elapsed_time(b) * 1e3)
    return {name: sorted(v) for name, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--tau", type=float, default=0.05)
    ap.add_argument("--spread", type=float, default=0.25, help="every state component starts in [-spread, spread]")
    args = ap.parse_args()
    import torch

    import gym_reinmav_amd as g

    assert torch.cuda.is_available(), "a measurement needs the GPU"
    n, T = args.envs, 64
    lag = g.Actuator(args.tau)
    start = g.StartState(-args.spread, args.spread)
    SIDES = {"actuator": (True, False), "actuator+start_state": (True, True), "start_state": (False, True)}
    BASE_OF = {"actuator+start_state": "actuator", "start_state": "actuator"}

    def env(side):
        lagged, ranged = SIDES[side]
        return g.BatchedQuadrotor("quad3d", n, seed=1, actuator=lag if lagged else None, start_state=start if ranged else None)

    shapes = {}
    # (a) fused rollouts into a cold ring
    per_set = T * n * (4 * (4 + 10 + 1) + 1)
    R = max(5, -(-int(1.5e9) // per_set))
    ring = [{"actions": torch.zeros((T, 4, n), device="cuda"), "obs": torch.zeros((T, 10, n), device="cuda"), "rew": torch.zeros((T, n), device="cuda"),
             "done": torch.zeros((T, n), dtype=torch.uint8, device="cuda")} for _ in range(R)]
    want = ("actions", "obs", "rew", "done")
    shapes[f"rollout_random_{n}x{T}"] = (T, {side: (lambda i, e=env(side): e.rollout(T, mode="random", device_out=True, want=want, out=ring[i % R]))
                                             for side in SIDES})
    # (b) single steps
    act = torch.full((n, 4), 2.45, device="cuda")
    bufs = {side: (torch.zeros((n, 10), device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")) for side in SIDES}
    shapes[f"step_{n}"] = (1, {side: (lambda i, e=env(side), b=bufs[side]: e.step(act, out=b)) for side in SIDES})

    # (c) policy rollouts
    from gym_reinmav_amd.ppo import FusedPolicyCollector, MlpPolicy

    TP = 32
    for actor in ("fp32_mfma", "f16", "f16_shared"):
        cols = {}
        for side in SIDES:
            e = env(side)
            torch.manual_seed(3)
            pol = MlpPolicy(e.nS, e.nA, value_network="shared" if actor == "f16_shared" else "copy").cuda()
            cols[side] = FusedPolicyCollector(e, pol, TP, f16_mfma=(actor == "f16"))
        shapes[f"policy_{actor}_{n}x{TP}"] = (TP, {side: (lambda i, c=c: c.collect()) for side, c in cols.items()})

    res = {"device": torch.cuda.get_device_name(0), "envs": n, "reps_per_side_and_pass": args.reps, "passes": args.passes,
           "actuator": repr(lag), "start_state": repr(start), "shapes": {}}
    for tag, (steps, sides) in shapes.items():
        med = {name: [] for name in sides}
        for _ in range(args.passes):
            for name, ts in alternate(sides, args.reps).items():
                med[name].append(round(statistics.median(ts), 2))
        row = {name: {"median_us_by_pass": v, "median_us": round(statistics.median(v), 2), "spread_us": round(max(v) - min(v), 2),
                      "env_steps_per_s_G": round(n * steps / (statistics.median(v) * 1e-6) / 1e9, 3)} for name, v in med.items()}
        for name, base in BASE_OF.items():
            row[name][f"ratio_over_{base}"] = round(row[name]["median_us"] / row[base]["median_us"], 4)
        res["shapes"][tag] = row
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()

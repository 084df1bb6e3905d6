#!/usr/bin/env python3
"""Timings behind profiles/r22/termination.md: what a handle with a termination spec (rmav_set_termination) pays for its route - the *_tc
kernels are the bodies of a start-state spec with the rule behind every dynamics sub-step - against the *_ss kernels they are cut from, at
65 536 quadrotor3d envs.  Three handles of the SAME build (tools/isa_compare.py: the *_ss kernels have the parent commit's instruction
streams), all reset once, so that they run the same episodes:

  start_state               the identity start-state spec alone: the *_ss kernels
  termination               the all-infinite termination spec: the *_tc kernels, the same episodes        (against *_ss)
  hover_box                 the reference's hovering box (|x|, |y| <= 2, z >= 0.3): the *_tc kernels, whose episodes end more often - the
                            extra resets are workload, not kernel cost, so the done rate stands beside every ratio   (against *_ss)

  (a) rollout   64-step random-action launches, trajectory (actions, obs, reward, done) stored into a cold ring of buffer sets (bench.py's
                method: >= 5 sets, > 1.5 GB)
  (b) step      rmav_step (device pointers, batch-major actions and obs)
  (c) policy    32-step in-kernel policy rollouts (FusedPolicyCollector, trajectory stored) of the three actors

The sides live in one process and alternate launch by launch so that clock and co-tenant drift hit them alike; every launch sits between
two HIP events (5 warm-up launches per side, then `--reps` timed ones per side), and the whole sequence runs `--passes` times; the table
has the median per side and pass, the spread over the passes, the ratios of the medians and the share of env-steps that ended an episode.

    python tools/termination_ab.py [--out FILE] [--passes 3] [--reps 30]"""
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
    args = ap.parse_args()
    import torch

    import gym_reinmav_amd as g

    assert torch.cuda.is_available(), "a measurement needs the GPU"
    n, T = args.envs, 64
    inf = float("inf")
    SIDES = {"start_state": dict(start_state=g.StartState(-1.0, 1.0)), "termination": dict(termination=g.Termination()),
             "hover_box": dict(termination=g.Termination(pos_lo=(-2.0, -2.0, 0.3), pos_hi=(2.0, 2.0, inf)))}
    BASE_OF = {"termination": "start_state", "hover_box": "start_state"}
    dones = {}   # tag -> side -> the done bytes of the last launch (a device tensor)

    def env(side):
        e = g.BatchedQuadrotor("quad3d", n, seed=1, **SIDES[side])
        if "start_state" not in SIDES[side]:
            e.reset()   # (the start_state= keyword resets once: all three sides run from reset index 1)
        return e

    shapes = {}
    # (a) fused rollouts into a cold ring
    per_set = T * n * (4 * (4 + 10 + 1) + 1)
    R = max(5, -(-int(1.5e9) // per_set))
    ring = [{"actions": torch.zeros((T, 4, n), device="cuda"), "obs": torch.zeros((T, 10, n), device="cuda"), "rew": torch.zeros((T, n), device="cuda"),
             "done": torch.zeros((T, n), dtype=torch.uint8, device="cuda")} for _ in range(R)]
    want = ("actions", "obs", "rew", "done")
    rollers = {side: (lambda i, e=env(side): e.rollout(T, mode="random", device_out=True, want=want, out=ring[i % R])) for side in SIDES}
    shapes[f"rollout_random_{n}x{T}"] = (T, rollers)
    # (the ring is shared: one more launch of the side into set 0, read before any other side writes there)
    dones[f"rollout_random_{n}x{T}"] = {side: (lambda fn=fn: (fn(0), ring[0]["done"].clone())[1]) for side, fn in rollers.items()}
    # (b) single steps
    act = torch.full((n, 4), 2.45, device="cuda")
    bufs = {side: (torch.zeros((n, 10), device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")) for side in SIDES}
    shapes[f"step_{n}"] = (1, {side: (lambda i, e=env(side), b=bufs[side]: e.step(act, out=b)) for side in SIDES})
    dones[f"step_{n}"] = {side: (lambda side=side: bufs[side][2]) for side in SIDES}

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
        dones[f"policy_{actor}_{n}x{TP}"] = {side: (lambda c=c: c.done) for side, c in cols.items()}

    res = {"device": torch.cuda.get_device_name(0), "envs": n, "reps_per_side_and_pass": args.reps, "passes": args.passes,
           "sides": {side: repr(next(iter(kw.values()))) for side, kw in SIDES.items()}, "shapes": {}}
    for tag, (steps, sides) in shapes.items():
        med = {name: [] for name in sides}
        for _ in range(args.passes):
            for name, ts in alternate(sides, args.reps).items():
                med[name].append(round(statistics.median(ts), 2))
        row = {name: {"median_us_by_pass": v, "median_us": round(statistics.median(v), 2), "spread_us": round(max(v) - min(v), 2),
                      "env_steps_per_s_G": round(n * steps / (statistics.median(v) * 1e-6) / 1e9, 3)} for name, v in med.items()}
        for name, base in BASE_OF.items():
            row[name][f"ratio_over_{base}"] = round(row[name]["median_us"] / row[base]["median_us"], 4)
        for name in sides:   # the share of env-steps of the last launch that ended an episode
            row[name]["done_rate"] = round(float(dones[tag][name]().float().mean().item()), 5)
        res["shapes"][tag] = row
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()

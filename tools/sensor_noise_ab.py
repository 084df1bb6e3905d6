#!/usr/bin/env python3
"""Timings behind profiles/r19/sensor_noise.md: what a handle with sensor noise (rmav_set_sensor_noise) pays for its route - the *_sn
kernels are the disturbed bodies with the observation draw - against a handle of the SAME build that has the all-zero disturbance and no
sensor noise (the *_ds kernels: the bodies the *_sn kernels are cut from), at 65 536 quadrotor3d envs:

  (a) rollout   64-step random-action launches, trajectory (actions, obs, reward, done) stored into a cold ring of buffer sets (bench.py's
                method: >= 5 sets, > 1.5 GB): k_rollout_sn against k_rollout_ds
  (b) step      rmav_step (device pointers, batch-major actions and obs): k_step_sn against k_step_ds
  (c) policy    32-step in-kernel policy rollouts (FusedPolicyCollector, trajectory stored) of the three actors: k_rollout_nrm_sn /
                k_rollout_pair_sn / k_rollout_pair_shared_sn against their *_ds counterparts

Both sides live in one process and alternate launch by launch - a, b, a, b - so that clock and co-tenant drift hit both alike; every
launch sits between two HIP events (5 warm-up launches per side, then `--reps` timed ones per side), and the whole sequence runs
`--passes` times; the table has the median per side and pass, the spread over the passes and the ratio of the medians.

    python tools/sensor_noise_ab.py [--out FILE] [--passes 3] [--reps 30] [--sigma 0.01]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reinmav-gym_amd"))
WARM = 5
CALM = dict(wind=0.0, gust=0.0, hold=1 << 20)   # the all-zero disturbance at the hold the *_sn launches of a calm handle pass


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
    ap.add_argument("--sigma", type=float, default=0.01)
    args = ap.parse_args()
    import torch

    import gym_reinmav_amd as g

    assert torch.cuda.is_available(), "a measurement needs the GPU"
    n, T = args.envs, 64
    calm = g.Disturbance(**CALM)
    noise = g.SensorNoise(args.sigma)

    def env(noisy):
        return g.BatchedQuadrotor("quad3d", n, seed=1, disturbance=calm, sensor_noise=noise if noisy else None)

    shapes = {}
    # (a) fused rollouts into a cold ring
    per_set = T * n * (4 * (4 + 10 + 1) + 1)
    R = max(5, -(-int(1.5e9) // per_set))
    ring = [{"actions": torch.zeros((T, 4, n), device="cuda"), "obs": torch.zeros((T, 10, n), device="cuda"), "rew": torch.zeros((T, n), device="cuda"),
             "done": torch.zeros((T, n), dtype=torch.uint8, device="cuda")} for _ in range(R)]
    want = ("actions", "obs", "rew", "done")
    ea, eb = env(False), env(True)
    shapes[f"rollout_random_{n}x{T}"] = (T, {"disturbance": lambda i: ea.rollout(T, mode="random", device_out=True, want=want, out=ring[i % R]),
                                             "disturbance+sensor_noise": lambda i: eb.rollout(T, mode="random", device_out=True, want=want, out=ring[i % R])})
    # (b) single steps
    sa, sb = env(False), env(True)
    act = torch.full((n, 4), 2.45, device="cuda")
    bufs = [(torch.zeros((n, 10), device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")) for _ in range(2)]
    shapes[f"step_{n}"] = (1, {"disturbance": lambda i: sa.step(act, out=bufs[0]), "disturbance+sensor_noise": lambda i: sb.step(act, out=bufs[1])})

    # (c) policy rollouts
    from gym_reinmav_amd.ppo import FusedPolicyCollector, MlpPolicy

    TP = 32
    for actor in ("fp32_mfma", "f16", "f16_shared"):
        cols = []
        for noisy in (False, True):
            e = env(noisy)
            torch.manual_seed(3)
            pol = MlpPolicy(e.nS, e.nA, value_network="shared" if actor == "f16_shared" else "copy").cuda()
            cols.append(FusedPolicyCollector(e, pol, TP, f16_mfma=(actor == "f16")))
        shapes[f"policy_{actor}_{n}x{TP}"] = (TP, {"disturbance": lambda i, c=cols[0]: c.collect(),
                                                   "disturbance+sensor_noise": lambda i, c=cols[1]: c.collect()})

    res = {"device": torch.cuda.get_device_name(0), "envs": n, "reps_per_side_and_pass": args.reps, "passes": args.passes,
           "disturbance": repr(calm), "sensor_noise": repr(noise), "shapes": {}}
    for tag, (steps, sides) in shapes.items():
        med = {name: [] for name in sides}
        for _ in range(args.passes):
            for name, ts in alternate(sides, args.reps).items():
                med[name].append(round(statistics.median(ts), 2))
        base = next(iter(sides))
        row = {name: {"median_us_by_pass": v, "median_us": round(statistics.median(v), 2), "spread_us": round(max(v) - min(v), 2),
                      "env_steps_per_s_G": round(n * steps / (statistics.median(v) * 1e-6) / 1e9, 3)} for name, v in med.items()}
        for name in sides:
            if name != base:
                row[name][f"ratio_over_{base}"] = round(row[name]["median_us"] / row[base]["median_us"], 4)
        res["shapes"][tag] = row
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()

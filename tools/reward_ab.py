#!/usr/bin/env python3
"""Timings behind profiles/r17/reward.md: what a handle with a tracking reward (rmav_set_reward) pays for its route - the *_rw kernels are
the frame-skip bodies at k = 1 with the reward evaluated in the loop - against a plain handle of the SAME build, at 65 536 quadrotor3d
envs:

  (a) rollout   64-step random-action launches, trajectory (actions, obs, reward, done) stored into a cold ring of buffer sets (bench.py's
                method: >= 5 sets, > 1.5 GB): k_rollout_rw at k = 1, no range, against the plain one-wavefront k_rollout
                (RMAV_TUNE_SPLIT = 0 on the plain handle: a handle with a spec has no two-wavefront kernel, and that difference is
                reported apart, as `plain_split`: the plain handle under its default launch rules)
  (b) step      rmav_step (device pointers, batch-major actions and obs) of such a handle against a plain one
  (c) policy    the shared-trunk policy rollout (RMAV_POLICY_F16_SHARED) at 32 steps against the plain one

Both sides live in one process and alternate launch by launch - a, b, a, b - so that clock and co-tenant drift hit both alike; every
launch sits between two HIP events (5 warm-up launches per side, then `--reps` timed ones per side), and the whole sequence runs
`--passes` times; the table has the median per side and pass, the spread over the passes and the ratio of the medians.

    python tools/reward_ab.py [--out FILE] [--passes 3] [--reps 30]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reinmav-gym_amd"))
WARM = 5
SPEC = dict(goal=(0.0, 0.0, 2.0), alive=1.0, w_pos=1.0, w_vel=0.1, w_act=0.01, terminal=-10.0)


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
    from gym_reinmav_amd.ppo import FusedPolicyCollector, MlpPolicy

    assert torch.cuda.is_available(), "a measurement needs the GPU"
    n, T = args.envs, 64
    reward = g.TrackingReward(**SPEC)

    def env(spec, **tune):
        e = g.BatchedQuadrotor("quad3d", n, seed=1, reward=reward if spec else None)
        if tune:
            e.set_tuning(**tune)
        return e

    shapes = {}
    # (a) fused rollouts into a cold ring
    per_set = T * n * (4 * (4 + 10 + 1) + 1)
    R = max(5, -(-int(1.5e9) // per_set))
    ring = [{"actions": torch.zeros((T, 4, n), device="cuda"), "obs": torch.zeros((T, 10, n), device="cuda"), "rew": torch.zeros((T, n), device="cuda"),
             "done": torch.zeros((T, n), dtype=torch.uint8, device="cuda")} for _ in range(R)]
    want = ("actions", "obs", "rew", "done")
    ea, eb, ec = env(False, split=0), env(True), env(False)
    shapes[f"rollout_random_{n}x{T}"] = (T, {"plain_one_wavefront": lambda i: ea.rollout(T, mode="random", device_out=True, want=want, out=ring[i % R]),
                                             "reward": lambda i: eb.rollout(T, mode="random", device_out=True, want=want, out=ring[i % R]),
                                             "plain_split": lambda i: ec.rollout(T, mode="random", device_out=True, want=want, out=ring[i % R])})
    # (b) single steps
    sa, sb = env(False), env(True)
    act = torch.full((n, 4), 2.45, device="cuda")
    bufs = [(torch.zeros((n, 10), device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")) for _ in range(2)]
    shapes[f"step_{n}"] = (1, {"plain": lambda i: sa.step(act, out=bufs[0]), "reward": lambda i: sb.step(act, out=bufs[1])})
    # (c) the shared-trunk policy rollout
    calls = {}
    for name, spec in (("plain", False), ("reward", True)):
        e = env(spec)
        torch.manual_seed(0)
        pol = MlpPolicy(e.nS, e.nA, value_network="shared").cuda()
        with torch.no_grad():
            pol.pi[2].bias[0] = 9.8
        col = FusedPolicyCollector(e, pol, 32)
        col._pack()
        calls[name] = (e, col, col._call[0], col._call[1:])
    shapes[f"policy_shared_{n}x32"] = (32, {name: (lambda i, c=c: g._abi.check(c[2](c[0]._h, *c[3]))) for name, c in calls.items()})

    res = {"device": torch.cuda.get_device_name(0), "envs": n, "reps_per_side_and_pass": args.reps, "passes": args.passes, "spec": SPEC, "shapes": {}}
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

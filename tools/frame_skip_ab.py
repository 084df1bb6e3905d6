#!/usr/bin/env python3
"""Timings behind profiles/r16/frame_skip.md: what holding each action for k dynamics sub-steps inside the kernels (rmav_set_frame_skip)
buys per stored sample and per actor evaluation, and that a handle with k = 1 costs what it cost before.

The baseline (a) is a built checkout of the PARENT commit (`--baseline-root`: its package and its library, which has no frame-skip
kernels), the candidate (b) this tree.  Two libraries cannot share a process, so the driver alternates child processes - a, b, a, b:
interleaved passes, one GPU process at a time; each child times every shape with HIP events around single launches (5 warm-up
launches, median of 30) and prints one JSON line.  The parent child measures k = 1 only; this tree's child k = 1, 2, 4, 8.  The driver
prints, per shape, the k = 1 medians of both sides with their spread over the passes, and for every k the agent steps / s and the
dynamics sub-steps / s (= k x agent steps / s: an upper bound - a lane that terminates inside an agent step runs fewer); `--out FILE`
also writes the object.

    python tools/frame_skip_ab.py --baseline-root /path/to/built/parent/checkout [--out FILE] [--passes 2]

Shapes: q3d = quadrotor3d, 65 536 envs x 64-step random-action rollouts with the trajectory (actions, obs, reward, done) stored into a
cold ring of buffer sets (bench.py's method: >= 5 sets, > 1.5 GB); the policy rollouts at 65 536 x 32 - f16 pair, shared-trunk pair,
fp32 matrix-core actor - as tools/domain_rand_ab.py times them."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REP, WARM = 30, 5
SKIPS = (1, 2, 4, 8)


def child(side: str, root: str):
    sys.path.insert(0, os.path.join(root, "reinmav-gym_amd"))
    import torch

    import gym_reinmav_amd as g
    from gym_reinmav_amd.ppo import FusedPolicyCollector, MlpPolicy

    def timed(fn):
        for i in range(WARM):
            fn(i)
        ts = []
        for i in range(REP):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(WARM + i)
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        ts.sort()
        return {"median_us": round(statistics.median(ts), 2), "min_us": round(ts[0], 2), "p90_us": round(ts[int(0.9 * len(ts))], 2)}

    def make(n, k):
        env = g.BatchedQuadrotor("quad3d", n, seed=1)
        if k != 1:
            env.frame_skip = k   # (the parent's package has no such attribute: its child runs k = 1 only)
        return env

    out = {"side": side, "lib": g._abi.LIB_PATH, "device": torch.cuda.get_device_name(0)}
    n, T = 65536, 64
    per_set = T * n * (4 * (4 + 10 + 1) + 1)
    R = max(5, -(-int(1.5e9) // per_set))
    ring = [{"actions": torch.zeros((T, 4, n), device="cuda"), "obs": torch.zeros((T, 10, n), device="cuda"), "rew": torch.zeros((T, n), device="cuda"),
             "done": torch.zeros((T, n), dtype=torch.uint8, device="cuda")} for _ in range(R)]
    for k in SKIPS if side == "branch" else (1,):
        env = make(n, k)
        out[f"q3d_random_65536x64_k{k}"] = timed(lambda i: env.rollout(T, mode="random", device_out=True, want=("actions", "obs", "rew", "done"), out=ring[i % R]))
        env.close()
    del ring
    for actor, shared in (("f16", False), ("f16", True), ("f32m", False)):
        for k in SKIPS if side == "branch" else (1,):
            env = make(n, k)
            torch.manual_seed(0)
            pol = MlpPolicy(env.nS, env.nA, value_network="shared" if shared else "copy").cuda()
            with torch.no_grad():
                pol.pi[2].bias[0] = 9.8
            col = FusedPolicyCollector(env, pol, 32, f16_mfma=(actor == "f16"))
            col._pack()
            fn, args = col._call[0], col._call[1:]
            out[f"policy_{'shared' if shared else actor}_65536x32_k{k}"] = timed(lambda i: g._abi.check(fn(env._h, *args)))
            env.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-root", help="a checkout of the parent commit with its library built (make -C reinmav-gym_amd)")
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--out")
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--child", choices=["parent", "branch"])
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.root)
    base = os.path.abspath(args.baseline_root or "")
    if not os.path.exists(os.path.join(base, "reinmav-gym_amd", "gym_reinmav_amd", "librmav.so")):
        raise SystemExit("--baseline-root: a built checkout of the parent commit is required (the baseline is never the code under test)")
    runs = {"parent": [], "branch": []}
    for _ in range(args.passes):
        for side in ("parent", "branch"):
            env = dict(os.environ)
            env.pop("RMAV_LIB_PATH", None)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", side, "--root", base if side == "parent" else ROOT], env=env,
                               capture_output=True, text=True, timeout=300)
            if r.returncode != 0:   # nothing more is started after a failed GPU process
                raise SystemExit(f"{side} child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            runs[side].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    res = {"device": runs["branch"][0]["device"], "launches_per_median": REP, "passes": args.passes, "k1": {}, "throughput": {}}
    for tag in [t for t in runs["parent"][0] if t not in ("side", "lib", "device")]:
        a = [r[tag]["median_us"] for r in runs["parent"]]
        b = [r[tag]["median_us"] for r in runs["branch"]]
        res["k1"][tag] = {"parent_us": a, "branch_us": b, "parent_spread_us": round(max(a) - min(a), 2), "branch_spread_us": round(max(b) - min(b), 2),
                          "ratio_branch_over_parent": round(statistics.median(b) / statistics.median(a), 4)}
    for tag in [t for t in runs["branch"][0] if t not in ("side", "lib", "device")]:
        us = [r[tag]["median_us"] for r in runs["branch"]]
        k = int(tag.rsplit("_k", 1)[1])
        n, T = (int(x) for x in tag.split("_")[-2].split("x"))
        agent = n * T / (statistics.median(us) * 1e-6)
        res["throughput"][tag] = {"us": us, "agent_steps_per_s": round(agent / 1e9, 3), "sub_steps_per_s_upper": round(k * agent / 1e9, 3), "unit": "G/s"}
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Timings behind profiles/r25/ladder.md: the host launch cost of the single step before and after the feature ladder was written once
(csrc/rmav_ladder.hpp).  The device code of the two builds is identical (tools/isa_compare.py), so only the host path between rmav_step and
the kernel launch can move: eight flag tests and a direct call before, rung_of and one call through the table behind.

Three handles at 65 536 quadrotor3d envs:
  plain         no feature: k_step, off the ladder (rung_of returns RUNG_NONE after its eight tests)
  termination   the all-infinite termination spec alone: the top rung, k_step_tc
  all_eight     every switch of the ladder set (a range, a skip of 2, a tracking reward, a disturbance, sensor noise, actuator lag, a
                start-state spec, a termination spec): k_step_tc with every slot of its argument list filled from a spec

Every side is a fresh PROCESS that loads one library (RMAV_LIB_PATH), builds the three handles and times, per handle, `--reps` windows of
`--launches` single-step launches (rmav_rollout with fused = 0: the library's own loop over launch_step_k, device pointers, outputs
stored) between two HIP events, after a warm-up window; it prints the median window as us per launch.  The driver starts the sides in
turn - parent, parent again, branch - `--rounds` times, so that clock and co-tenant drift hit them alike.  The two parent sides give
the spread (the largest difference between two medians of the same library over all rounds); the branch passes where its median over
the rounds lies within that spread of the parent's.

At 65 536 envs the device needs longer per launch than the host, so those windows show what a training loop sees and hide a host path that
stays below the device's time.  The host path itself is timed on handles of 64 envs (`host64_*`: one wavefront, whose kernel is shorter
than its enqueue): the host's wall clock around the same call - `--launches` launches enqueued from the library's loop, nothing waited
for - with a device synchronise only behind the clock's second reading; us of host time per launch, the same sides, rounds and rule.

    python tools/ladder_ab.py --parent OLD/librmav.so [--branch NEW/librmav.so] [--out DIR] [--rounds 5]
    python tools/ladder_ab.py --side          (one side: prints one JSON line)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reinmav-gym_amd"))
KIND, NS, NA = "quad3d", 10, 4
HANDLES = ("plain", "termination", "all_eight")


def handle(g, name, n):
    kw = {}
    if name != "plain":
        kw["termination"] = g.Termination()
    if name == "all_eight":
        kw.update(randomize={"mass": (0.9, 1.1)}, frame_skip=2, reward=g.TrackingReward(goal=(0.0, 0.0, 1.0), w_pos=1.0), disturbance=g.Disturbance(wind=0.1, gust=0.1, hold=8),
                  sensor_noise=g.SensorNoise(0.01), actuator=g.Actuator(0.05), start_state=g.StartState(-0.5, 0.5))
    return g.BatchedQuadrotor(KIND, n, seed=0, **kw)


def side(args):
    import torch

    import gym_reinmav_amd as g

    dev = torch.device("cuda", 0)
    n, K = args.envs, args.launches
    stream = torch.cuda.Stream(device=dev)
    out = {"lib": g._abi.LIB_PATH}
    with torch.cuda.stream(stream):
        ring = torch.empty((K, NA, n), dtype=torch.float32, device=dev).uniform_(4.0, 6.0)
        bufs = {"obs": torch.empty((K, NS, n), device=dev), "rew": torch.empty((K, n), device=dev), "done": torch.empty((K, n), dtype=torch.uint8, device=dev)}
        for name in HANDLES:
            env = handle(g, name, n)

            def run():
                env.rollout(K, mode="buffer", actions=ring, layout="soa", fused=False, want=("obs", "rew", "done"), device_out=True, out=bufs)

            run()
            torch.cuda.synchronize()
            us = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                run()
                e1.record(stream)
                e1.synchronize()
                us.append(e0.elapsed_time(e1) / K * 1e3)
            out[name] = {"median": statistics.median(us), "min": min(us), "max": max(us)}
            env.close()
        # the host path alone: 64 envs, the wall clock around the enqueue of K launches (no wait inside the window)
        small = {k: v[:, ..., :64].contiguous() for k, v in bufs.items()}
        ring64 = ring[:, :, :64].contiguous()
        for name in HANDLES:
            env = handle(g, name, 64)

            def enqueue():
                env.rollout(K, mode="buffer", actions=ring64, layout="soa", fused=False, want=("obs", "rew", "done"), device_out=True, out=small)

            enqueue()
            torch.cuda.synchronize()
            us = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                enqueue()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                us.append((t1 - t0) / K * 1e6)
            out["host64_" + name] = {"median": statistics.median(us), "min": min(us), "max": max(us)}
            env.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", action="store_true")
    ap.add_argument("--parent")
    ap.add_argument("--branch", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "ladder_ab"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--launches", type=int, default=512)
    ap.add_argument("--envs", type=int, default=65536)
    args = ap.parse_args()
    if args.side:
        return side(args)
    if not args.parent or not os.path.exists(args.parent):
        sys.exit("--parent: the parent commit's librmav.so")
    os.makedirs(args.out, exist_ok=True)
    sides = (("parent", args.parent), ("parent_again", args.parent), ("branch", args.branch))
    rows = []
    for rnd in range(args.rounds):
        for who, lib in sides:
            env = dict(os.environ, RMAV_LIB_PATH=lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--side", "--reps", str(args.reps), "--launches", str(args.launches), "--envs", str(args.envs)],
                               env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:   # a side that failed ends the run: nothing more is started on the GPU
                sys.exit(f"round {rnd} {who}: exit {p.returncode}\n{p.stderr[-2000:]}")
            r = json.loads([ln for ln in p.stdout.split("\n") if ln.startswith("{")][-1])
            rows.append({"round": rnd, "side": who, **r, "lib": who.split("_")[0]})
            print(rnd, who, " ".join(f"{h} {v['median']:.3f}" for h, v in r.items() if h != "lib"), flush=True)
    res = {"envs": args.envs, "launches": args.launches, "reps": args.reps, "rounds": args.rounds, "rows": rows, "summary": {}}
    md = ["| handle | parent (us per launch, median of the rounds; each round) | parent again | branch | parent-parent spread | branch - parent | inside |", "|---|---|---|---|---|---|---|"]
    for h in HANDLES + tuple("host64_" + x for x in HANDLES):
        per = {who: [r[h]["median"] for r in rows if r["side"] == who] for who, _ in sides}
        same = per["parent"] + per["parent_again"]
        spread = max(same) - min(same)
        med = {who: statistics.median(v) for who, v in per.items()}
        delta = med["branch"] - statistics.median(same)
        res["summary"][h] = {"median": med, "spread": spread, "delta": delta, "inside": abs(delta) <= spread}
        cell = lambda who: f"{med[who]:.3f} ({', '.join(f'{x:.3f}' for x in per[who])})"
        md.append(f"| {h} | {cell('parent')} | {cell('parent_again')} | {cell('branch')} | {spread:.3f} | {delta:+.3f} | {'yes' if abs(delta) <= spread else 'NO'} |")
    open(os.path.join(args.out, "ladder_ab.json"), "w").write(json.dumps(res, indent=1) + "\n")
    open(os.path.join(args.out, "ladder_ab.md"), "w").write("\n".join(md) + "\n")
    print("\n".join(md))


if __name__ == "__main__":
    main()

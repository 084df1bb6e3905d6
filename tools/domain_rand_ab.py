#!/usr/bin/env python3
"""Timings behind profiles/r11/domain_randomisation.md: what per-episode domain randomisation (rmav_set_env_param_range) costs
against FIXED per-env constants (rmav_set_env_param), which is what a caller had before.

The baseline (a) is a built checkout of the PARENT commit (`--baseline-root`: its package and its library, which has no ranged
kernels), the candidate (b) this tree with ranges on the same parameters.  Two libraries cannot share a process, so the driver alternates child processes
- a, b, a, b, a, b: three interleaved passes - one GPU process at a time; each child times every shape with HIP events around
single launches (5 warm-up launches, median of 40) and prints one JSON line.  The driver prints, per shape, the medians of every
pass, their spread over the passes and the ratio b / a; `--out FILE` also writes the object.

    python tools/domain_rand_ab.py --baseline-root /path/to/built/parent/checkout [--out FILE] [--passes 3]

Shapes: c4 = quadrotor3d-slungload, 262 144 envs x 64-step random-action rollouts (bench.py's c4_per_env_params), q3d = quadrotor3d,
65 536 x 64; c5 = the per-GPU policy-rollout shape (quadrotor3d, 65 536 x 32; fp32-MFMA, f16 pair, shared-trunk pair);
step = rmav_step of quadrotor3d at 262 144 envs.  The ranges are +-10 % around the shared constants, as the fixed arrays are."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REP, WARM = 40, 5
NAMES = ("mass", "load_mass", "tether_length")


def child(ranged: bool, root: str):
    sys.path.insert(0, os.path.join(root, "reinmav-gym_amd"))
    import torch

    import gym_reinmav_amd as g
    from gym_reinmav_amd.ppo import FusedPolicyCollector, MlpPolicy

    def timed(fn):
        for _ in range(WARM):
            fn()
        ts = []
        for _ in range(REP):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        ts.sort()
        return {"median_us": round(statistics.median(ts), 2), "min_us": round(ts[0], 2), "p90_us": round(ts[int(0.9 * len(ts))], 2)}

    def make(kind, n):
        env = g.BatchedQuadrotor(kind, n, seed=1)
        base = {"mass": env.params.mass, "load_mass": env.params.load_mass, "tether_length": env.params.tether_length}
        gen = torch.Generator().manual_seed(3)
        for nm in NAMES if kind.endswith("_sl") else NAMES[:1]:
            if ranged:
                env.set_env_param_range(nm, 0.9 * base[nm], 1.1 * base[nm])
            else:
                env.set_env_param(nm, (base[nm] * (0.9 + 0.2 * torch.rand(n, generator=gen))).to(torch.float32).numpy())
        return env

    out = {"side": "ranged" if ranged else "fixed", "lib": g._abi.LIB_PATH, "device": torch.cuda.get_device_name(0)}
    for tag, kind, n, T in (("c4_quad3d_sl_262144x64", "quad3d_sl", 262144, 64), ("quad3d_65536x64", "quad3d", 65536, 64)):
        env = make(kind, n)
        bufs = env.rollout(T, mode="random", device_out=True, want=("obs", "rew", "done"))
        out[tag] = timed(lambda: env.rollout(T, mode="random", device_out=True, want=("obs", "rew", "done"), out=bufs))
        env.close()
    env = make("quad3d", 262144)
    acts = torch.rand((4, 262144), device="cuda") * 10.0
    o = (torch.empty((10, 262144), device="cuda"), torch.empty(262144, device="cuda"), torch.empty(262144, dtype=torch.uint8, device="cuda"))
    out["step_quad3d_262144"] = timed(lambda: env.step(acts, layout="soa", out=o))
    env.close()
    for actor, shared in (("f32m", False), ("f16", False), ("f16", True)):
        env = make("quad3d", 65536)
        torch.manual_seed(0)
        pol = MlpPolicy(env.nS, env.nA, value_network="shared" if shared else "copy").cuda()
        with torch.no_grad():
            pol.pi[2].bias[0] = 9.8
        col = FusedPolicyCollector(env, pol, 32, f16_mfma=(actor == "f16"))
        col._pack()
        fn, args = col._call[0], col._call[1:]
        out[f"c5_policy_{'shared' if shared else actor}_65536x32"] = timed(lambda: g._abi.check(fn(env._h, *args)))
        env.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-root", help="a checkout of the parent commit with its library built (make -C reinmav-gym_amd)")
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--out")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--child", choices=["fixed", "ranged"])
    args = ap.parse_args()
    if args.child:
        return child(args.child == "ranged", args.root)
    base = os.path.abspath(args.baseline_root or "")
    if not os.path.exists(os.path.join(base, "reinmav-gym_amd", "gym_reinmav_amd", "librmav.so")):
        raise SystemExit("--baseline-root: a built checkout of the parent commit is required (the baseline is never the code under test)")
    runs = {"fixed": [], "ranged": []}
    for _ in range(args.passes):
        for side in ("fixed", "ranged"):
            env = dict(os.environ)
            env.pop("RMAV_LIB_PATH", None)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", side, "--root", base if side == "fixed" else ROOT], env=env,
                               capture_output=True, text=True, timeout=300)
            if r.returncode != 0:   # nothing more is started after a failed GPU process
                raise SystemExit(f"{side} child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            runs[side].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    res = {"device": runs["ranged"][0]["device"], "launches_per_median": REP, "passes": args.passes, "shapes": {}}
    for tag in [k for k in runs["ranged"][0] if k not in ("side", "lib", "device")]:
        a = [r[tag]["median_us"] for r in runs["fixed"]]
        b = [r[tag]["median_us"] for r in runs["ranged"]]
        ma, mb = statistics.median(a), statistics.median(b)
        res["shapes"][tag] = {"fixed_parent_us": a, "ranged_us": b, "fixed_spread_us": round(max(a) - min(a), 2), "ranged_spread_us": round(max(b) - min(b), 2),
                              "ratio_ranged_over_fixed": round(mb / ma, 4)}
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()

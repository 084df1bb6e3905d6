#!/usr/bin/env python3
"""A/B of observation normalisation (profiles/r09/obs_norm.md), device-event timings, the two sides alternating in one process:

    python tools/obs_norm_ab.py rollout             # rmav_rollout_policy vs rmav_rollout_policy_norm, the three actors
    python tools/obs_norm_ab.py moments             # the statistics passes: us, achieved fraction of 8 TB/s, us added per VecEnv step
    python tools/obs_norm_ab.py parent OTHER.so     # rmav_rollout_policy of this build vs another build of the library (the parent
                                                    # commit's), alternating child processes (one library per process: RMAV_LIB_PATH)

Shape: BASELINE C5's per-GPU shape, 65 536 quadrotor3d envs x 32 steps.  The rollout launch is timed on its own (the weight pack is
the same launch on both sides and stays outside the window): BLOCK launches between two events, ROUNDS rounds of A-block, B-block."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "reinmav-gym_amd")]

N, T, KIND = 65536, 32, "quad3d"
ROUNDS, BLOCK, WARM = 15, 10, 5
ACTORS = (("f32m", False), ("f16", False), ("f16_shared", True))
HBM = 8.0e12


def _timed(fn, reps):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps   # us per call


def _collector(actor, shared, norm):
    import torch
    from gym_reinmav_amd import BatchedQuadrotor
    from gym_reinmav_amd import ppo as P
    from gym_reinmav_amd.obs_norm import RunningObsNorm

    env = BatchedQuadrotor(KIND, N, seed=1)
    torch.manual_seed(0)
    stats = None
    if norm:   # statistics of a random-action rollout: far from identity, the default clip
        stats = RunningObsNorm(env.nS, f"cuda:{env.device}")
        twin = BatchedQuadrotor(KIND, N, seed=2)
        stats.update(twin.rollout(T, mode="random", layout="soa", device_out=True, want=("obs",))["obs"], env=twin)
        twin.sync()
        twin.close()
    pol = P.MlpPolicy(env.nS, env.nA, value_network="shared" if shared else "copy", obs_norm=stats).cuda()
    col = P.FusedPolicyCollector(env, pol, T, f16_mfma=actor.startswith("f16"))
    col._pack()
    return env, col, (lambda: col._A.check(col._call[0](env._h, *col._call[1:])))


def _summary(v):
    return f"{statistics.median(v):.1f} | {min(v):.1f} | {max(v):.1f}"


def rollout():
    print(f"rmav_rollout_policy (A) vs rmav_rollout_policy_norm (B), {KIND} {N} envs x {T} steps, us per launch over {ROUNDS} alternating rounds of {BLOCK}\n")
    print("| actor | A median | A min | A max | B median | B min | B max | B / A (medians) |")
    print("|---|---|---|---|---|---|---|---|")
    for actor, shared in ACTORS:
        ea, _, fa = _collector(actor, shared, False)
        eb, _, fb = _collector(actor, shared, True)
        for f in (fa, fb):
            _timed(f, WARM)
        ta, tb = [], []
        for _ in range(ROUNDS):
            ta.append(_timed(fa, BLOCK))
            tb.append(_timed(fb, BLOCK))
        print(f"| {actor} | {_summary(ta)} | {_summary(tb)} | {statistics.median(tb) / statistics.median(ta):.3f} |", flush=True)
        ea.close()
        eb.close()


def moments():
    import torch
    from gym_reinmav_amd import BatchedQuadrotor
    from gym_reinmav_amd.obs_norm import RunningObsNorm

    env = BatchedQuadrotor(KIND, N, seed=1)
    norm = RunningObsNorm(env.nS, f"cuda:{env.device}")
    soa = env.rollout(T, mode="random", layout="soa", device_out=True, want=("obs",))["obs"]
    aos = soa[0].t().contiguous()
    out = torch.empty_like(aos)
    print(f"statistics passes, {KIND} {N} envs, us per call (median | min | max over {ROUNDS} blocks of {BLOCK})\n")
    print("| call | us | bytes read | fraction of 8 TB/s (median) |")
    print("|---|---|---|---|")
    for name, fn, nbytes in (
            (f"update (moments + fold + merge), SoA {T} x {N}", lambda: norm.update(soa, env=env), soa.numel() * 4),
            (f"update (moments + fold + merge), AoS 1 x {N}", lambda: norm.update(aos, layout="aos", env=env), aos.numel() * 4),
            (f"normalize, AoS 1 x {N}", lambda: norm.normalize(aos, out=out, layout="aos", env=env), aos.numel() * 4),
            ("update + normalize, AoS (what VecNormalize adds to a step)",
             lambda: (norm.update(aos, layout="aos", env=env), norm.normalize(aos, out=out, layout="aos", env=env)), aos.numel() * 8)):
        _timed(fn, WARM)
        v = [_timed(fn, BLOCK) for _ in range(ROUNDS)]
        print(f"| {name} | {_summary(v)} | {nbytes} | {nbytes / (statistics.median(v) * 1e-6) / HBM:.3f} |", flush=True)
    env.close()


def child():
    """rmav_rollout_policy alone, the three actors: one JSON line {actor: [us per launch of each block]}"""
    import ctypes

    from gym_reinmav_amd import _abi as A

    have = ctypes.CDLL(A.LIB_PATH)   # an older build lacks the newest entry points: bind what it has
    for name in [n for n in A.PROTOTYPES if not hasattr(have, n)]:
        del A.PROTOTYPES[name]
    res = {}
    for actor, shared in ACTORS:
        e, _, f = _collector(actor, shared, False)
        _timed(f, WARM)
        res[actor] = [_timed(f, BLOCK) for _ in range(ROUNDS)]
        e.close()
    print("RESULT " + json.dumps(res), flush=True)


def parent(other):
    """this build (A) vs `other` (B), three alternating child processes each"""
    runs = {"A": [], "B": []}
    for rep in range(3):
        for side, lib in (("A", None), ("B", os.path.abspath(other))):
            env = dict(os.environ)
            if lib:
                env["RMAV_LIB_PATH"] = lib
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=600)
            if run.returncode != 0:
                raise SystemExit(f"child {side} failed ({run.returncode}):\n{run.stderr[-2000:]}")
            out = run.stdout
            runs[side].append(json.loads(next(line for line in out.splitlines() if line.startswith("RESULT "))[7:]))
    print(f"rmav_rollout_policy, this build (A) vs {os.path.basename(other)} (B), {KIND} {N} x {T}, us per launch: median of each process's "
          f"{ROUNDS} blocks of {BLOCK}, processes alternating A B A B A B\n")
    print("| actor | A per process | B per process | A / B (medians of medians) |")
    print("|---|---|---|---|")
    for actor, _ in ACTORS:
        a = [statistics.median(r[actor]) for r in runs["A"]]
        b = [statistics.median(r[actor]) for r in runs["B"]]
        print(f"| {actor} | {' '.join(f'{x:.1f}' for x in a)} | {' '.join(f'{x:.1f}' for x in b)} | {statistics.median(a) / statistics.median(b):.3f} |")


if __name__ == "__main__":
    case = sys.argv[1] if len(sys.argv) > 1 else "rollout"
    if case == "rollout":
        rollout()
    elif case == "moments":
        moments()
    elif case == "child":
        child()
    elif case == "parent":
        parent(sys.argv[2])
    else:
        raise SystemExit(f"unknown case {case}")

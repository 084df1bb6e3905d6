#!/usr/bin/env python3
"""The policy action rule (profiles/r12/action_rule.md), device-event timings at BASELINE C5's per-GPU shape (quadrotor3d, 65 536 envs x
32 steps):

    python tools/action_rule_ab.py nrm OTHER.so   # rule OFF: rmav_rollout_policy_norm of this build (A) vs another build of the library
                                                  # (the parent commit's, B) - the kernels that gained the rule's arithmetic; alternating
                                                  # child processes (one library per process: RMAV_LIB_PATH), REPS of each
    python tools/action_rule_ab.py eval           # env-steps/s of evaluate_policy (deterministic, clipped, no act / obs stores) beside
                                                  # the training rollout of the same actor

Accept `nrm` if A's median is no slower than B's median plus B's own max - min spread in the session."""
import json
import os
import statistics
import subprocess
import sys
import time

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
from obs_norm_ab import ACTORS, BLOCK, KIND, ROUNDS, WARM, N, T, _collector, _timed  # noqa: E402

REPS = 5


def child():
    """rmav_rollout_policy_norm alone, the three actors: one JSON line {actor: [us per launch of each block]}"""
    import ctypes

    from gym_reinmav_amd import _abi as A

    have = ctypes.CDLL(A.LIB_PATH)   # an older build lacks the newest entry points: bind what it has
    for name in [n for n in A.PROTOTYPES if not hasattr(have, n)]:
        del A.PROTOTYPES[name]
    res = {}
    for actor, shared in ACTORS:
        e, _, f = _collector(actor, shared, True)
        _timed(f, WARM)
        res[actor] = [_timed(f, BLOCK) for _ in range(ROUNDS)]
        e.close()
    print("RESULT " + json.dumps(res), flush=True)


def nrm(other):
    runs = {"A": [], "B": []}
    for rep in range(REPS):
        for side, lib in (("B", os.path.abspath(other)), ("A", None)):
            env = dict(os.environ)
            if lib:
                env["RMAV_LIB_PATH"] = lib
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True, timeout=600)
            if run.returncode != 0:
                raise SystemExit(f"child {side} failed ({run.returncode}):\n{run.stderr[-2000:]}")
            runs[side].append(json.loads(next(line for line in run.stdout.splitlines() if line.startswith("RESULT "))[7:]))
    print(f"rmav_rollout_policy_norm, no action rule: this build (A) vs {os.path.basename(other)} (B), {KIND} {N} x {T}, us per launch: median "
          f"of each process's {ROUNDS} blocks of {BLOCK}, {REPS} processes each, alternating B A B A ...\n")
    print("| actor | A per process | B per process | A median | B median | B max - min | A <= B + spread |")
    print("|---|---|---|---|---|---|---|")
    for actor, _ in ACTORS:
        a = [statistics.median(r[actor]) for r in runs["A"]]
        b = [statistics.median(r[actor]) for r in runs["B"]]
        ma, mb, sp = statistics.median(a), statistics.median(b), max(b) - min(b)
        print(f"| {actor} | {' '.join(f'{x:.1f}' for x in a)} | {' '.join(f'{x:.1f}' for x in b)} | {ma:.1f} | {mb:.1f} | {sp:.1f} | "
              f"{'yes' if ma <= mb + sp else 'NO'} |")


def evaluate():
    import torch
    from gym_reinmav_amd import BatchedQuadrotor
    from gym_reinmav_amd import ppo as P
    from gym_reinmav_amd.evaluate import evaluate_policy

    print(f"{KIND} {N} envs, max_episode_steps = {T}: G env-steps/s, median | min | max of {REPS} repetitions\n")
    print("| actor | training rollout (weight pack + launch) | deterministic + clipped, no act / obs stores (weight pack + launch) | evaluate_policy (reset, launches, reduction, host wall clock) |")
    print("|---|---|---|---|")
    fmt = lambda v: f"{statistics.median(v):.2f} | {min(v):.2f} | {max(v):.2f}"  # noqa: E731
    for actor, shared in ACTORS:
        env = BatchedQuadrotor(KIND, N, seed=1, max_episode_steps=T)
        torch.manual_seed(0)
        pol = P.MlpPolicy(env.nS, env.nA, value_network="shared" if shared else "copy").cuda()
        kw = dict(f16_mfma=actor.startswith("f16"))
        train = P.FusedPolicyCollector(env, pol, T, **kw)
        ev = P.FusedPolicyCollector(env, pol, T, deterministic=True, clip_actions=True, store_trajectory=False, **kw)
        rates = {"train": [], "eval": [], "call": []}
        for col, key in ((train, "train"), (ev, "eval")):
            _timed(col.collect, WARM)
            rates[key] = [N * T / (_timed(col.collect, BLOCK) * 1e-6) / 1e9 for _ in range(REPS)]
        evaluate_policy(pol, env, **kw)
        for _ in range(REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            evaluate_policy(pol, env, **kw)   # (its float() results synchronise)
            rates["call"].append(N * T / (time.perf_counter() - t0) / 1e9)
        print(f"| {actor} | {fmt(rates['train'])} | {fmt(rates['eval'])} | {fmt(rates['call'])} |", flush=True)
        env.close()


if __name__ == "__main__":
    case = sys.argv[1] if len(sys.argv) > 1 else "eval"
    if case == "nrm":
        nrm(sys.argv[2])
    elif case == "child":
        child()
    elif case == "eval":
        evaluate()
    else:
        raise SystemExit(f"unknown case {case}")

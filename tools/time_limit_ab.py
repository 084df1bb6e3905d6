#!/usr/bin/env python3
"""Launch driver of the episode-time-limit A/B (profiles/r07/time_limit.md): the same launches with and without a limit on one
box, for `rocprofv3 --kernel-trace --stats` (one run per case, so that every kernel name in a run's stats belongs to one shape).

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/<case> -- python tools/time_limit_ab.py <case>

cases: step65536 | step262144 | step1048576 (k_step vs k_step_tl, quadrotor3d, caller actions), c2 (quadrotor3d 65 536 x 64 random
actions: default two-wavefront kernel, RMAV_TUNE_SPLIT = 0, limited), c3 (131 072 envs x 64, chunk-major: unlimited, limited), c5
(65 536 x 32 policy rollouts: fp32-MFMA, f16 pair, f16 shared trunk; unlimited, limited).  The limit is H = 1000: it fires
rarely, so the kernels do the same work and the difference is the time-limit bookkeeping itself."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "reinmav-gym_amd")]

import torch  # noqa: E402

from gym_reinmav_amd import BatchedQuadrotor  # noqa: E402
from gym_reinmav_amd import ppo as P  # noqa: E402

H, REPS, WARM = 1000, 40, 5


def env(n, limited, **tune):
    e = BatchedQuadrotor("quad3d", n, seed=1, max_episode_steps=H if limited else None)
    if tune:
        e.set_tuning(**tune)
    return e


def step(n):
    acts = torch.rand((4, n), device="cuda") * 10.0
    for limited in (False, True):
        e = env(n, limited)
        out = (torch.empty((10, n), device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda"))
        for _ in range(WARM + 5 * REPS):
            e.step(acts, layout="soa", out=out)
        torch.cuda.synchronize()
        e.close()


def rollouts(n, T, chunked):
    for limited, tune in ((False, {}), (False, {"split": 0}), (True, {})):
        if chunked and tune:
            continue   # (chunk-major calls always take the two-wavefront kernel without a limit)
        e = env(n, limited, **tune)
        out = None
        for _ in range(WARM + REPS):
            if chunked:
                out = e.rollout_chunked(T, mode="random", want=("obs", "rew", "done"), out=out)
            else:
                out = e.rollout(T, mode="random", device_out=True, want=("obs", "rew", "done"), out=out)
        torch.cuda.synchronize()
        e.close()


def policy(n, T):
    for actor, shared in (("f32m", False), ("f16", False), ("f16", True)):
        for limited in (False, True):
            e = env(n, limited)
            pol = P.MlpPolicy(e.nS, e.nA, value_network="shared" if shared else "copy").cuda()
            col = P.FusedPolicyCollector(e, pol, T, f16_mfma=(actor == "f16"))
            for _ in range(WARM + REPS):
                col.collect()
            torch.cuda.synchronize()
            e.close()


if __name__ == "__main__":
    case = sys.argv[1]
    if case.startswith("step"):
        step(int(case[4:]))
    elif case == "c2":
        rollouts(65536, 64, False)
    elif case == "c3":
        rollouts(131072, 64, True)
    elif case == "c5":
        policy(65536, 32)
    else:
        raise SystemExit(f"unknown case {case}")
    print("done", case)

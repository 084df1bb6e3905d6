#!/usr/bin/env python3
"""Launch driver and parser of the truncation-bootstrap A/B (profiles/r08/truncation_bootstrap.md), in the style of
tools/time_limit_ab.py: the same launches through the time-limited kernel and through its *_boot / *_final sibling in one process,
for `rocprofv3 --kernel-trace --stats` (kernel trace only; one run per case).

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/<case> -- python tools/boot_ab.py <case>
    python tools/boot_ab.py parse OUT          # median kernel times per case and kernel family, markdown

cases: policy1000 | policy16 (65 536 x 32 policy rollouts, quadrotor3d, H = 1000 / 16: rmav_rollout_policy vs rmav_rollout_policy_boot for the
fp32-MFMA, f16 pair and f16 shared-trunk actors), step65536 | step262144 (rmav_step vs rmav_step_final, H = 1000), gae32 | gae128
(rmav_gae vs rmav_gae_boot at 65 536 x 32 / x 128).  The baselines are the kernels the parent commit ships: tools/isa_compare.py shows
them instruction-identical in this build."""
import csv
import glob
import os
import re
import statistics
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "reinmav-gym_amd")]

REPS, WARM = 40, 5


def policy(n, T, H):
    import torch
    from gym_reinmav_amd import BatchedQuadrotor
    from gym_reinmav_amd import ppo as P

    for actor, shared in (("f32m", False), ("f16", False), ("f16", True)):
        for boot in (False, True):
            e = BatchedQuadrotor("quad3d", n, seed=1, max_episode_steps=H)
            torch.manual_seed(0)
            pol = P.MlpPolicy(e.nS, e.nA, value_network="shared" if shared else "copy").cuda()
            col = P.FusedPolicyCollector(e, pol, T, f16_mfma=(actor == "f16"), bootstrap_truncated=boot)
            for _ in range(WARM + REPS):
                col.collect()
            torch.cuda.synchronize()
            e.close()


def step(n, H=1000):
    import torch
    from gym_reinmav_amd import BatchedQuadrotor

    acts = torch.rand((4, n), device="cuda") * 10.0
    for final in (False, True):
        e = BatchedQuadrotor("quad3d", n, seed=1, max_episode_steps=H)
        out = (torch.empty((10, n), device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda"))
        extra = (torch.zeros((10, n), device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda"))
        for _ in range(WARM + 5 * REPS):
            if final:
                e.step_final(acts, layout="soa", out=out + extra)
            else:
                e.step(acts, layout="soa", out=out)
        torch.cuda.synchronize()
        e.close()


def gae(n, T):
    import torch
    from gym_reinmav_amd import BatchedQuadrotor

    e = BatchedQuadrotor("quad3d", n, seed=1, track_episodes=False)
    g = torch.Generator(device="cuda").manual_seed(0)
    rew, val = torch.randn((T, n), generator=g, device="cuda"), torch.randn((T + 1, n), generator=g, device="cuda")
    done = (torch.rand((T, n), generator=g, device="cuda") < 0.07).to(torch.uint8)
    boot = torch.where(done != 0, torch.randn((T, n), generator=g, device="cuda"), torch.zeros((), device="cuda"))
    out = (torch.empty_like(rew), torch.empty_like(rew))
    for b in (None, boot):
        for _ in range(WARM + REPS):
            e.gae(rew, done, val, out=out, boot=b)
        torch.cuda.synchronize()
    e.close()


FAMILIES = ("k_rollout_boot", "k_rollout_tl", "k_rollout_pair_boot", "k_rollout_pair_tl", "k_rollout_pair_shared_boot",
            "k_rollout_pair_shared_tl", "k_step_final", "k_step_tl", "k_gae_boot", "k_gae")


def parse(root):
    print("| case | kernel | calls | median us | min us | max us |")
    print("|---|---|---|---|---|---|")
    for case in sorted(os.listdir(root)):
        hits = glob.glob(os.path.join(root, case, "**", "*kernel_trace.csv"), recursive=True)
        if not hits:
            continue
        dur = defaultdict(list)
        for r in csv.DictReader(open(hits[0])):
            m = re.search(r"rmav::(\w+)", r["Kernel_Name"])
            if m and m.group(1) in FAMILIES:
                dur[m.group(1)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        for k in FAMILIES:
            if k in dur:
                v = dur[k][WARM:] if len(dur[k]) > 2 * WARM else dur[k]
                print(f"| {case} | {k} | {len(v)} | {statistics.median(v):.2f} | {min(v):.2f} | {max(v):.2f} |")


if __name__ == "__main__":
    case = sys.argv[1]
    if case == "parse":
        parse(sys.argv[2])
        sys.exit(0)
    if case.startswith("policy"):
        policy(65536, 32, int(case[6:]))
    elif case.startswith("step"):
        step(int(case[4:]))
    elif case.startswith("gae"):
        gae(65536, int(case[3:]))
    else:
        raise SystemExit(f"unknown case {case}")
    print("done", case)

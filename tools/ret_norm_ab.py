#!/usr/bin/env python3
"""Timings behind profiles/r10/ret_norm.md: the return-normalisation launches against the launches they stand beside, on one GPU, in
one process - HIP events around every launch (pair / triple of launches where a path is several), 5 warm-up calls, medians of 40, three
interleaved passes (the spread between the passes of one entry is the run-to-run spread).  Prints one JSON object; `--out FILE` also
writes it.

    python tools/ret_norm_ab.py [--out FILE]
"""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "reinmav-gym_amd"))
import torch

import gym_reinmav_amd as g
from gym_reinmav_amd.obs_norm import RunningObsNorm
from gym_reinmav_amd.ppo import PPO, FusedPolicyCollector, MlpPolicy
from gym_reinmav_amd.ret_norm import RunningReturnNorm

N, T, REP = 65536, 32, 40
A, L = g._abi, g._abi.lib()
p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
out = {"device": torch.cuda.get_device_name(0), "N": N, "T": T, "launches": REP}


def timed(fn, rep=REP, warm=5):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(rep):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return {"median_us": round(statistics.median(ts), 2), "min_us": round(ts[0], 2), "p90_us": round(ts[int(0.9 * len(ts))], 2)}


env = g.BatchedQuadrotor("quad3d", N, seed=0)
dev = torch.device("cuda", env.device)
rew = 3 * torch.randn(T, N, device=dev) + 1
done = (torch.rand(T, N, device=dev) < 0.05).to(torch.uint8)
val, boot = torch.randn(T + 1, N, device=dev), torch.zeros(T, N, device=dev)
adv, ret = torch.empty_like(rew), torch.empty_like(rew)
sums = torch.zeros(2, dtype=torch.float64, device=dev)
norm = RunningReturnNorm(dev)
norm.update(rew, done, env=env)
carry, rec = norm.carry(env), torch.zeros(3, dtype=torch.float64, device=dev)

for rnd in range(3):   # three interleaved passes: the spread between passes is the run-to-run spread
    out[f"gae_{rnd}"] = timed(lambda: L.rmav_gae(env._h, T, p(rew), p(done), p(val), 0.99, 0.95, 1.0, p(adv), p(ret), p(sums)))
    out[f"gae_norm_{rnd}"] = timed(lambda: L.rmav_gae_norm(env._h, T, p(rew), p(done), p(val), None, p(norm.buf), 0.99, 0.95, 1.0, p(adv), p(ret), p(sums)))
    out[f"gae_boot_{rnd}"] = timed(lambda: L.rmav_gae_boot(env._h, T, p(rew), p(done), p(val), p(boot), 0.99, 0.95, 1.0, p(adv), p(ret), p(sums)))
    out[f"gae_norm_boot_{rnd}"] = timed(lambda: L.rmav_gae_norm(env._h, T, p(rew), p(done), p(val), p(boot), p(norm.buf), 0.99, 0.95, 1.0, p(adv), p(ret), p(sums)))
    out[f"ret_moments_merge_{rnd}"] = timed(lambda: (L.rmav_ret_moments(env._h, T, p(rew), p(done), 1.0, 0.99, p(carry), p(rec)),
                                                      L.rmav_ret_norm_merge(env._h, p(norm.buf), p(rec), 1)))
    out[f"ret_moments_only_{rnd}"] = timed(lambda: L.rmav_ret_moments(env._h, T, p(rew), p(done), 1.0, 0.99, p(carry), p(rec)))

# the per-step paths of VecNormalize: three launches each on one [N] / [N, nS] step
r1, d1, z1 = rew[0].contiguous(), done[0].contiguous(), torch.empty(N, device=dev)
out["step_reward_path_3_launches"] = timed(lambda: (norm.update(r1, d1, env=env), norm.normalize(r1, env=env, out=z1)))
on = RunningObsNorm(env.nS, dev)
o1 = torch.randn(N, env.nS, device=dev)
oz = torch.empty_like(o1)
out["step_obs_path_3_launches"] = timed(lambda: (on.update(o1, layout="aos", env=env), on.normalize(o1, out=oz, layout="aos", env=env)))
env.close()

# share of a full collect + update iteration (C5's per-GPU shape)
env = g.BatchedQuadrotor("quad3d", N, seed=0, max_episode_steps=200)
torch.manual_seed(0)
pol = MlpPolicy(env.nS, env.nA).cuda()
col = FusedPolicyCollector(env, pol, T, f16_mfma=True, bootstrap_truncated=True)
for label, rn in (("iteration_plain", None), ("iteration_ret_norm", RunningReturnNorm(dev))):
    ppo = PPO(pol, ret_norm=rn)
    out[label] = timed(lambda: (col.collect(), ppo.update(col), col.roll_over()), rep=5, warm=2)
env.close()
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out, indent=1))

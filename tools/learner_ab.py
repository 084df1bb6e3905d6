#!/usr/bin/env python3
"""A/B of the PPO learner: torch autograd (PPO.update as it always was) against the fused learner (PPO(fused_learner=True) ->
rmav_ppo_grad), in ONE process, alternating, on the same rollouts.

    python tools/learner_ab.py [--envs 65536] [--steps 32] [--rounds 6] [--value-network copy|shared] [--fused-optimizer | --matrix-learner]
                                  [--out profiles/r23/learner_ab.json]

Shape: quadrotor3d, the per-GPU shape of the PPO benchmark (65 536 envs x 32 steps, 4 epochs x 4 minibatches of 524 288 samples).
Reports, as one JSON object (also written to --out):
  update_ms        ms per PPO.update on each path (median and min over the rounds; HIP events around the call, which ends in a host
                   read of its statistics)
  grad_us          us per rmav_ppo_grad call (two net launches + the fold) on one minibatch, by HIP events, median of 20
  flop             the FLOP count of one minibatch: 6 (2 nS 64 + 2 64 64 + 64 nA + 64) per sample (forward, backward and weight
                   gradients of both nets count 2 FLOP per multiply-add), and the fraction of the fp32 matrix roofline (155 TFLOP/s) and
                   of the plain vector-FMA rate (half of it) the call reaches
  end_to_end       env-steps/s of collect + update per actor (fp32 matrix-core, f16 pair) and path
Timings of one process on one GPU; the two paths see the same rollout data in every round.

--value-network shared: the same for an MlpPolicy(value_network="shared") and rmav_ppo_grad_shared (one net launch + the fold).  flop
is then 6 (nS 64 + 64 64 + 64 (nA + 1)) per sample, grad_us also holds one rmav_ppo_grad call on a copy policy of the same shapes taken
in the same session (rmav_ppo_grad_copy_same_session), and end_to_end has the one actor of that architecture, f16_shared.  The default,
copy, prints what it always printed.

--fused-optimizer: the A/B is PPO(fused_learner=True) against PPO(fused_learner=True, fused_optimizer=True) instead (both take their
gradients from the fused learner; "off" is the path without the flag), same alternation, same rollouts:
  update_ms        as above, per path ("off", "on")
  call_us          us per rmav_adv_moments call next to torch.std_mean(adv[idx]) + the stack it replaces, and per rmav_ppo_adam call next
                   to clip_grad_norm_ + Adam.step() on the same gradient (HIP events, median of 20)
  end_to_end       env-steps/s of collect + update on each path (fp32 matrix-core actor, or f16_shared)

--matrix-learner (with --value-network shared): the A/B is the vector-ALU shared-trunk kernel (rmav_ppo_grad_shared) against the
matrix-core one (rmav_ppo_grad_shared_mfma, PPO(matrix_learner=True)), both with the fused optimiser on, same alternation, same rollouts:
  update_ms        as above, per path ("vector", "matrix"), with the spread max - min of each
  grad_us          us per call of each kernel (net + fold) on one minibatch: in every round 20 calls of each, the order alternating;
                   median and min over the rounds' medians, and the round-to-round spread (max - min of the rounds' medians)
  end_to_end       env-steps/s of collect + update on each path (f16_shared actor)"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "reinmav-gym_amd"))

MATRIX_FP32_TFLOPS = 155.0


def timed(fn, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def finish(res, out):
    print(json.dumps(res))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def main_optimizer(args):
    import torch

    import gym_reinmav_amd as g
    from gym_reinmav_amd.ppo import PPO, FusedPolicyCollector, MlpPolicy

    torch.manual_seed(0)
    N, T = args.envs, args.steps
    res = {"shape": {"kind": "quad3d", "envs": N, "steps": T, "epochs": 4, "minibatches": 4, "minibatch": N * T // 4,
                     "value_network": args.value_network}, "device": torch.cuda.get_device_name(0)}
    env = g.BatchedQuadrotor("quad3d", N, seed=0)
    pols = {"off": MlpPolicy(env.nS, env.nA, value_network=args.value_network).cuda()}
    pols["on"] = copy.deepcopy(pols["off"])
    ppos = {k: PPO(p, fused_learner=True, fused_optimizer=(k == "on")) for k, p in pols.items()}
    ro = FusedPolicyCollector(env, pols["off"], T)
    ms = {"off": [], "on": []}
    for r in range(args.rounds + 1):   # round 0 warms both paths up
        ro.collect()
        for k in ("off", "on") if r % 2 == 0 else ("on", "off"):
            t, st = timed(lambda: ppos[k].update(ro), torch)
            if r:
                ms[k].append(t)
        ro.roll_over()
    res["update_ms"] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v} for k, v in ms.items()}
    res["update_gain_ms_median"] = res["update_ms"]["off"]["median"] - res["update_ms"]["on"]["median"]

    def med_us(fn):
        ts = []
        for _ in range(23):
            t, _ = timed(fn, torch)
            ts.append(t * 1e3)
        return statistics.median(ts[3:])

    B = N * T
    adv = ppos["on"].adv.reshape(-1)
    idx = torch.randperm(B, device="cuda")[:B // 4]

    def torch_moments():
        std, mean = torch.std_mean(adv[idx])
        return torch.stack((mean, 1.0 / (std + 1e-8)))

    ppo = ppos["off"]   # its p.grad views hold the last minibatch's gradient; both calls below step on that gradient again and again
    ps, flat = ppo._fused[0], ppo._fused[1]
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    shared = args.value_network == "shared"

    def torch_step():
        torch.nn.utils.clip_grad_norm_(ppo.policy.parameters(), ppo.max_grad_norm)
        ppo.opt.step()

    keep = flat.clone()

    def torch_step_fresh():   # clip_grad_norm_ rewrites p.grad: restore it (one 40 KB copy, inside the timed span of both arms)
        flat.copy_(keep)
        torch_step()

    def fused_step_fresh():
        flat.copy_(keep)
        env.ppo_adam(ps, flat, m, v, 7, max_grad_norm=ppo.max_grad_norm, shared=shared)

    res["call_us"] = {"rmav_adv_moments": med_us(lambda: env.adv_moments(adv, idx)), "torch_std_mean_gather_stack": med_us(torch_moments),
                      "rmav_ppo_adam_with_grad_copy": med_us(fused_step_fresh), "torch_clip_and_adam_with_grad_copy": med_us(torch_step_fresh),
                      "grad_copy_alone": med_us(lambda: flat.copy_(keep)), "samples": B // 4, "params": flat.numel()}
    res["end_to_end"] = {}
    actor = "f16_shared" if shared else "fp32_mfma"
    for k in ("off", "on"):
        col = FusedPolicyCollector(env, pols[k], T)
        rates = []
        for r in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            col.collect()
            ppos[k].update(col)
            col.roll_over()
            torch.cuda.synchronize()
            if r:
                rates.append(N * T / (time.perf_counter() - t0))
        res["end_to_end"][f"{actor}/{k}"] = {"env_steps_per_s_median": statistics.median(rates), "all": rates}
    env.close()
    finish(res, args.out)


def main_matrix(args):
    import torch

    import gym_reinmav_amd as g
    from gym_reinmav_amd.ppo import PPO, FusedPolicyCollector, MlpPolicy

    if args.value_network != "shared":
        raise SystemExit("--matrix-learner needs --value-network shared (the matrix-core learner computes the shared-trunk policy)")
    torch.manual_seed(0)
    N, T = args.envs, args.steps
    res = {"shape": {"kind": "quad3d", "envs": N, "steps": T, "epochs": 4, "minibatches": 4, "minibatch": N * T // 4,
                     "value_network": "shared", "fused_optimizer": True}, "device": torch.cuda.get_device_name(0)}
    env = g.BatchedQuadrotor("quad3d", N, seed=0)
    pols = {"vector": MlpPolicy(env.nS, env.nA, value_network="shared").cuda()}
    pols["matrix"] = copy.deepcopy(pols["vector"])
    ppos = {k: PPO(p, fused_learner=True, fused_optimizer=True, matrix_learner=(k == "matrix")) for k, p in pols.items()}
    ro = FusedPolicyCollector(env, pols["vector"], T)
    B = N * T
    idx = torch.randperm(B, device="cuda")[:B // 4]
    ms, us = {"vector": [], "matrix": []}, {"vector": [], "matrix": []}
    fns = {"vector": env.ppo_grad_shared, "matrix": env.ppo_grad_shared_mfma}
    for r in range(args.rounds + 1):   # round 0 warms both paths up
        ro.collect()
        order = ("vector", "matrix") if r % 2 == 0 else ("matrix", "vector")
        for k in order:
            t, st = timed(lambda: ppos[k].update(ro), torch)
            if r:
                ms[k].append(t)
        # one call of each kernel on one minibatch of this rollout, in the same order
        obs = ro.obs[:T].permute(1, 0, 2).reshape(env.nS, B)
        act = ro.act.permute(1, 0, 2).reshape(env.nA, B)
        logp, val = ro.logp.reshape(-1), ro.val[:T].reshape(-1).contiguous()
        adv, ret = ppos["vector"].adv.reshape(-1), ppos["vector"].ret.reshape(-1)
        an = torch.stack((adv[idx].mean(), 1.0 / (adv[idx].std() + 1e-8)))
        ps = ppos["vector"]._fused[0]
        for k in order:
            ts = []
            for _ in range(23):
                t, _ = timed(lambda: fns[k](ps, obs, act, logp, val, adv, ret, an, idx=idx), torch)
                ts.append(t * 1e3)
            if r:
                us[k].append(statistics.median(ts[3:]))
        ro.roll_over()

    def summary(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) - min(v), "all": v}

    res["update_ms"] = {k: summary(v) for k, v in ms.items()}
    res["grad_us"] = {k: summary(v) for k, v in us.items()}
    res["grad_us"]["samples"] = B // 4
    res["grad_speedup_median"] = res["grad_us"]["vector"]["median"] / res["grad_us"]["matrix"]["median"]
    res["update_speedup_median"] = res["update_ms"]["vector"]["median"] / res["update_ms"]["matrix"]["median"]
    flop = 6 * (env.nS * 64 + 64 * 64 + 64 * (env.nA + 1)) * (B // 4)
    res["flop"] = {"per_minibatch": flop, "roofline_tflops": MATRIX_FP32_TFLOPS,
                   "of_matrix_fp32_roofline": {k: flop / res["grad_us"][k]["median"] / 1e6 / MATRIX_FP32_TFLOPS for k in ("vector", "matrix")}}
    res["end_to_end"] = {}
    for k in ("vector", "matrix"):
        col = FusedPolicyCollector(env, pols[k], T)
        rates = []
        for r in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            col.collect()
            ppos[k].update(col)
            col.roll_over()
            torch.cuda.synchronize()
            if r:
                rates.append(N * T / (time.perf_counter() - t0))
        res["end_to_end"][f"f16_shared/{k}"] = {"env_steps_per_s_median": statistics.median(rates), "all": rates}
    env.close()
    finish(res, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--value-network", dest="value_network", default="copy", choices=["copy", "shared"])
    ap.add_argument("--fused-optimizer", dest="fused_optimizer", action="store_true")
    ap.add_argument("--matrix-learner", dest="matrix_learner", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.matrix_learner:
        return main_matrix(args)
    if args.fused_optimizer:
        return main_optimizer(args)
    import torch

    import gym_reinmav_amd as g
    from gym_reinmav_amd.ppo import PPO, FusedPolicyCollector, MlpPolicy

    torch.manual_seed(0)
    N, T = args.envs, args.steps
    shared = args.value_network == "shared"
    res = {"shape": {"kind": "quad3d", "envs": N, "steps": T, "epochs": 4, "minibatches": 4, "minibatch": N * T // 4},
           "device": torch.cuda.get_device_name(0)}
    if shared:
        res["shape"]["value_network"] = "shared"
    env = g.BatchedQuadrotor("quad3d", N, seed=0)
    pols = {"torch": MlpPolicy(env.nS, env.nA, value_network=args.value_network).cuda()}
    pols["fused"] = copy.deepcopy(pols["torch"])
    ppos = {k: PPO(p, fused_learner=(k == "fused")) for k, p in pols.items()}
    ro = FusedPolicyCollector(env, pols["torch"], T)
    ms = {"torch": [], "fused": []}
    for r in range(args.rounds + 1):   # round 0 warms both paths up (allocator, lazy initialisation)
        ro.collect()
        for k in ("torch", "fused") if r % 2 == 0 else ("fused", "torch"):
            t, st = timed(lambda: ppos[k].update(ro), torch)
            if r:
                ms[k].append(t)
        ro.roll_over()
    res["update_ms"] = {k: {"median": statistics.median(v), "min": min(v), "all": v} for k, v in ms.items()}
    res["update_speedup_median"] = res["update_ms"]["torch"]["median"] / res["update_ms"]["fused"]["median"]

    # one rmav_ppo_grad (shared: rmav_ppo_grad_shared) call on one minibatch of the last rollout
    ppo = ppos["fused"]
    B = N * T
    obs = ro.obs[:T].permute(1, 0, 2).reshape(env.nS, B)
    act = ro.act.permute(1, 0, 2).reshape(env.nA, B)
    logp, val = ro.logp.reshape(-1), ro.val[:T].reshape(-1).contiguous()
    adv, ret = ppo.adv.reshape(-1), ppo.ret.reshape(-1)
    idx = torch.randperm(B, device="cuda")[:B // 4]
    ts = []
    for _ in range(23):
        t, _ = timed(lambda: ppo._fused_step(env, obs, act, logp, val, adv, ret, idx), torch)
        ts.append(t * 1e3)
    step_us = statistics.median(ts[3:])
    an = torch.stack((adv[idx].mean(), 1.0 / (adv[idx].std() + 1e-8)))
    ps, flat, _, stats = ppo._fused

    def grad_call_us(fn, ps, out):
        ts = []
        for _ in range(23):
            t, _ = timed(lambda: fn(ps, obs, act, logp, val, adv, ret, an, idx=idx, out=out), torch)
            ts.append(t * 1e3)
        return statistics.median(ts[3:])

    grad_us = grad_call_us(env.ppo_grad_shared if shared else env.ppo_grad, ps, (flat, stats))
    if shared:
        flop = 6 * (env.nS * 64 + 64 * 64 + 64 * (env.nA + 1)) * (B // 4)
        res["grad_us"] = {"rmav_ppo_grad_shared": grad_us, "with_adv_moments_and_grad_views": step_us, "samples": B // 4}
        cps = PPO(MlpPolicy(env.nS, env.nA).cuda(), fused_learner=True)._fused_params()   # the copy learner on the same minibatch
        res["grad_us"]["rmav_ppo_grad_copy_same_session"] = grad_call_us(env.ppo_grad, cps, None)
        res["flop_of_copy"] = flop / (6 * (2 * env.nS * 64 + 2 * 64 * 64 + 64 * env.nA + 64) * (B // 4))
    else:
        flop = 6 * (2 * env.nS * 64 + 2 * 64 * 64 + 64 * env.nA + 64) * (B // 4)
        res["grad_us"] = {"rmav_ppo_grad": grad_us, "with_adv_moments_and_grad_views": step_us, "samples": B // 4}
    res["flop"] = {"per_minibatch": flop, "tflops": flop / grad_us / 1e6, "of_matrix_fp32_roofline": flop / grad_us / 1e6 / MATRIX_FP32_TFLOPS,
                   "of_vector_fma_rate": flop / grad_us / 1e6 / (MATRIX_FP32_TFLOPS / 2), "roofline_tflops": MATRIX_FP32_TFLOPS}

    # end to end: collect + update, per actor and path
    res["end_to_end"] = {}
    for actor, kw in ((("f16_shared", {}),) if shared else (("fp32_mfma", {}), ("f16_pair", {"f16_mfma": True}))):
        for k in ("torch", "fused"):
            col = FusedPolicyCollector(env, pols[k], T, **kw)
            rates = []
            for r in range(4):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                col.collect()
                ppos[k].update(col)
                col.roll_over()
                torch.cuda.synchronize()
                if r:
                    rates.append(N * T / (time.perf_counter() - t0))
            res["end_to_end"][f"{actor}/{k}"] = {"env_steps_per_s_median": statistics.median(rates), "all": rates}
    env.close()
    finish(res, args.out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Train / save / load / play with the batched envs - the flow of the reference's entry point
(`python -m gym_reinmav.run --alg=ppo2 --env=quadrotor3d-v0 --num_timesteps=... --save_path=... [--load_path=...] [--play]`,
gym_reinmav/run.py:186-211) on top of this library, with the same flag names.  baselines / TensorFlow are third party and
absent; the learner is gym_reinmav_amd.ppo.PPO (baselines' ppo2 defaults), the model file is a torch state_dict.

    python examples/train_ppo2.py --env quadrotor3d-v0 --num_env 8192 --num_timesteps 2e7 --save_path /tmp/quad3d.pt
    python examples/train_ppo2.py --env quadrotor3d-v0 --load_path /tmp/quad3d.pt --num_timesteps 0 --play
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "reinmav-gym_amd"))
import torch

import gym_reinmav_amd as g
from gym_reinmav_amd.evaluate import evaluate_policy
from gym_reinmav_amd.obs_norm import RunningObsNorm
from gym_reinmav_amd.ppo import PPO, FusedPolicyCollector, MlpPolicy
from gym_reinmav_amd.ret_norm import RunningReturnNorm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="quadrotor3d-v0", choices=sorted(g.ENV_IDS))
    ap.add_argument("--num_env", type=int, default=8192, help="envs on this GPU (the reference: SubprocVecEnv workers)")
    ap.add_argument("--num_timesteps", type=float, default=2e7)
    ap.add_argument("--nsteps", type=int, default=64, help="env-steps per env and rollout")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reward_scale", type=float, default=None, help="default 0.05, or 1 with --normalize-reward")
    ap.add_argument("--actor", default="f16", choices=["fp32", "bf16", "f16"], help="arithmetic of the in-kernel actor")
    ap.add_argument("--max_episode_steps", type=int, default=0, help="episode time limit H (gym's TimeLimit, inside the kernels); 0 = none")
    ap.add_argument("--bootstrap_truncated", action="store_true",
                    help="with --max_episode_steps: value targets of truncated steps are r + gamma V(s_final) instead of r")
    ap.add_argument("--normalize-obs", dest="normalize_obs", action="store_true",
                    help="VecNormalize(ob=True) in front of the nets, inside the rollout kernel (statistics frozen per rollout); "
                         "with --max_episode_steps it needs --bootstrap_truncated; not with --actor bf16")
    ap.add_argument("--normalize-reward", dest="normalize_reward", action="store_true",
                    help="VecNormalize(ret=True) in front of GAE: rewards divided by the running std of the discounted return")
    ap.add_argument("--frame-skip", dest="frame_skip", type=int, default=1,
                    help="dynamics steps per action, held inside the kernels (gym MuJoCo's frame_skip); lengths and the time limit count actions")
    ap.add_argument("--reward", default=None, metavar="SPEC",
                    help="tracking reward inside the kernels in place of the reference's -|pos|, e.g. "
                         "goal=0,0,2:alive=1:w_pos=1:w_vel=0.1:w_act=0.01:terminal=-10 (goal defaults to the controller's set-point, act_ref to "
                         "the hover action); not with --actor bf16")
    ap.add_argument("--disturbance", default=None, metavar="SPEC",
                    help="wind and gusts drawn and applied inside the step kernels, e.g. wind=-1:1,-1:1,0:0:gust=0.5,0.5,0.2:hold=25 (per-episode "
                         "wind lo:hi per axis, gust amplitude per axis, agent steps a gust is held; m/s^2); not with --actor bf16")
    ap.add_argument("--sensor-noise", default=None, metavar="SIGMA[,SIGMA...]",
                    help="Gaussian noise on every observation, drawn inside the kernels: one standard deviation for all components or one per "
                         "component, e.g. 0.01; the in-kernel actor acts on the noisy observation it stores (the fp32 matrix-core actor only)")
    ap.add_argument("--actuator-tau", type=float, default=None, metavar="SECONDS",
                    help="actuator lag inside the kernels: a first-order filter with this time constant between every action and the "
                         "dynamics, e.g. 0.05, starting each episode from the hover action; not with --actor bf16")
    ap.add_argument("--start-state", default=None, metavar="LO:HI[,LO:HI...]",
                    help="the range every episode's start state is drawn from, inside the kernels: one pair per state component, or a single "
                         "pair for all of them, e.g. -0.1:0.1; default: the reference's U[-1, 1) on every component; not with --actor bf16")
    ap.add_argument("--termination", default=None, metavar="box=LO:HI,LO:HI[,LO:HI][:tilt=RAD]",
                    help="termination rules inside the kernels, ORed into the env's own: a per-axis position box (inf = no bound), a tilt "
                         "limit in radians, and always a finiteness test, e.g. box=-2:2,-2:2,0.3:inf:tilt=1.2; not with --actor bf16")
    ap.add_argument("--randomize", action="append", default=[], metavar="NAME=LO:HI",
                    help="per-episode domain randomisation inside the kernels, e.g. mass=0.8:1.2 (mass | load_mass | tether_length; "
                         "repeatable); not with --actor bf16")
    ap.add_argument("--clip-actions", dest="clip_actions", action="store_true",
                    help="the dynamics take clip(action, Box.low, Box.high), inside the kernel; the learner keeps the unclipped action and "
                         "its log-probability (stable-baselines' PPO2 runner); not with --actor bf16")
    ap.add_argument("--eval-every", dest="eval_every", type=int, default=0, metavar="K",
                    help="every K iterations: the deterministic (mean-action, clipped) return of the policy on a separate eval env "
                         "with the same seed base, time limit and ranges (evaluate_policy); not with --actor bf16")
    ap.add_argument("--eval-envs", dest="eval_envs", type=int, default=1024, metavar="M")
    ap.add_argument("--eval-steps", dest="eval_steps", type=int, default=0,
                    help="steps of an evaluation; default --max_episode_steps (every env then finishes one episode), 256 without one")
    ap.add_argument("--value-network", dest="value_network", default="copy", choices=["copy", "shared"],
                    help="copy: a separate value net of the policy's shape; shared: a value head on the policy's latent (what baselines "
                         "builds for these envs), collected by the f16 shared-trunk actor whatever --actor says (not with --actor bf16)")
    ap.add_argument("--fused-learner", dest="fused_learner", action="store_true",
                    help="every minibatch's loss and gradients from the fused learner (rmav_ppo_grad, or rmav_ppo_grad_shared with "
                         "--value-network shared) instead of torch autograd; the all-reduce, the norm clip and Adam stay in torch")
    ap.add_argument("--fused-optimizer", dest="fused_optimizer", action="store_true",
                    help="with --fused-learner: the advantage moments, the norm clip and Adam in HIP too (rmav_adv_moments, rmav_ppo_adam: "
                         "one launch instead of clip_grad_norm_ + Adam.step()); the optimiser's state stays torch.optim.Adam's")
    ap.add_argument("--matrix-learner", dest="matrix_learner", action="store_true",
                    help="with --fused-learner and --value-network shared: the fused learner's products on the fp32 matrix cores "
                         "(rmav_ppo_grad_shared_mfma); the same precision class, another order of summation")
    ap.add_argument("--save_path", default=None)
    ap.add_argument("--load_path", default=None)
    ap.add_argument("--play", action="store_true", help="after training: run the policy (mean action) on one env and print its path")
    args = ap.parse_args()
    if args.reward_scale is None:
        args.reward_scale = 1.0 if args.normalize_reward else 0.05

    torch.manual_seed(args.seed)
    kind = g.ENV_IDS[args.env]
    if args.bootstrap_truncated and not args.max_episode_steps:
        ap.error("--bootstrap_truncated needs --max_episode_steps")
    if args.fused_optimizer and not args.fused_learner:
        ap.error("--fused-optimizer needs --fused-learner")
    if args.matrix_learner and not (args.fused_learner and args.value_network == "shared"):
        ap.error("--matrix-learner needs --fused-learner and --value-network shared")
    if args.value_network == "shared" and args.actor == "bf16":
        ap.error("--value-network shared runs on the f16 shared-trunk actor, not with --actor bf16")
    randomize = {}
    for item in args.randomize:
        try:
            name, rng = item.split("=")
            lo, hi = (float(v) for v in rng.split(":"))
        except ValueError:
            ap.error(f"--randomize wants NAME=LO:HI, got {item!r}")
        randomize[name] = (lo, hi)
    try:
        reward = g.TrackingReward.parse(args.reward) if args.reward is not None else None
    except (TypeError, ValueError) as e:
        ap.error(str(e))
    try:
        disturbance = g.Disturbance.parse(args.disturbance) if args.disturbance is not None else None
    except (TypeError, ValueError) as e:
        ap.error(str(e))
    try:
        sensor_noise = g.SensorNoise.parse(args.sensor_noise) if args.sensor_noise is not None else None
    except (TypeError, ValueError) as e:
        ap.error(str(e))
    try:
        actuator = g.Actuator(args.actuator_tau) if args.actuator_tau is not None else None
    except (TypeError, ValueError) as e:
        ap.error(str(e))
    try:
        start_state = g.StartState.parse(args.start_state) if args.start_state is not None else None
    except (TypeError, ValueError) as e:
        ap.error(str(e))
    try:
        termination = g.Termination.parse(args.termination) if args.termination is not None else None
    except (TypeError, ValueError) as e:
        ap.error(str(e))
    env = g.BatchedQuadrotor(kind, args.num_env, seed=args.seed, max_episode_steps=args.max_episode_steps or None,
                             randomize=randomize or None, frame_skip=args.frame_skip, reward=reward, disturbance=disturbance,
                             sensor_noise=sensor_noise, actuator=actuator, start_state=start_state, termination=termination)
    obs_norm = RunningObsNorm(env.nS, f"cuda:{env.device}") if args.normalize_obs else None   # run.py:91-92 VecNormalize(env)
    ret_norm = RunningReturnNorm(f"cuda:{env.device}") if args.normalize_reward else None   # ... and its ret=True half
    policy = MlpPolicy(env.nS, env.nA, value_network=args.value_network, obs_norm=obs_norm).cuda()
    if args.load_path:                                      # run.py:188 model.load(load_path)
        policy.load_state_dict(torch.load(args.load_path, map_location="cuda"))
        if obs_norm is not None and os.path.exists(args.load_path + ".obs_norm"):
            obs_norm.load_state_dict(torch.load(args.load_path + ".obs_norm"))
        if ret_norm is not None and os.path.exists(args.load_path + ".ret_norm"):
            ret_norm.load_state_dict(torch.load(args.load_path + ".ret_norm"))
    elif kind in ("quad3d", "quad3d_sl"):
        with torch.no_grad():
            policy.pi[2].bias[0] = 9.8                      # start around hover thrust
    actor_kw = dict(bf16_mfma=(args.actor == "bf16"), f16_mfma=(args.actor == "f16"))
    collector = FusedPolicyCollector(env, policy, args.nsteps, bootstrap_truncated=args.bootstrap_truncated, clip_actions=args.clip_actions,
                                     **actor_kw)
    eval_env = None
    if args.eval_every > 0:   # its own handle: the training envs' states, episode clocks and statistics are not disturbed
        eval_env = g.BatchedQuadrotor(kind, args.eval_envs, seed=args.seed, env_id_base=args.num_env,
                                      max_episode_steps=args.max_episode_steps or None, randomize=randomize or None,
                                      frame_skip=args.frame_skip, reward=reward, disturbance=disturbance, sensor_noise=sensor_noise,
                                      actuator=actuator, start_state=start_state, termination=termination)
    learner = PPO(policy, lr=1e-3, reward_scale=args.reward_scale, ret_norm=ret_norm, fused_learner=args.fused_learner,
                  fused_optimizer=args.fused_optimizer, matrix_learner=args.matrix_learner)
    iters = int(args.num_timesteps // (args.num_env * args.nsteps))
    t0 = time.perf_counter()
    for it in range(iters):
        env.episode_totals(clear=True)
        collector.collect()                                 # one kernel launch: policy + env for nsteps steps of every env
        stats = learner.update(collector)                   # GAE + clipped-surrogate epochs
        collector.roll_over()
        if it % 10 == 0 or it == iters - 1:
            tot = env.episode_totals()
            print(f"iter {it:4d}  timesteps {(it + 1) * args.num_env * args.nsteps:.3g}  eprewmean {tot['return_sum'] / max(1, tot['episodes']):8.2f}  "
                  f"eplenmean {tot['length_sum'] / max(1, tot['episodes']):7.1f}  explained_variance {stats['explained_variance']:.3f}  "
                  f"{(it + 1) * args.num_env * args.nsteps / (time.perf_counter() - t0):.3g} steps/s", flush=True)
        if eval_env is not None and ((it + 1) % args.eval_every == 0 or it == iters - 1):
            ev = evaluate_policy(policy, eval_env, n_steps=args.eval_steps or args.max_episode_steps or 256, **actor_kw)
            print(f"iter {it:4d}  eval (deterministic, clipped): mean_return {ev['mean_return']:8.2f} +- {ev['std_return']:.2f}  "
                  f"mean_length {ev['mean_length']:7.1f}  episodes {ev['episodes']}  unfinished {ev['unfinished']}", flush=True)
    if eval_env is not None:
        eval_env.close()
    env.close()
    if args.save_path:                                      # run.py:186 model.save(save_path)
        torch.save(policy.state_dict(), args.save_path)
        if obs_norm is not None:                            # the statistics belong to the weights
            torch.save(obs_norm.state_dict(), args.save_path + ".obs_norm")
        if ret_norm is not None:
            torch.save(ret_norm.state_dict(), args.save_path + ".ret_norm")
        print("saved", args.save_path)
    if args.play:                                           # run.py:190-211: obs = env.reset(); loop model.step / env.step
        if obs_norm is not None:
            obs_norm.freeze = True                          # evaluation: the policy keeps normalising, the statistics stop moving
        venv = g.QuadrotorVecEnv(args.env, 1, seed=args.seed)
        obs = venv.reset()
        ep_rew = 0.0
        for k in range(400):
            with torch.no_grad():
                mean, _ = policy(obs.t().contiguous())      # the policy is feature-major: obs [nS, N]
            obs, rew, done, _ = venv.step(mean.t().contiguous())
            ep_rew += float(rew[0])
            if bool(done[0]):
                print(f"episode_rew={ep_rew:.2f} after {k + 1} steps")
                ep_rew = 0.0
        print("final obs", [round(float(x), 3) for x in obs[0]])
        venv.close()


if __name__ == "__main__":
    main()

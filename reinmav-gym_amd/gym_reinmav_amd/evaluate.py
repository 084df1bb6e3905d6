"""Evaluation of a policy through the fused rollout kernels: stable-baselines' ``evaluate_policy`` / ``predict(deterministic=True)`` for
the batched envs.  The launches run under the env's action rule (``BatchedQuadrotor.set_policy_action_rule``: mean action, clipped to
the action space), store neither actions nor observations, and the episode statistics are reduced on the device."""
from __future__ import annotations

import torch


def first_episode_stats(rew, done, carry=None):
    """Return and length of the FIRST episode every env finishes inside time-major ``rew`` / ``done`` ``[T, N]`` (``done`` != 0 = the
    episode ended with step t) -> ``(returns [N] f32, lengths [N] i64, finished [N] bool)``.  An env that has not finished holds its
    running return and length so far, so the result is the ``carry`` of the next chunk: chunk by chunk gives the bits of one call over
    the whole array (the rewards are added in step order, in fp32 - the order the kernels' own episode return uses).  Only each env's
    first episode counts: taking the first n episodes to finish across a batch would favour the short ones.  Pure torch; CPU or GPU."""
    T, N = rew.shape
    if carry is None:
        ret = torch.zeros(N, dtype=torch.float32, device=rew.device)
        length = torch.zeros(N, dtype=torch.int64, device=rew.device)
        fin = torch.zeros(N, dtype=torch.bool, device=rew.device)
    else:
        ret, length, fin = (x.clone() for x in carry)
    rew = rew.to(torch.float32)
    for t in range(T):
        live = ~fin
        ret = torch.where(live, ret + rew[t], ret)
        length = length + live
        fin = fin | (live & (done[t] != 0))
    return ret, length, fin


def evaluate_policy(policy, env, n_steps=None, deterministic=True, clip_actions=True, chunk=64, **actor_kw):
    """Runs ``policy`` on ``env`` from ``env.reset()`` for ``n_steps`` steps of fused launches (at most ``chunk`` steps each) and returns
    the statistics of every env's first episode: ``mean_return``, ``std_return`` (population), ``mean_length`` over the envs that
    finished one, ``episodes`` (their number), ``unfinished``, and the device tensors ``returns`` / ``lengths`` ``[N]`` (running values
    where ``finished`` is False) with ``finished``.

    ``n_steps`` defaults to ``env.max_episode_steps`` - every env then finishes exactly one episode - and is required without a time
    limit.  ``deterministic`` / ``clip_actions`` and ``actor_kw`` (``f16_mfma=True`` ...) are :class:`~gym_reinmav_amd.ppo.FusedPolicyCollector`'s.
    The launches store only rewards, dones, log-probabilities and values; a policy's ``obs_norm`` statistics are read, never updated.
    The env is left wherever the rollout ended, with this call's action rule set."""
    from .ppo import FusedPolicyCollector

    limit = getattr(env, "max_episode_steps", None)
    if n_steps is None:
        if not limit:
            raise ValueError("n_steps is required on an env without max_episode_steps")
        n_steps = limit
    n_steps, chunk = int(n_steps), int(chunk)
    if n_steps <= 0 or chunk <= 0:
        raise ValueError("n_steps and chunk must be > 0")
    env.reset(layout="soa", device_out=True)
    col = FusedPolicyCollector(env, policy, min(chunk, n_steps), deterministic=deterministic, clip_actions=clip_actions, store_trajectory=False,
                               bootstrap_truncated=bool(limit) and getattr(policy, "obs_norm", None) is not None, **actor_kw)
    carry = None
    with torch.no_grad():
        for s in range(0, n_steps, col.T):
            k = min(col.T, n_steps - s)
            col.collect(k)
            carry = first_episode_stats(col.rew[:k], col.done[:k], carry)
        ret, length, fin = carry
        n_fin = int(fin.sum())
        r64, l64 = ret[fin].double(), length[fin].double()
        nan = float("nan")
        return {"mean_return": float(r64.mean()) if n_fin else nan, "std_return": float(r64.std(unbiased=False)) if n_fin else nan,
                "mean_length": float(l64.mean()) if n_fin else nan, "episodes": n_fin, "unfinished": int(fin.numel()) - n_fin,
                "returns": ret, "lengths": length, "finished": fin}

"""Running return statistics - the reward half of baselines' ``VecNormalize(ret=True)`` (third party, restated from memory in
``include/rmav_ppo.h``) - in the one small buffer the HIP kernels read.

baselines keeps one discounted return ``R = gamma R + rew`` per env (zeroed at every ``done`` and at ``reset()``), feeds every ``R``
into ONE scalar ``RunningMeanStd`` and divides the reward by ``sqrt(var + eps)`` (no mean subtraction), clipped to ``+-cliprew``.
``RunningReturnNorm`` owns that statistics buffer (``rmav_ret_norm_bytes()`` = 64 bytes; field offsets in ``include/rmav_ppo.h``):
the running state in fp64 (``count``, ``mean``, ``m2`` with ``var = m2 / count``), the settings, and the fp32 table ``rstd_f``,
``clip_f`` every consumer reads - ``rmav_gae_norm`` inside the GAE launch, ``rmav_ret_normalize`` for stored rewards, ``normalize``
in torch.  All of them compute ``clamp((reward_scale * r) * rstd_f, -clip, clip)`` in fp32, in this order.

The ``[N]`` carry ``R`` belongs to an env batch, not to the statistics (several collectors may feed one object): it is kept here
keyed by the env object - ``carry(env)``, zeros on first use, ``reset_carry(env)`` - and is not part of ``state_dict()``
(baselines does not save it either).

**Order.**  ``PPO.update`` merges rollout k's returns first and then scales rollout k's rewards with statistics that already include
them - baselines' order at rollout granularity (the reward statistics are only needed after the rollout, unlike the observation
statistics of ``obs_norm.py``).  What remains different: all T steps of a rollout share one scale, where baselines scales step t
with the statistics through step t.  ``vec_env.VecNormalize(norm_reward=True)`` has a meeting point per step and keeps baselines'
exact order.

On a GPU an update is ``rmav_ret_moments`` -> (all-gather of 3 doubles per rank) -> ``rmav_ret_norm_merge`` on the env's stream, with
no host synchronisation; only the ``count`` / ``mean`` / ``var`` properties and ``state_dict()`` read the buffer back.  For CPU
tensors the same rule runs in torch float64 (carry included; what the host-only tests exercise).
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np
import torch

from ._running import RunningStats

N_BYTES = 64   # rmav_ret_norm_bytes()
REC = 3        # a batch record: count, mean, m2


class RunningReturnNorm(RunningStats):
    N_BYTES, N_FEAT = N_BYTES, 1
    _OFF = {"count": 0, "mean": 8, "m2": 16, "eps": 24, "clip": 32, "rstd_f": 48, "clip_f": 52}
    _WHAT = "rewards"
    _BAD_STATE = "state_dict of another buffer layout"

    def __init__(self, device="cpu", gamma: float = 0.99, clip: float = 10.0, eps: float = 1e-8, count0: float = 1e-4):
        """``gamma``: the discount of the return carry (baselines: 0.99); ``clip``: baselines' ``cliprew`` (``float('inf')`` = none);
        ``eps``: the epsilon under the square root; ``count0``: the count the statistics start from (mean 0, var 1).
        ``freeze = True`` turns ``update`` into a no-op (evaluation)."""
        super().__init__(1, device, clip, eps, count0)
        self.gamma = float(gamma)
        self._carry = {}      # id(env) -> (weak reference or None, R [N])

    # ---- what the consumers read: views of the buffer (no copy, no synchronisation, valid under graph replay) -------------------------
    @property
    def rstd_f(self) -> torch.Tensor:
        return self._rstd_f[0]

    @property
    def clip_f(self) -> torch.Tensor:
        return self._clip_f[0]

    # ---- the running state (these synchronise) -----------------------------------------------------------------------------------------
    @property
    def mean(self) -> float:
        return float(self._mean.cpu()[0])

    @property
    def var(self) -> float:
        return float(self._m2.cpu()[0] / self._count.cpu()[0])

    def state_dict(self) -> dict:
        """the whole buffer (state, settings and table: a round trip is exact) and gamma; the per-env carry is not part of it"""
        return {"gamma": self.gamma, **super().state_dict()}

    def load_state_dict(self, sd: dict):
        super().load_state_dict(sd)
        self.gamma = float(sd["gamma"])

    # ---- the per-env discounted return ----------------------------------------------------------------------------------------------------
    def carry(self, env, like: torch.Tensor = None) -> torch.Tensor:
        """``R [N]`` of the env batch ``env`` (any object; ``None`` is one anonymous batch): zeros on first use.  float32 on the
        statistics' device for a ``BatchedQuadrotor``, else shaped after ``like`` (``[N]``; float64 for CPU tensors)."""
        ent = self._carry.get(id(env))
        if ent is not None and (ent[0] is None or ent[0]() is env):
            return ent[1]
        if like is not None and not like.is_cuda:
            R = torch.zeros(like.shape[-1], dtype=torch.float64)
        else:
            R = torch.zeros(env.num_envs if like is None else like.shape[-1], dtype=torch.float32, device=self.device)
        ref = None
        if env is not None:
            try:
                key = id(env)
                ref = weakref.ref(env, lambda _r, k=key, d=self._carry: d.pop(k, None))
            except TypeError:   # an object that takes no weak reference: its entry lives as long as the statistics
                ref = None
        self._carry[id(env)] = (ref, R)
        return R

    def reset_carry(self, env=None):
        """``R <- 0`` for the batch of ``env`` (after ``env.reset()``), in place"""
        ent = self._carry.get(id(env))
        if ent is not None and (ent[0] is None or ent[0]() is env):
            ent[1].zero_()

    # ---- normalise ------------------------------------------------------------------------------------------------------------------------
    def normalize(self, rew: torch.Tensor, reward_scale: float = 1.0, env=None, out=None):
        """``clamp((rew * reward_scale) * rstd_f, -clip, clip)`` in fp32.  With ``env`` (a ``BatchedQuadrotor``) and a contiguous CUDA
        tensor it is one launch of ``rmav_ret_normalize`` on the env's stream; otherwise the torch expression - the same bits for
        finite rewards.  ``out`` may be ``rew``."""
        if env is not None and rew.is_cuda:
            from . import _abi as A

            dst = torch.empty_like(rew) if out is None else out
            assert rew.dtype == torch.float32 and rew.is_contiguous() and dst.dtype == torch.float32 and dst.is_contiguous()
            assert dst.shape == rew.shape
            A.check(A.lib().rmav_ret_normalize(env._h, C.c_void_p(self.data_ptr()), C.c_void_p(rew.data_ptr()), C.c_void_p(dst.data_ptr()),
                                               rew.numel(), float(reward_scale)))
            return dst
        z = (rew * float(reward_scale)) * self.rstd_f
        c = self.clip_f
        return torch.clamp(z, -c, c, out=out) if out is not None else torch.clamp(z, -c, c)

    # ---- update ---------------------------------------------------------------------------------------------------------------------------
    def update(self, rew: torch.Tensor, done: torch.Tensor, env=None, reward_scale: float = 1.0, group=None):
        """Runs the discounted-return recurrence of ``env``'s batch over ``rew`` / ``done`` (``[T, N]`` time-major, or ``[N]`` = one
        step) and merges the T x N returns into the running statistics with RunningMeanStd's rule.  CUDA tensors need ``env`` (the
        ``BatchedQuadrotor`` whose batch this is): scan and merge are launches on its stream.  ``group`` (or the default process group,
        when one is initialised) with more than one rank: every rank's 3-double record is all-gathered and merged in rank order, so
        all ranks end with the same bits."""
        if rew.dim() == 1:
            rew, done = rew[None], done[None]
        return self._update(env, group, rew, done, float(reward_scale))

    def _moments_gpu(self, env, rec, rew, done, scale):
        from . import _abi as A

        T, N = rew.shape
        assert tuple(done.shape) == (T, N) and N == env.num_envs
        assert rew.dtype == torch.float32 and rew.is_contiguous() and done.is_contiguous() and done.element_size() == 1
        A.check(A.lib().rmav_ret_moments(env._h, T, C.c_void_p(rew.data_ptr()), C.c_void_p(done.data_ptr()), scale, self.gamma,
                                         C.c_void_p(self.carry(env).data_ptr()), rec))

    def _merge_gpu(self, env, recs, n):
        from . import _abi as A

        A.check(A.lib().rmav_ret_norm_merge(env._h, C.c_void_p(self.data_ptr()), recs, n))

    def _moments_cpu(self, env, rew, done, scale):
        T, N = rew.shape
        assert tuple(done.shape) == (T, N)
        R = self.carry(env, like=rew)
        x, d = rew.detach().to(torch.float64) * float(np.float32(scale)), done != 0   # the kernels take the scale as a float
        rets = torch.empty_like(x)
        for t in range(T):
            R.mul_(self.gamma).add_(x[t])
            rets[t] = R
            R[d[t]] = 0.0
        rec = torch.zeros(REC, dtype=torch.float64)
        B = rets.numel()
        rec[0] = B
        if B:
            rec[1] = rets.mean()
            rec[2] = rets.var(unbiased=False) * B
        return rec

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
import torch.distributed as dist

N_BYTES = 64   # rmav_ret_norm_bytes()
REC = 3        # a batch record: count, mean, m2
_O_COUNT, _O_MEAN, _O_M2, _O_EPS, _O_CLIP, _O_RSTD_F, _O_CLIP_F = 0, 8, 16, 24, 32, 48, 52


class RunningReturnNorm:
    def __init__(self, device="cpu", gamma: float = 0.99, clip: float = 10.0, eps: float = 1e-8, count0: float = 1e-4):
        """``gamma``: the discount of the return carry (baselines: 0.99); ``clip``: baselines' ``cliprew`` (``float('inf')`` = none);
        ``eps``: the epsilon under the square root; ``count0``: the count the statistics start from (mean 0, var 1).
        ``freeze = True`` turns ``update`` into a no-op (evaluation)."""
        if not clip > 0 or not eps >= 0 or not count0 > 0:
            raise ValueError("clip must be > 0 (inf = no clip), eps >= 0, count0 > 0")
        self.gamma, self.device, self.freeze = float(gamma), torch.device(device), False
        host = np.zeros(N_BYTES, np.uint8)
        f64 = host[:_O_CLIP].view(np.float64)
        f64[0], f64[1], f64[2], f64[3] = count0, 0.0, count0, eps   # var = 1
        host[_O_CLIP:_O_CLIP + 4].view(np.float32)[0] = clip
        host[_O_RSTD_F:_O_RSTD_F + 4].view(np.float32)[0] = np.float32(1.0 / np.sqrt(1.0 + eps))
        host[_O_CLIP_F:_O_CLIP_F + 4].view(np.float32)[0] = clip
        self.buf = torch.zeros(N_BYTES, dtype=torch.uint8, device=self.device)
        assert self.buf.data_ptr() % 16 == 0
        b = self.buf
        self._state = b[_O_COUNT:_O_EPS].view(torch.float64)   # count, mean, m2
        self._rstd_f = b[_O_RSTD_F:_O_RSTD_F + 4].view(torch.float32)[0]
        self._clip_f = b[_O_CLIP_F:_O_CLIP_F + 4].view(torch.float32)[0]
        self._eps, self._clip = float(eps), float(np.float32(clip))
        self._batch = None    # device records of update(): [world, 3] float64
        self._carry = {}      # id(env) -> (weak reference or None, R [N])
        self.buf.copy_(torch.from_numpy(host))

    # ---- what the consumers read: views of the buffer (no copy, no synchronisation, valid under graph replay) -------------------------
    @property
    def rstd_f(self) -> torch.Tensor:
        return self._rstd_f

    @property
    def clip_f(self) -> torch.Tensor:
        return self._clip_f

    @property
    def clip(self) -> float:
        return self._clip

    @property
    def eps(self) -> float:
        return self._eps

    def data_ptr(self) -> int:
        return self.buf.data_ptr()

    # ---- the running state (these synchronise) -----------------------------------------------------------------------------------------
    @property
    def count(self) -> float:
        return float(self._state.cpu()[0])

    @property
    def mean(self) -> float:
        return float(self._state.cpu()[1])

    @property
    def var(self) -> float:
        s = self._state.cpu()
        return float(s[2] / s[0])

    def state_dict(self) -> dict:
        """the whole buffer (state, settings and table: a round trip is exact) and gamma; the per-env carry is not part of it"""
        return {"gamma": self.gamma, "buffer": self.buf.cpu().clone()}

    def load_state_dict(self, sd: dict):
        if tuple(sd["buffer"].shape) != (N_BYTES,) or sd["buffer"].dtype != torch.uint8:
            raise ValueError("state_dict of another buffer layout")
        host = sd["buffer"].cpu().numpy()
        self.gamma = float(sd["gamma"])
        self._eps = float(host[_O_EPS:_O_CLIP].view(np.float64)[0])
        self._clip = float(host[_O_CLIP:_O_CLIP + 4].view(np.float32)[0])
        self.buf.copy_(sd["buffer"])   # in place: the pointer the kernels and captured graphs hold stays valid

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
        z = (rew * float(reward_scale)) * self._rstd_f
        neg = -self._clip_f
        return torch.clamp(z, neg, self._clip_f, out=out) if out is not None else torch.clamp(z, neg, self._clip_f)

    # ---- update ---------------------------------------------------------------------------------------------------------------------------
    def update(self, rew: torch.Tensor, done: torch.Tensor, env=None, reward_scale: float = 1.0, group=None):
        """Runs the discounted-return recurrence of ``env``'s batch over ``rew`` / ``done`` (``[T, N]`` time-major, or ``[N]`` = one
        step) and merges the T x N returns into the running statistics with RunningMeanStd's rule.  CUDA tensors need ``env`` (the
        ``BatchedQuadrotor`` whose batch this is): scan and merge are launches on its stream.  ``group`` (or the default process group,
        when one is initialised) with more than one rank: every rank's 3-double record is all-gathered and merged in rank order, so
        all ranks end with the same bits."""
        if self.freeze:
            return self
        world = 1
        if dist.is_available() and dist.is_initialized():
            world = dist.get_world_size(group)
        if rew.dim() == 1:
            rew, done = rew[None], done[None]
        T, N = rew.shape
        assert tuple(done.shape) == (T, N)
        if rew.is_cuda:
            from . import _abi as A

            if env is None:
                raise ValueError("update() of CUDA rewards needs env= (the BatchedQuadrotor they belong to)")
            assert rew.dtype == torch.float32 and rew.is_contiguous() and done.is_contiguous() and done.element_size() == 1
            assert N == env.num_envs
            R = self.carry(env)
            if self._batch is None or self._batch.shape[0] != world:
                self._batch = torch.zeros((world, REC), dtype=torch.float64, device=self.buf.device)
            rank = dist.get_rank(group) if world > 1 else 0
            A.check(A.lib().rmav_ret_moments(env._h, T, C.c_void_p(rew.data_ptr()), C.c_void_p(done.data_ptr()), float(reward_scale),
                                             self.gamma, C.c_void_p(R.data_ptr()), C.c_void_p(self._batch[rank].data_ptr())))
            if world > 1:
                dist.all_gather_into_tensor(self._batch.view(-1), self._batch[rank].clone(), group=group)
            A.check(A.lib().rmav_ret_norm_merge(env._h, C.c_void_p(self.data_ptr()), C.c_void_p(self._batch.data_ptr()), world))
            return self
        rec = self._moments_cpu(rew, done, self.carry(env, like=rew), float(reward_scale))
        recs = [rec]
        if world > 1:
            recs = [torch.zeros_like(rec) for _ in range(world)]
            dist.all_gather(recs, rec, group=group)
        for r in recs:
            self._merge_cpu(r)
        return self

    def _moments_cpu(self, rew, done, R, scale):
        T = rew.shape[0]
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

    def _merge_cpu(self, rec):
        bc = float(rec[0])
        if not bc > 0:
            return
        s = self._state
        count = float(s[0])
        tot = count + bc
        d = float(rec[1]) - float(s[1])
        s[1] += d * bc / tot
        s[2] = float(s[2]) + float(rec[2]) + d * d * count * bc / tot
        s[0] = tot
        self._rstd_f.fill_(float(np.float32(1.0 / np.sqrt(float(s[2]) / tot + self._eps))))

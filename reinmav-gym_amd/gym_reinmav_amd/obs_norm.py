"""Running observation statistics - baselines' ``VecNormalize(ob=True, ret=False)`` / ``RunningMeanStd`` (third party, restated from
memory in ``include/rmav_ppo.h``) - in the one small buffer the HIP kernels read.

``RunningObsNorm`` owns that buffer (``rmav_obs_norm_bytes()`` = 432 bytes; field offsets in ``include/rmav_ppo.h``): the running
state in fp64 (``count``, ``mean[16]``, ``m2[16]`` with ``var = m2 / count``), the settings, and the fp32 tables ``mean_f``,
``rstd_f``, ``clip_f`` every consumer reads - ``rmav_rollout_policy_norm`` inside the fused rollout, ``MlpPolicy(obs_norm=...)`` in torch,
``rmav_obs_normalize`` for stored observations.  All of them compute ``clamp((x - mean_f) * rstd_f, -clip, clip)`` in fp32, in this
order, so the learner sees exactly the numbers the actor saw.

**One deliberate difference from baselines.**  baselines updates the statistics every env-step and normalises with the statistics
of that moment.  A fused rollout launch runs T steps without a grid-wide meeting point, so inside a fused rollout the statistics
are FROZEN: rollout k is collected, and learned from, with the statistics of the rollouts before it, and absorbs its own T x N
observations afterwards (``PPO.update`` does that after its last minibatch).  The one-launch-per-step ``VecEnv`` path
(``vec_env.VecNormalize``) has a meeting point every step and keeps baselines' order: update first, then normalise.

On a GPU everything is a launch on the env's stream: an update is moments -> (all-gather of 33 doubles per rank) -> merge, with no
host synchronisation; only the ``mean`` / ``var`` / ``count`` properties and ``state_dict()`` read the buffer back.  For CPU tensors
the same update rule runs in torch float64 (what the host-only tests exercise); there is no GPU-free path behind the C ABI.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._running import RunningStats

N_FEAT = 16           # features of the buffer (the widest kind has 16 state components)
N_BYTES = 432         # rmav_obs_norm_bytes()
REC = 1 + 2 * N_FEAT  # a batch record: count, mean[16], m2[16]


class RunningObsNorm(RunningStats):
    N_BYTES, N_FEAT = N_BYTES, N_FEAT
    _OFF = {"count": 0, "mean": 8, "m2": 136, "eps": 264, "clip": 272, "mean_f": 288, "rstd_f": 352, "clip_f": 416}
    _WHAT = "observations"
    _BAD_STATE = "state_dict of another observation size / buffer layout"

    def __init__(self, n_obs: int, device="cpu", clip: float = 10.0, eps: float = 1e-8, count0: float = 1e-4):
        """``clip``: baselines' ``clipob`` (``float('inf')`` = none); ``eps``: the epsilon under the square root; ``count0``: the
        count the statistics start from (mean 0, var 1).  ``freeze = True`` turns ``update`` into a no-op (evaluation)."""
        if not 1 <= int(n_obs) <= N_FEAT:
            raise ValueError(f"n_obs must be in [1, {N_FEAT}]")
        self.n_obs = int(n_obs)
        super().__init__(n_obs, device, clip, eps, count0)
        self._mean_f = self._view("mean_f", torch.float32)

    # ---- what the consumers read: views of the buffer (no copy, no synchronisation, valid under graph replay) -------------------------
    @property
    def mean_f(self) -> torch.Tensor:
        return self._mean_f[:self.n_obs]

    @property
    def rstd_f(self) -> torch.Tensor:
        return self._rstd_f[:self.n_obs]

    @property
    def clip_f(self) -> torch.Tensor:
        return self._clip_f

    # ---- the running state (these synchronise) -----------------------------------------------------------------------------------------
    @property
    def mean(self) -> np.ndarray:
        return self._mean[:self.n_obs].cpu().numpy().copy()

    @property
    def var(self) -> np.ndarray:
        return (self._m2[:self.n_obs].cpu().numpy() / self.count).copy()

    def state_dict(self) -> dict:
        """the whole buffer (state, settings and tables: a round trip is exact) - keep it in a checkpoint beside the weights"""
        return {"n_obs": self.n_obs, **super().state_dict()}

    def load_state_dict(self, sd: dict):
        if int(sd["n_obs"]) != self.n_obs:
            raise ValueError(self._BAD_STATE)
        super().load_state_dict(sd)

    # ---- normalise ------------------------------------------------------------------------------------------------------------------------
    def normalize(self, obs: torch.Tensor, out=None, layout: str = "soa", env=None):
        """``clamp((obs - mean_f) * rstd_f, -clip, clip)`` in fp32.  ``layout='soa'``: features on the second-to-last axis (``[nS, N]``,
        ``[T, nS, N]``: what the policies take); ``'aos'``: on the last (``[N, nS]``).  With ``env`` (a ``BatchedQuadrotor`` whose batch
        this is) and contiguous CUDA tensors it is one launch of ``rmav_obs_normalize``; otherwise the torch expression - the same bits
        for finite inputs.  ``out`` may be ``obs``.  No gradient flows into the statistics."""
        m, r, c = self.mean_f, self.rstd_f, self.clip_f
        if env is not None and obs.is_cuda:
            from . import _abi as A

            dst = obs.new_empty(obs.shape) if out is None else out
            n_rows, lay, pitch = self._rows(obs, layout, env)
            assert dst.shape == obs.shape and dst.stride() == obs.stride() and dst.dtype == torch.float32
            A.check(A.lib().rmav_obs_normalize(env._h, C.c_void_p(self.data_ptr()), C.c_void_p(obs.data_ptr()), C.c_void_p(dst.data_ptr()),
                                               lay, n_rows, pitch))
            return dst
        if layout == "soa":
            m, r = m[:, None], r[:, None]
        with torch.no_grad():
            neg = -c
        z = (obs - m) * r
        return torch.clamp(z, neg, c, out=out) if out is not None else torch.clamp(z, neg, c)

    def _rows(self, obs, layout, env):
        """(n_rows, layout code, pitch) of a float32 CUDA tensor that holds whole batches of ``env``"""
        from . import _abi as A

        nS, N = self.n_obs, env.num_envs
        assert obs.dtype == torch.float32 and nS == env.nS
        if layout == "soa":
            x = obs if obs.dim() == 3 else obs[None]
            assert x.shape[1:] == (nS, N) and x.stride(2) == 1, "soa observations are [T, nS, N] / [nS, N] with unit stride along N"
            pitch = x.stride(1) if nS > 1 else N
            assert pitch >= N and (x.shape[0] == 1 or x.stride(0) == nS * pitch), "rows must be nS * pitch apart"
            return int(x.shape[0]), A.SOA, (0 if pitch == N else int(pitch))
        assert layout == "aos"
        x = obs if obs.dim() == 3 else obs[None]
        assert x.shape[1:] == (N, nS) and x.is_contiguous(), "aos observations are contiguous [T, N, nS] / [N, nS]"
        return int(x.shape[0]), A.AOS, 0

    # ---- update ---------------------------------------------------------------------------------------------------------------------------
    def update(self, obs: torch.Tensor, layout: str = "soa", env=None, group=None):
        """Merges the batch ``obs`` (``'soa'`` ``[T, nS, N]`` / ``[nS, N]`` or ``'aos'`` ``[T, N, nS]`` / ``[N, nS]``) into the running
        statistics with RunningMeanStd's rule.  CUDA tensors need ``env`` (the ``BatchedQuadrotor`` whose batch this is): moments and
        merge are launches on its stream.  ``group`` (or the default process group, when one is initialised) with more than one rank:
        every rank's 33-double record is all-gathered and merged in rank order, so all ranks end with the same bits."""
        return self._update(env, group, obs, layout)

    def _moments_gpu(self, env, rec, obs, layout):
        from . import _abi as A

        n_rows, lay, pitch = self._rows(obs, layout, env)
        A.check(A.lib().rmav_obs_moments(env._h, C.c_void_p(obs.data_ptr()), lay, n_rows, pitch, rec))

    def _merge_gpu(self, env, recs, n):
        from . import _abi as A

        A.check(A.lib().rmav_obs_norm_merge(env._h, C.c_void_p(self.data_ptr()), recs, n))

    def _moments_cpu(self, env, obs, layout):
        n = self.n_obs
        x = obs.detach().to(torch.float64)
        x = (x.movedim(-2, -1) if layout == "soa" else x).reshape(-1, n)
        rec = torch.zeros(REC, dtype=torch.float64)
        B = x.shape[0]
        rec[0] = B
        if B:
            rec[1:1 + n] = x.mean(0)
            rec[1 + N_FEAT:1 + N_FEAT + n] = x.var(0, unbiased=False) * B
        return rec

    def _merge_cpu(self, rec):
        if super()._merge_cpu(rec):
            self._mean_f[:self.n_obs] = self._mean[:self.n_obs].to(torch.float32)

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
import torch.distributed as dist

N_FEAT = 16           # features of the buffer (the widest kind has 16 state components)
N_BYTES = 432         # rmav_obs_norm_bytes()
REC = 1 + 2 * N_FEAT  # a batch record: count, mean[16], m2[16]
_O_COUNT, _O_MEAN, _O_M2, _O_EPS, _O_CLIP, _O_MEAN_F, _O_RSTD_F, _O_CLIP_F = 0, 8, 136, 264, 272, 288, 352, 416


class RunningObsNorm:
    def __init__(self, n_obs: int, device="cpu", clip: float = 10.0, eps: float = 1e-8, count0: float = 1e-4):
        """``clip``: baselines' ``clipob`` (``float('inf')`` = none); ``eps``: the epsilon under the square root; ``count0``: the
        count the statistics start from (mean 0, var 1).  ``freeze = True`` turns ``update`` into a no-op (evaluation)."""
        if not 1 <= int(n_obs) <= N_FEAT:
            raise ValueError(f"n_obs must be in [1, {N_FEAT}]")
        if not clip > 0 or not eps >= 0 or not count0 > 0:
            raise ValueError("clip must be > 0 (inf = no clip), eps >= 0, count0 > 0")
        self.n_obs, self.device, self.freeze = int(n_obs), torch.device(device), False
        host = np.zeros(N_BYTES, np.uint8)
        host[_O_COUNT:_O_MEAN].view(np.float64)[0] = count0
        host[_O_M2:_O_EPS].view(np.float64)[:] = count0                      # var = 1
        host[_O_EPS:_O_CLIP].view(np.float64)[0] = eps
        host[_O_CLIP:_O_CLIP + 4].view(np.float32)[0] = clip
        self._alloc(host)
        self._write_tables_host(host)
        self.buf.copy_(torch.from_numpy(host))

    def _alloc(self, host):
        self.buf = torch.zeros(N_BYTES, dtype=torch.uint8, device=self.device)
        assert self.buf.data_ptr() % 16 == 0
        b = self.buf
        self._count, self._mean, self._m2 = (b[_O_COUNT:_O_MEAN].view(torch.float64), b[_O_MEAN:_O_M2].view(torch.float64),
                                             b[_O_M2:_O_EPS].view(torch.float64))
        self._mean_f, self._rstd_f = b[_O_MEAN_F:_O_RSTD_F].view(torch.float32), b[_O_RSTD_F:_O_CLIP_F].view(torch.float32)
        self._clip_f = b[_O_CLIP_F:_O_CLIP_F + 4].view(torch.float32)
        self._eps = float(host[_O_EPS:_O_CLIP].view(np.float64)[0])
        self._clip = float(host[_O_CLIP:_O_CLIP + 4].view(np.float32)[0])
        self._batch = None   # device records of update(): [world, 33] float64

    def _write_tables_host(self, host):
        """tables from the fp64 state, as the merge kernel writes them (features >= n_obs: mean 0, scale 1)"""
        n = self.n_obs
        count = host[_O_COUNT:_O_MEAN].view(np.float64)[0]
        mean, m2 = host[_O_MEAN:_O_M2].view(np.float64), host[_O_M2:_O_EPS].view(np.float64)
        mf, rf = host[_O_MEAN_F:_O_RSTD_F].view(np.float32), host[_O_RSTD_F:_O_CLIP_F].view(np.float32)
        mf[:], rf[:] = 0.0, 1.0
        mf[:n] = mean[:n].astype(np.float32)
        rf[:n] = (1.0 / np.sqrt(m2[:n] / count + self._eps)).astype(np.float32)
        host[_O_CLIP_F:_O_CLIP_F + 4].view(np.float32)[0] = self._clip

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
        return float(self._count.cpu()[0])

    @property
    def mean(self) -> np.ndarray:
        return self._mean[:self.n_obs].cpu().numpy().copy()

    @property
    def var(self) -> np.ndarray:
        return (self._m2[:self.n_obs].cpu().numpy() / self.count).copy()

    def state_dict(self) -> dict:
        """the whole buffer (state, settings and tables: a round trip is exact) - keep it in a checkpoint beside the weights"""
        return {"n_obs": self.n_obs, "buffer": self.buf.cpu().clone()}

    def load_state_dict(self, sd: dict):
        if int(sd["n_obs"]) != self.n_obs or tuple(sd["buffer"].shape) != (N_BYTES,) or sd["buffer"].dtype != torch.uint8:
            raise ValueError("state_dict of another observation size / buffer layout")
        host = sd["buffer"].cpu().numpy()
        self._eps = float(host[_O_EPS:_O_CLIP].view(np.float64)[0])
        self._clip = float(host[_O_CLIP:_O_CLIP + 4].view(np.float32)[0])
        self.buf.copy_(sd["buffer"])   # in place: the pointer the kernels and captured graphs hold stays valid

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
        if self.freeze:
            return self
        world = 1
        if dist.is_available() and dist.is_initialized():
            world = dist.get_world_size(group)
        if obs.is_cuda:
            from . import _abi as A

            if env is None:
                raise ValueError("update() of CUDA observations needs env= (the BatchedQuadrotor they belong to)")
            n_rows, lay, pitch = self._rows(obs, layout, env)
            if self._batch is None or self._batch.shape[0] != world:
                self._batch = torch.zeros((world, REC), dtype=torch.float64, device=self.buf.device)
            rank = dist.get_rank(group) if world > 1 else 0
            A.check(A.lib().rmav_obs_moments(env._h, C.c_void_p(obs.data_ptr()), lay, n_rows, pitch, C.c_void_p(self._batch[rank].data_ptr())))
            if world > 1:
                dist.all_gather_into_tensor(self._batch.view(-1), self._batch[rank].clone(), group=group)
            A.check(A.lib().rmav_obs_norm_merge(env._h, C.c_void_p(self.data_ptr()), C.c_void_p(self._batch.data_ptr()), world))
            return self
        rec = self._moments_cpu(obs, layout)
        recs = [rec]
        if world > 1:
            recs = [torch.zeros_like(rec) for _ in range(world)]
            dist.all_gather(recs, rec, group=group)
        for r in recs:
            self._merge_cpu(r)
        return self

    def _moments_cpu(self, obs, layout):
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
        n, bc = self.n_obs, float(rec[0])
        if not bc > 0:
            return
        count = float(self._count[0])
        tot = count + bc
        d = rec[1:1 + n] - self._mean[:n]
        self._mean[:n] += d * bc / tot
        self._m2[:n] = self._m2[:n] + rec[1 + N_FEAT:1 + N_FEAT + n] + d * d * count * bc / tot
        self._m2[n:] = tot
        self._count[0] = tot
        self._mean_f[:n] = self._mean[:n].to(torch.float32)
        self._rstd_f[:n] = (1.0 / torch.sqrt(self._m2[:n] / tot + self._eps)).to(torch.float32)

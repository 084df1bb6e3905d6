"""What ``RunningObsNorm`` (``obs_norm.py``) and ``RunningReturnNorm`` (``ret_norm.py``) share: one small statistics buffer the
HIP kernels read - running state in fp64 (``count``, ``mean[F]``, ``m2[F]`` with ``var = m2 / count``), the settings ``eps`` and
``clip``, the fp32 tables - and RunningMeanStd's update of it: batch moments -> (all-gather of one record per rank) -> merge.

A subclass gives the layout (``N_BYTES``, ``N_FEAT`` = F, the byte offsets ``_OFF``), the two ways to a batch record ``(count, mean[F], m2[F])`` -
``_moments_gpu(env, rec_ptr, x, ...)`` (a launch) and ``_moments_cpu(env, x, ...)`` (torch float64) - and ``_merge_gpu(env, recs_ptr,
n)``, the launch that merges ``n`` records into the buffer.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.distributed as dist


class RunningStats:
    N_BYTES: int   # size of the buffer
    N_FEAT: int    # features of the buffer; a batch record has 1 + 2 * N_FEAT doubles
    _OFF: dict     # field -> byte offset: count, mean, m2, eps, clip, rstd_f, clip_f
    _WHAT: str     # what update() takes, for its error message
    _BAD_STATE: str   # the error message of load_state_dict()

    def __init__(self, n: int, device, clip: float, eps: float, count0: float):
        """``n`` <= N_FEAT features in use; the statistics start from ``count0`` samples of mean 0, var 1"""
        if not clip > 0 or not eps >= 0 or not count0 > 0:
            raise ValueError("clip must be > 0 (inf = no clip), eps >= 0, count0 > 0")
        self._n, self.device, self.freeze = int(n), torch.device(device), False
        self.buf = torch.zeros(self.N_BYTES, dtype=torch.uint8, device=self.device)
        assert self.buf.data_ptr() % 16 == 0
        self._count, self._mean, self._m2 = self._view("count", torch.float64, 1), self._view("mean"), self._view("m2")
        self._rstd_f, self._clip_f = self._view("rstd_f", torch.float32), self._view("clip_f", torch.float32, 1)
        self._batch = None   # device records of update(): [world, 1 + 2 * N_FEAT] float64
        host = torch.zeros(self.N_BYTES, dtype=torch.uint8)
        self._view("count", k=1, buf=host)[0] = count0
        self._view("m2", buf=host)[:] = count0   # var = 1
        self._view("eps", k=1, buf=host)[0] = eps
        self._view("clip", torch.float32, 1, host)[0] = clip
        self._read_settings(host)
        # the tables, as the merge kernels write them (features >= n: mean 0, scale 1)
        rstd_f = self._view("rstd_f", torch.float32, buf=host)
        rstd_f[:] = 1.0
        rstd_f[:self._n] = float(np.float32(1.0 / np.sqrt(1.0 + self._eps)))
        self._view("clip_f", torch.float32, 1, host)[0] = self._clip
        self.buf.copy_(host)

    def _view(self, name, dtype=torch.float64, k=None, buf=None):
        """``k`` (default N_FEAT) elements of the field ``name``, of ``buf`` (default: the buffer itself)"""
        o, size = self._OFF[name], 8 if dtype == torch.float64 else 4
        return (self.buf if buf is None else buf)[o:o + (self.N_FEAT if k is None else k) * size].view(dtype)

    def _read_settings(self, host):
        self._eps = float(self._view("eps", k=1, buf=host)[0])
        self._clip = float(self._view("clip", torch.float32, 1, host)[0])

    # ---- what the consumers read (no copy, no synchronisation) ---------------------------------------------------------------------------
    @property
    def clip(self) -> float:
        return self._clip

    @property
    def eps(self) -> float:
        return self._eps

    def data_ptr(self) -> int:
        return self.buf.data_ptr()

    # ---- the running state (this synchronises) -------------------------------------------------------------------------------------------
    @property
    def count(self) -> float:
        return float(self._count.cpu()[0])

    def state_dict(self) -> dict:
        """the whole buffer: state, settings and tables, so a round trip is exact"""
        return {"buffer": self.buf.cpu().clone()}

    def load_state_dict(self, sd: dict):
        if tuple(sd["buffer"].shape) != (self.N_BYTES,) or sd["buffer"].dtype != torch.uint8:
            raise ValueError(self._BAD_STATE)
        self._read_settings(sd["buffer"].cpu())
        self.buf.copy_(sd["buffer"])   # in place: the pointer the kernels and captured graphs hold stays valid

    # ---- update --------------------------------------------------------------------------------------------------------------------------
    def _update(self, env, group, x, *more):
        """RunningMeanStd's update with the batch ``x, *more`` (what the subclass's two ``_moments`` take).  CUDA: moments and merge
        are launches on ``env``'s stream.  ``group`` (or the default process group, when one is initialised) with more than one
        rank: every rank's record is all-gathered and merged in rank order, so all ranks end with the same bits."""
        if self.freeze:
            return self
        world = 1
        if dist.is_available() and dist.is_initialized():
            world = dist.get_world_size(group)
        if x.is_cuda:
            if env is None:
                raise ValueError(f"update() of CUDA {self._WHAT} needs env= (the BatchedQuadrotor they belong to)")
            if self._batch is None or self._batch.shape[0] != world:
                self._batch = torch.zeros((world, 1 + 2 * self.N_FEAT), dtype=torch.float64, device=self.buf.device)
            rank = dist.get_rank(group) if world > 1 else 0
            self._moments_gpu(env, C.c_void_p(self._batch[rank].data_ptr()), x, *more)
            if world > 1:
                dist.all_gather_into_tensor(self._batch.view(-1), self._batch[rank].clone(), group=group)
            self._merge_gpu(env, C.c_void_p(self._batch.data_ptr()), world)
            return self
        rec = self._moments_cpu(env, x, *more)
        recs = [rec]
        if world > 1:
            recs = [torch.zeros_like(rec) for _ in range(world)]
            dist.all_gather(recs, rec, group=group)
        for r in recs:
            self._merge_cpu(r)
        return self

    def _merge_cpu(self, rec):
        """the merge kernels' rule, in their order of operations; returns False for an empty record (skipped)"""
        n, F, bc = self._n, self.N_FEAT, float(rec[0])
        if not bc > 0:
            return False
        count = float(self._count[0])
        tot = count + bc
        d = rec[1:1 + n] - self._mean[:n]
        self._mean[:n] += d * bc / tot
        self._m2[:n] = self._m2[:n] + rec[1 + F:1 + F + n] + d * d * count * bc / tot
        self._m2[n:] = tot   # var = 1
        self._count[0] = tot
        self._rstd_f[:n] = (1.0 / torch.sqrt(self._m2[:n] / tot + self._eps)).to(torch.float32)
        return True

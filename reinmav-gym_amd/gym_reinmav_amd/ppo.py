"""PPO2-style rollout collection (and a minimal learner) on top of the batched HIP envs.

This is the *caller* side of the hot path: what ``python -m gym_reinmav.run --alg=ppo2 --env=quadrotor3d-v0
--network=mlp`` does through baselines (``gym_reinmav/run.py:63-68``: ``learn(env=...)`` whose ``Runner``
alternates ``model.step(obs)`` and ``env.step(actions)``, then GAE(lambda) and clipped-surrogate
minibatch epochs).  baselines / TensorFlow 1 are third party and absent; the hyper-parameters below are
baselines' documented ppo2 defaults (nsteps 2048 for ONE env - here the batch is 10^4-10^6 envs, so a
rollout is ``nsteps`` x N transitions with a small ``nsteps``).

MI355X-first choices:
* everything stays on the GPU: observations never leave HBM, ``env.step`` receives the action tensor's
  device pointer and writes obs / reward / done straight into the rollout buffers (zero copies);
* **feature-major layout end to end**: the env's native layout is SoA ``[dim, N]``; the policy computes
  ``W @ X`` on ``X = obs[nS, N]`` and emits actions ``[nA, N]``, so neither side ever transposes and
  every env access stays coalesced (no AoS emit needed);
* the whole T-step rollout (policy + env launches) can be captured in ONE hipGraph
  (``RolloutCollector(graph=True)``): ``rmav_step`` with device pointers allocates nothing and never
  synchronises, so it is capturable; replay removes ~10 eager launches of host overhead per env-step;
* data parallel over GPUs = env sharding; gradients are averaged with one flat all-reduce per minibatch
  (~10 k parameters: latency-bound on xGMI, so a single bucket).
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch
import torch.distributed as dist

from .core import BatchedQuadrotor, policy_action_rule


class _LinearFM(torch.autograd.Function):
    """``W @ x + b[:, None]`` on feature-major activations ``x [in, B]`` with a weight gradient that suits the learner's
    shapes.  ``dW = dy @ x^T`` is a 64 x 64 result reduced over B = 524 288 samples: the BLAS library's pick for that
    long-K product ran 355 us per call - 45 % of a PPO iteration at 65 536 envs x 32 steps.  Cut into chunks of
    ``CHUNK`` columns it is a batched 64 x 64 x CHUNK product over hundreds of workgroups plus a small sum."""

    CHUNK = 8192
    _ones = None   # one vector of ones, grown to the largest batch seen (sliced for smaller ones)

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        return torch.addmm(bias[:, None], weight, x)

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gx = weight.t() @ gy if ctx.needs_input_grad[0] else None
        B, C = x.shape[1], _LinearFM.CHUNK
        if B % C == 0 and B > C:
            nb = B // C
            # autograd may hand over a non-contiguous gy (expanded / transposed grads), callers a permuted x
            gy_c, x_c = gy.contiguous(), x.contiguous()
            gw = torch.bmm(gy_c.view(gy.shape[0], nb, C).transpose(0, 1),          # [nb, out, C]
                           x_c.view(x.shape[0], nb, C).permute(1, 2, 0)).sum(0)     # [nb, C, in] -> [out, in]
        else:
            gw = gy @ x.t()
        # bias gradient as a matrix-vector product with ones (the generic row reduction ran at 2.7 TB/s)
        ones = _LinearFM._ones
        if ones is None or ones.numel() < B or ones.device != gy.device or ones.dtype != gy.dtype:
            ones = _LinearFM._ones = torch.ones(B, dtype=gy.dtype, device=gy.device)
        return gx, gw, torch.mv(gy, ones[:B])


class MlpPolicy(torch.nn.Module):
    """baselines ``mlp`` (2 x 64 tanh) Gaussian policy, in feature-major form.

    ``value_network``: ``'copy'`` (default) = a separate value net of the same shape - baselines' MuJoCo default and its classic
    ``MlpPolicy``; ``'shared'`` = a scalar value head on the policy's latent - what baselines' ``build_policy`` does when
    ``value_network`` is None, i.e. for an env type without a ppo2 defaults entry such as the native envs of gym_reinmav
    (``run.py:63-68``; third-party behaviour restated from memory).  ``self.vf`` is then the one-layer head.  Both architectures have
    an in-kernel actor (``FusedPolicyCollector``) and, with ``hidden=64``, a fused learner (``PPO(fused_learner=True)``).

    ``obs_norm`` (a :class:`~gym_reinmav_amd.obs_norm.RunningObsNorm`): ``forward`` first normalises its input,
    ``clamp((obs - mean_f) * rstd_f, -clip, clip)`` in fp32 from the statistics buffer's tables - the numbers the in-kernel actors of
    ``rmav_rollout_policy_norm`` feed their first layer, bit for bit.  No gradient flows into the statistics; the collectors and
    ``PPO.update`` keep storing and passing RAW observations."""

    def __init__(self, n_obs: int, n_act: int, hidden: int = 64, init_logstd: float = 0.0, value_network: str = "copy", obs_norm=None):
        super().__init__()
        assert value_network in ("copy", "shared")
        if obs_norm is not None and obs_norm.n_obs != n_obs:
            raise ValueError("obs_norm was made for another observation size")
        self.obs_norm = obs_norm
        self.shared = value_network == "shared"
        mk = lambda i, o: torch.nn.Linear(i, o)  # noqa: E731
        self.pi = torch.nn.ModuleList([mk(n_obs, hidden), mk(hidden, hidden), mk(hidden, n_act)])
        self.vf = torch.nn.ModuleList([mk(hidden, 1)] if self.shared else [mk(n_obs, hidden), mk(hidden, hidden), mk(hidden, 1)])
        self.logstd = torch.nn.Parameter(torch.full((n_act,), float(init_logstd)))
        for net, last_gain in ((self.pi, 0.01), (self.vf, 1.0)):
            for i, lin in enumerate(net):
                torch.nn.init.orthogonal_(lin.weight, gain=last_gain if lin is net[-1] else math.sqrt(2.0))
                torch.nn.init.zeros_(lin.bias)

    @staticmethod
    def _mlp(net, x):  # x [in, N] -> [out, N]
        for i, lin in enumerate(net):
            x = (_LinearFM.apply(x, lin.weight, lin.bias) if torch.is_grad_enabled() and x.is_cuda
                 else torch.addmm(lin.bias[:, None], lin.weight, x))
            if i < 2:
                x = torch.tanh(x)
        return x

    def _lin(self, lin, x):
        return (_LinearFM.apply(x, lin.weight, lin.bias) if torch.is_grad_enabled() and x.is_cuda
                else torch.addmm(lin.bias[:, None], lin.weight, x))

    def forward(self, obs_fm: torch.Tensor):
        """obs_fm [nS, N] -> (mean [nA, N], value [N])."""
        if self.obs_norm is not None:
            obs_fm = self.obs_norm.normalize(obs_fm)
        if self.shared:
            h = torch.tanh(self._lin(self.pi[1], torch.tanh(self._lin(self.pi[0], obs_fm))))
            return self._lin(self.pi[2], h), self._lin(self.vf[0], h)[0]
        return self._mlp(self.pi, obs_fm), self._mlp(self.vf, obs_fm)[0]

    def log_prob(self, mean, act):
        z = (act - mean) * torch.exp(-self.logstd)[:, None]
        return -0.5 * (z * z).sum(0) - self.logstd.sum() - 0.5 * mean.shape[0] * math.log(2 * math.pi)

    def entropy(self):
        return (self.logstd + 0.5 * math.log(2 * math.pi * math.e)).sum()


class RolloutCollector:
    """Collects ``nsteps`` transitions of every env into device-resident, time-major, feature-major buffers."""

    def __init__(self, env: BatchedQuadrotor, policy: MlpPolicy, nsteps: int, graph: bool = False, bootstrap_truncated: bool = False,
                 deterministic: bool = False, clip_actions=False):
        """``deterministic=True``: the mean action, no noise (``logp`` = the log-density of the mean).  ``clip_actions``: ``True`` = the
        env steps with ``clamp(act, params.act_lo, params.act_hi)``, ``(lo, hi)`` = explicit bounds; ``act`` and ``logp`` stay those of
        the unclipped action, as in stable-baselines' PPO2 runner.  The semantics of :class:`FusedPolicyCollector`'s arguments of the
        same names (``rmav_set_policy_action_rule``); ``graph=True`` still captures.

        ``bootstrap_truncated=True`` (needs ``env.max_episode_steps``): the collector also owns ``boot [T, N]`` - the value net on
        the state a truncated episode ended in (``rmav_step_final``'s ``final_obs``, which the auto-reset has replaced in ``obs``), 0
        where the step was not truncated - and ``trunc [T, N]``; ``PPO.update`` then targets ``r + gamma V(s_final)`` on those steps.
        One more policy forward per step, no host synchronisation: ``graph=True`` still captures (the env's ``step_count`` then stays
        where it was at the capture: the replayed launches carry their episode clock with them, see ``_capture``)."""
        assert env.auto_reset, "rollouts need VecEnv semantics (auto-reset)"
        if graph and getattr(env, "sensor_noise", None) is not None:
            # (a captured launch keeps the step counter it was captured with - include/rmav.h - and the sensor noise is a function of it:
            # every replay would draw the same noise per env and step of the rollout)
            raise ValueError("graph=True on an env with sensor_noise= would replay one noise pattern: every captured launch keeps its step "
                             "counter; collect without a graph")
        self.env, self.policy, self.T = env, policy, int(nsteps)
        det, lo, hi = policy_action_rule(deterministic, clip_actions, lambda: (env.params.act_lo, env.params.act_hi))
        self.deterministic = bool(det)
        self.clip = None if (lo, hi) == (-math.inf, math.inf) else (lo, hi)
        self.boot = self.trunc = None
        if bootstrap_truncated:
            if not env.max_episode_steps:
                raise ValueError("bootstrap_truncated=True needs an env with max_episode_steps")
            dev_ = torch.device("cuda", env.device)
            self.boot = torch.zeros((self.T, env.num_envs), dtype=torch.float32, device=dev_)
            self.trunc = torch.zeros((self.T, env.num_envs), dtype=torch.uint8, device=dev_)
            self._final = torch.zeros((env.nS, env.num_envs), dtype=torch.float32, device=dev_)   # rows of unfinished envs: stale, masked
        dev = torch.device("cuda", env.device)
        N, nS, nA, T = env.num_envs, env.nS, env.nA, self.T
        f32 = dict(dtype=torch.float32, device=dev)
        self.obs = torch.empty((T + 1, nS, N), **f32)   # obs[t] is the observation action t was computed from
        self.act = torch.empty((T, nA, N), **f32)
        self.logp = torch.empty((T, N), **f32)
        self.val = torch.empty((T + 1, N), **f32)
        self.rew = torch.empty((T, N), **f32)
        self.done = torch.empty((T, N), dtype=torch.uint8, device=dev)
        self._act_env = torch.empty((nA, N), **f32) if self.clip is not None else None   # what the env is stepped with
        self.obs[0].copy_(env.observe(layout="soa", device_out=True))   # (get_state's bits on an env without sensor noise)
        self._graph = None
        if graph:
            self._capture()

    # one env-step of the loop baselines' Runner.run() executes (model.step -> env.step)
    def _step(self, t: int):
        mean, v = self.policy(self.obs[t])
        if self.deterministic:   # noise x 0: the mean, and the log-density of the mean
            self.act[t].copy_(mean)
            self.logp[t] = -self.policy.logstd.sum() - 0.5 * mean.shape[0] * math.log(2 * math.pi)
        else:
            noise = torch.randn_like(mean)
            torch.addcmul(mean, noise, torch.exp(self.policy.logstd)[:, None], out=self.act[t])
            self.logp[t] = -0.5 * (noise * noise).sum(0) - self.policy.logstd.sum() - 0.5 * mean.shape[0] * math.log(2 * math.pi)
        self.val[t] = v
        act = self.act[t]   # stored (and learned from) unclipped; the env takes the clipped one
        if self.clip is not None:
            act = torch.clamp(act, self.clip[0], self.clip[1], out=self._act_env)
        if self.boot is None:
            self.env.step(act, layout="soa", out=(self.obs[t + 1], self.rew[t], self.done[t]))
        else:
            self.env.step_final(act, layout="soa", out=(self.obs[t + 1], self.rew[t], self.done[t], self._final, self.trunc[t]))
            torch.where(self.trunc[t] != 0, self.policy(self._final)[1], self.boot.new_zeros(()), out=self.boot[t])

    def _body(self):
        with torch.no_grad():
            for t in range(self.T):
                self._step(t)
            self.val[self.T] = self.policy(self.obs[self.T])[1]

    def _capture(self):
        env = self.env
        side = torch.cuda.Stream(device=env.device)
        side.wait_stream(torch.cuda.current_stream(env.device))
        state = env.observe(layout="soa", device_out=True)   # the observation the first action is computed from
        t0 = env.step_count
        with torch.cuda.stream(side):
            # warm-up (allocator, lazy inits of the torch ops) on a scratch env of the same shape, so that the
            # caller's envs - state, steps_beyond_done, reset counters, episode accumulators and totals, clocks -
            # are not advanced by it; the capture below records launches on the real env without executing them
            tmp = BatchedQuadrotor(env.kind, env.num_envs, device=env.device, seed=0, auto_reset=True,
                                   track_episodes=env.track_episodes, params=env.params, actuator=getattr(env, "actuator", None),
                                   start_state=getattr(env, "start_state", None), termination=getattr(env, "termination", None))
            self.env = tmp
            try:
                self._body()
            finally:
                self.env = env
            side.synchronize()
            tmp.close()
            env.use_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                self._body()
                if self.boot is not None:
                    # The episode clock is an argument of every captured launch, so a replay runs steps t0 .. t0 + T - 1 again
                    # whatever the host counter says.  The time limit compares that clock with the envs' episode starts: the
                    # graph ends by moving the starts back by T (rmav_set_step_count inside the capture: one small launch), so
                    # that the running lengths carry over from one replay to the next; collect() then leaves the counter alone.
                    env.step_count = t0
        self._graph = g
        cur = torch.cuda.current_stream(env.device)
        cur.wait_stream(side)
        env.use_stream(cur)                                     # replays run on the caller's current stream
        env.step_count = t0                                     # host-side counter advanced while capturing
        self.obs[0].copy_(state)

    def collect(self):
        """Run one rollout; buffers are valid after the current stream's work completes."""
        if self._graph is not None:
            self._graph.replay()
            if self.boot is None:
                self.env.step_count = self.env.step_count + self.T   # the captured launches carry no host-side effects
        else:
            self._body()
        return self

    def roll_over(self):
        """Make the last observation the first one of the next rollout."""
        self.obs[0].copy_(self.obs[self.T])


def _rowmap(s: int, h: int, j: int) -> int:
    """Row of the previous layer's output that MFMA B-slot (h, j) of K-slice s carries (csrc/rmav_policy_mfma.hpp)."""
    r = 8 * (s & 1) + j
    return 32 * (s >> 1) + (r & 3) + 8 * (r >> 2) + 4 * h


# The in-kernel actors: name -> (rmav_policy_precision constant of _abi, the library's weight count, has *_tl / *_boot / *_nrm / *_dr
# kernels).  FusedPolicyCollector resolves its keyword arguments and the policy's architecture to one of these names, once.
_ACTORS = {
    "fp32": ("POLICY_FP32", lambda L, kind: L.rmav_policy_weight_count(kind), False),          # fp32 FMAs on the vector ALU
    "fp32_mfma": ("POLICY_FP32_MFMA", lambda L, kind: L.rmav_policy_weight_count_f32_mfma(), True),
    "bf16": ("POLICY_BF16_MFMA", lambda L, kind: L.rmav_policy_weight_count_bf16(), False),
    "f16": ("POLICY_F16_MFMA", lambda L, kind: L.rmav_policy_weight_count_bf16(), True),
    "f16_shared": ("POLICY_F16_SHARED", lambda L, kind: L.rmav_policy_weight_count_shared(), True),   # one trunk, two heads
}


class _PolicyPacker:
    """Packs an ``MlpPolicy`` into the weight buffer ``rmav_rollout_policy`` reads (layouts in include/rmav.h).

    The layouts are fixed permutations (+ zero padding) of the flattened parameters, so the index map is
    built once (NumPy, host) and every repack is: one ``cat`` of the parameters, one gather, and for the
    bf16 fragments one dtype conversion - a handful of launches, cheap enough to run before every rollout."""

    K_TANH = 2.8853900817779268   # 2 log2(e): the f16 actor's layer-2 fragments carry -2 k W2, layer 3's -2 W3 (include/rmav.h)

    def __init__(self, policy: MlpPolicy, n_obs: int, actor: str):
        """``actor``: a key of ``_ACTORS``."""
        import numpy as np

        H = policy.pi[0].out_features
        assert H == 64 and policy.pi[1].in_features == 64, "the in-kernel policy is the 2 x 64 baselines mlp"
        assert n_obs <= 16
        assert actor in _ACTORS, actor
        assert bool(getattr(policy, "shared", False)) == (actor == "f16_shared"), "the shared-trunk policy runs on RMAV_POLICY_F16_SHARED, and only it"
        # fragments: the MFMA fragment layout of bf16 pairs - or (f16) of f16 pairs with the tanh fold's weight scales
        self.policy, self.shared, self.f16, self.fragments = policy, actor == "f16_shared", actor.startswith("f16"), actor in ("bf16", "f16", "f16_shared")
        if self.shared:
            self._init_shared(policy, n_obs)
            return
        self.params = [policy.pi[0].weight, policy.pi[0].bias, policy.pi[1].weight, policy.pi[1].bias,
                       policy.pi[2].weight, policy.pi[2].bias, policy.vf[0].weight, policy.vf[0].bias,
                       policy.vf[1].weight, policy.vf[1].bias, policy.vf[2].weight, policy.vf[2].bias, policy.logstd]
        offs = np.cumsum([0] + [p.numel() for p in self.params])
        ZERO = int(offs[-1])                       # index of the appended 0.0
        n_act = policy.logstd.numel()

        def W(net, layer, r, c):                   # flat index of weight[r][c] (or ZERO when outside the matrix)
            p = self.params[6 * net + 2 * layer]
            rows, cols = p.shape
            return int(offs[6 * net + 2 * layer]) + r * cols + c if (r < rows and c < cols) else ZERO

        def Bv(net, layer, r):
            p = self.params[6 * net + 2 * layer + 1]
            return int(offs[6 * net + 2 * layer + 1]) + r if r < p.numel() else ZERO

        logstd = [int(offs[12]) + c if c < n_act else ZERO for c in range(4)]
        if actor == "fp32_mfma":   # A operands of v_mfma_f32_32x32x2_f32 (include/rmav.h, csrc/rmav_policy_mfma32.hpp)
            def row(r, h):
                return (r & 3) + 8 * (r >> 2) + 4 * h

            idx = []
            for net in range(2):
                for T in range(2):               # A1[T][sq][lane][j] = W1p[32 T + m][2 (4 sq + j) + h]
                    for sq in range(2):
                        idx += [W(net, 0, 32 * T + (l & 31), 2 * (4 * sq + jj) + (l >> 5)) for l in range(64) for jj in range(4)]
                for To in range(2):              # A2[To][Tin][rq][lane][j] = W2[32 To + m][32 Tin + row(4 rq + j, h)]
                    for Tin in range(2):
                        for rq in range(4):
                            idx += [W(net, 1, 32 * To + (l & 31), 32 * Tin + row(4 * rq + jj, l >> 5)) for l in range(64) for jj in range(4)]
                for h in range(2):               # W3[h][o][16 Tin + r] = W3p[o][32 Tin + row(r, h)]
                    for o in range(4):
                        idx += [W(net, 2, o, 32 * Tin + row(r, h)) for Tin in range(2) for r in range(16)]
                idx += [Bv(net, 0, jj) for jj in range(64)] + [Bv(net, 1, jj) for jj in range(64)] + [Bv(net, 2, k) for k in range(4)]
            idx += logstd
            self.idx_f32 = torch.tensor(idx, dtype=torch.int64, device=policy.logstd.device)
            self.n_out = len(idx)
        elif not self.fragments:
            nsp = (n_obs + 3) // 4 * 4
            idx = []
            for net in range(2):
                idx += [W(net, 0, jj, i) for jj in range(H) for i in range(nsp)]          # W1 [H][NSP]
                idx += [Bv(net, 0, jj) for jj in range(H)]
                idx += [W(net, 1, jj, i) for i in range(H) for jj in range(H)]            # W2T[i][j] = W2[j][i]
                idx += [Bv(net, 1, jj) for jj in range(H)]
                idx += [W(net, 2, k, jj) for jj in range(H) for k in range(4)]            # W3T[j][k] = W3[k][j]
                idx += [Bv(net, 2, k) for k in range(4)]
            idx += logstd
            self.idx_f32 = torch.tensor(idx, dtype=torch.int64, device=policy.logstd.device)
            self.n_out = len(idx)
        else:
            frag, f32 = [], []                     # per net: bf16 fragment indices, fp32 (bias) indices
            for net in range(2):
                fr = []
                for Mt in range(2):                # A1[Mt][lane][j] = W1p[32 Mt + m][8 h + j]
                    fr += [W(net, 0, 32 * Mt + (l & 31), 8 * (l >> 5) + jj) for l in range(64) for jj in range(8)]
                for Mt in range(2):                # A2[Mt][s][lane][j] = W2[32 Mt + m][rowmap(s, h, j)]
                    for s_ in range(4):
                        fr += [W(net, 1, 32 * Mt + (l & 31), _rowmap(s_, l >> 5, jj)) for l in range(64) for jj in range(8)]
                for s_ in range(4):                # A3[s][lane][j] = W3p[m][rowmap(s, h, j)]
                    fr += [W(net, 2, l & 31, _rowmap(s_, l >> 5, jj)) for l in range(64) for jj in range(8)]
                frag.append(fr)
                f32.append([Bv(net, 0, r) for r in range(64)] + [Bv(net, 1, r) for r in range(64)] +
                           [Bv(net, 2, r) for r in range(32)])
            dev = policy.logstd.device
            self.idx_frag = torch.tensor(frag[0] + frag[1], dtype=torch.int64, device=dev)
            self.idx_bias = torch.tensor(f32[0] + f32[1] + logstd, dtype=torch.int64, device=dev)
            self.n_frag = len(frag[0]) // 2        # floats per net of fragments (2 bf16 per float)
            self.n_bias = len(f32[0])
            self.n_out = 2 * (self.n_frag + self.n_bias) + 4
            if self.f16:   # per fragment element: 1 (layer 1), -2k (layer 2), -2 (layer 3)
                per_net = [1.0] * (2 * 64 * 8) + [-2.0 * self.K_TANH] * (8 * 64 * 8) + [-2.0] * (4 * 64 * 8)
                self.frag_scale = torch.tensor(per_net + per_net, dtype=torch.float32, device=dev)

    def _init_shared(self, policy, n_obs):
        """ONE net in the bf16 fragment layout (include/rmav.h, RMAV_POLICY_F16_SHARED): output rows 0..3 of the padded 32-row output
        tile = the mean head, row 4 = the value head; then logstd [4]."""
        import numpy as np

        self.params = [policy.pi[0].weight, policy.pi[0].bias, policy.pi[1].weight, policy.pi[1].bias, policy.pi[2].weight,
                       policy.pi[2].bias, policy.vf[0].weight, policy.vf[0].bias, policy.logstd]
        offs = np.cumsum([0] + [p.numel() for p in self.params])
        ZERO, n_act = int(offs[-1]), policy.logstd.numel()
        assert n_act <= 4

        def W(k, r, c):
            rows, cols = self.params[k].shape
            return int(offs[k]) + r * cols + c if (r < rows and c < cols) else ZERO

        def W3(m, c):      # padded output layer: rows 0 .. nA-1 the mean head, row 4 the value head
            return W(4, m, c) if m < n_act else (W(6, 0, c) if m == 4 else ZERO)

        fr = []
        for Mt in range(2):
            fr += [W(0, 32 * Mt + (l & 31), 8 * (l >> 5) + jj) for l in range(64) for jj in range(8)]
        for Mt in range(2):
            for s_ in range(4):
                fr += [W(2, 32 * Mt + (l & 31), _rowmap(s_, l >> 5, jj)) for l in range(64) for jj in range(8)]
        for s_ in range(4):
            fr += [W3(l & 31, _rowmap(s_, l >> 5, jj)) for l in range(64) for jj in range(8)]
        b3 = [int(offs[5]) + r if r < n_act else (int(offs[7]) if r == 4 else ZERO) for r in range(32)]
        bias = [int(offs[1]) + r for r in range(64)] + [int(offs[3]) + r for r in range(64)] + b3
        logstd = [int(offs[8]) + c if c < n_act else ZERO for c in range(4)]
        dev = policy.logstd.device
        self.idx_frag = torch.tensor(fr, dtype=torch.int64, device=dev)
        self.idx_bias = torch.tensor(bias + logstd, dtype=torch.int64, device=dev)
        self.n_frag, self.n_bias = len(fr) // 2, len(bias)
        self.n_out = self.n_frag + self.n_bias + 4
        per_net = [1.0] * (2 * 64 * 8) + [-2.0 * self.K_TANH] * (8 * 64 * 8) + [-2.0] * (4 * 64 * 8)
        self.frag_scale = torch.tensor(per_net, dtype=torch.float32, device=dev)

    def native_maps(self):
        """(idx_lo, idx_hi) int32 device tensors of ``rmav_pack_policy``: output word i = flat[idx_lo[i]] (idx_hi[i] < 0) or the
        bf16 pair (flat[idx_lo[i]], flat[idx_hi[i]]); built once from the same index lists ``pack`` uses."""
        if getattr(self, "_native", None) is None:
            dev = self.params[0].device
            if self.shared:
                fr, bi = self.idx_frag.to(torch.int32), self.idx_bias.to(torch.int32)
                lo = torch.cat([fr[0::2], bi])
                hi = torch.cat([fr[1::2], torch.full((bi.numel(),), -1, dtype=torch.int32, device=dev)])
            elif not self.fragments:
                lo = self.idx_f32.to(torch.int32)
                hi = torch.full_like(lo, -1)
            else:
                fr, bi, nf, nb = self.idx_frag.to(torch.int32), self.idx_bias.to(torch.int32), self.n_frag, self.n_bias
                neg = lambda k: torch.full((k,), -1, dtype=torch.int32, device=dev)  # noqa: E731
                # pack(): [fragments net 0 | biases net 0 | fragments net 1 | biases net 1 | logstd]; a fragment word = bf16 pair
                lo = torch.cat([fr[0:2 * nf:2], bi[:nb], fr[2 * nf::2], bi[nb:2 * nb], bi[2 * nb:]])
                hi = torch.cat([fr[1:2 * nf:2], neg(nb), fr[2 * nf + 1::2], neg(nb), neg(bi.numel() - 2 * nb)])
            assert lo.numel() == self.n_out == hi.numel()
            self._native = (lo.contiguous(), hi.contiguous())
        return self._native

    def pack_native(self, env, out: torch.Tensor) -> torch.Tensor:
        """The same buffer as ``pack`` in ONE launch on the env's stream (``rmav_pack_policy``)."""
        import ctypes as C

        from . import _abi as A

        lo, hi = self.native_maps()
        ps = [p.detach() for p in self.params]
        assert all(p.is_contiguous() and p.dtype == torch.float32 and p.is_cuda for p in ps), "parameters must be contiguous fp32 CUDA tensors"
        n = len(ps)
        ptrs = (C.c_void_p * n)(*[p.data_ptr() for p in ps])
        sizes = (C.c_int64 * n)(*[p.numel() for p in ps])
        fn = A.lib().rmav_pack_policy_f16 if self.f16 else A.lib().rmav_pack_policy
        A.check(fn(env._h, n, ptrs, sizes, C.c_void_p(lo.data_ptr()), C.c_void_p(hi.data_ptr()), self.n_out, C.c_void_p(out.data_ptr())))
        return out

    def pack(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        with torch.no_grad():
            flat = torch.cat([p.detach().reshape(-1).float() for p in self.params] + [torch.zeros(1, device=self.params[0].device)])
            if self.shared:
                fr = (flat[self.idx_frag] * self.frag_scale).to(torch.float16).view(torch.int16).view(torch.float32)
                res = torch.cat([fr, flat[self.idx_bias]])
            elif not self.fragments:
                res = flat[self.idx_f32]
            else:
                if self.f16:
                    fr = (flat[self.idx_frag] * self.frag_scale).to(torch.float16).view(torch.int16).view(torch.float32)
                else:
                    fr = flat[self.idx_frag].to(torch.bfloat16).view(torch.int16).view(torch.float32)   # [2 * n_frag]
                bi = flat[self.idx_bias]
                res = torch.cat([fr[:self.n_frag], bi[:self.n_bias], fr[self.n_frag:], bi[self.n_bias:2 * self.n_bias],
                                 bi[2 * self.n_bias:]])
            if out is not None:
                out.copy_(res)
                return out
            return res.contiguous()


def pack_policy_weights(policy: MlpPolicy, n_obs: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 layout: per net  W1 [64][NSP] | b1 | W2^T [64][64] | b2 | W3^T [64][4] | b3 [4],  then logstd [4]."""
    return _PolicyPacker(policy, n_obs, "fp32").pack(out)


def pack_policy_weights_f32_mfma(policy: MlpPolicy, n_obs: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 A operands of v_mfma_f32_32x32x2_f32: per net A1 [2][2][64][4] | A2 [2][2][4][64][4] | W3 [2][4][32] |
    b1 [64] | b2 [64] | b3 [4], then logstd [4] (include/rmav.h)."""
    return _PolicyPacker(policy, n_obs, "fp32_mfma").pack(out)


def pack_policy_weights_bf16(policy: MlpPolicy, n_obs: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 MFMA fragments: per net A1 [2][64][8] | A2 [2][4][64][8] | A3 [4][64][8] (bf16) | b1 [64] | b2 [64] |
    b3 [32] (fp32), then logstd [4]."""
    return _PolicyPacker(policy, n_obs, "bf16").pack(out)


def pack_policy_weights_f16(policy: MlpPolicy, n_obs: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """f16 MFMA fragments in the bf16 layout, layers 2 / 3 pre-scaled by -2 * 2 log2(e) / -2 (tanh folded into the next
    layer: the kernel hands (1 - tanh z) / 2 on and derives the matching biases from these rounded weights)."""
    return _PolicyPacker(policy, n_obs, "f16_shared" if getattr(policy, "shared", False) else "f16").pack(out)


class FusedPolicyCollector:
    """Same buffers and semantics as :class:`RolloutCollector`, but ONE kernel launch per rollout: the policy
    (2 x 64 tanh MLP + value net, weights staged in LDS) is evaluated inside the rollout kernel by the lane
    that owns the env (``rmav_rollout_policy``), so nothing but the trajectory touches HBM."""

    def __init__(self, env: BatchedQuadrotor, policy: MlpPolicy, nsteps: int, bf16_mfma: bool = False,
                 f32_mfma: Optional[bool] = None, native_pack: bool = True, f16_mfma: bool = False, bootstrap_truncated: bool = False,
                 deterministic: bool = False, clip_actions=False, store_trajectory: bool = True):
        """``store_trajectory=False``: the launch gets NULL for ``actions_out`` / ``obs_out`` (``act`` and ``obs`` are None) and only
        ``rew``, ``done``, ``logp``, ``val`` (and ``boot`` / ``trunc``) reach HBM - what an evaluation needs (``evaluate.py``); such a
        collector cannot feed ``PPO.update``.

        ``deterministic`` / ``clip_actions`` (``True`` = the env's action space, or ``(lo, hi)``): the action rule of the launch
        (``BatchedQuadrotor.set_policy_action_rule``) - the mean action instead of a sample, and dynamics that take the clipped action
        while ``act`` / ``logp`` stay those of the unclipped one.  ``collect()`` sets the rule on the env before every launch, so a
        training collector and an evaluating one can share an env.  The fp32 matrix-core actor, ``f16_mfma=True`` or a shared-trunk policy.

        Actor arithmetic: fp32 on the fp32-input matrix instructions (``v_mfma_f32_32x32x2_f32``; the default),
        ``f32_mfma=False`` fp32 FMAs on the vector ALU (same precision class - only the summation order differs - at
        half the speed), ``bf16_mfma=True`` bf16 operands on the matrix cores (~1e-2 on means), ``f16_mfma=True`` f16
        operands with tanh folded into the next layer (the fastest, ~1e-3 on means; csrc/rmav_policy_pair.hpp).

        ``bootstrap_truncated=True`` (needs ``env.max_episode_steps``): the launch is ``rmav_rollout_policy_boot`` and the collector
        also owns ``boot [T, N]`` = the launch's value net on the state a truncated episode ended in (0 where the step was not
        truncated) and ``trunc [T, N]``; ``PPO.update`` then targets ``r + gamma V(s_final)`` on those steps.

        A policy with ``obs_norm`` runs ``rmav_rollout_policy_norm``: both nets see the normalised observation, with the statistics
        FROZEN for the launch (``obs_norm.py``); ``obs`` stays raw.  The fp32 matrix-core actor, ``f16_mfma=True`` or a shared-trunk
        policy; on an env with ``max_episode_steps`` the launch always leaves ``boot`` / ``trunc``, so ``bootstrap_truncated`` is
        required there."""
        import ctypes as C

        from . import _abi as A

        assert not (bf16_mfma and f16_mfma) and not (f32_mfma and (bf16_mfma or f16_mfma))
        if getattr(policy, "shared", False):   # one trunk, two heads: RMAV_POLICY_F16_SHARED (the only actor of that architecture)
            assert not bf16_mfma and not f32_mfma, "a shared-trunk policy runs on the f16 actor"
            actor = "f16_shared"
        else:
            actor = "f16" if f16_mfma else "bf16" if bf16_mfma else "fp32" if f32_mfma is not None and not f32_mfma else "fp32_mfma"
        precision, weight_count, has_variants = _ACTORS[actor]

        def refuse(feature, kernel):
            raise ValueError(f"{feature} runs the fp32 matrix-core actor (the default), f16_mfma=True or a shared-trunk policy: "
                             f"the fp32 vector-ALU (f32_mfma=False) and bf16 actors have no {kernel} kernel")

        assert env.auto_reset, "rollouts need VecEnv semantics (auto-reset)"
        limited = bool(getattr(env, "max_episode_steps", None))
        norm = getattr(policy, "obs_norm", None)
        if not has_variants:
            if limited:
                refuse("an env with max_episode_steps", "time-limited")
            if hasattr(env, "get_env_param_range") and any(env.get_env_param_range(nm) for nm in ("mass", "load_mass", "tether_length")):
                refuse("an env with randomize= / set_env_param_range", "ranged")
            if norm is not None:
                refuse("a policy with obs_norm", "normalised")
            if getattr(env, "frame_skip", 1) > 1:
                refuse("an env with frame_skip", "frame-skip")
            if getattr(env, "reward", None) is not None:
                refuse("an env with reward=", "tracking-reward")
            if getattr(env, "disturbance", None) is not None:
                refuse("an env with disturbance=", "disturbed")
        if not has_variants and getattr(env, "sensor_noise", None) is not None:
            refuse("an env with sensor_noise=", "sensor-noise")
        if not has_variants and getattr(env, "actuator", None) is not None:
            refuse("an env with actuator=", "actuator-lag")
        if not has_variants and getattr(env, "start_state", None) is not None:
            refuse("an env with start_state=", "start-state")
        if not has_variants and getattr(env, "termination", None) is not None:
            refuse("an env with termination=", "termination")
        self._rule = policy_action_rule(deterministic, clip_actions, lambda: (env.params.act_lo, env.params.act_hi))
        if not has_variants and self._rule != (0, -math.inf, math.inf):
            refuse("deterministic= / clip_actions=", "action-rule")
        if norm is not None:
            if limited and not bootstrap_truncated:
                raise ValueError("a policy with obs_norm on an env with max_episode_steps needs bootstrap_truncated=True "
                                 "(rmav_rollout_policy_norm always leaves the bootstrap term there)")
            if norm.buf.device != torch.device("cuda", env.device):
                raise ValueError("policy.obs_norm must live on the env's device")
        self.env, self.policy, self.T = env, policy, int(nsteps)
        self.actor = actor
        self.bf16_mfma, self.f32_mfma, self.f16_mfma = actor == "bf16", actor == "fp32_mfma", actor in ("f16", "f16_shared")
        self._C, self._A = C, A
        dev = torch.device("cuda", env.device)
        N, nS, nA, T = env.num_envs, env.nS, env.nA, self.T
        f32 = dict(dtype=torch.float32, device=dev)
        self.obs = torch.empty((T + 1, nS, N), **f32) if store_trajectory else None
        self.act = torch.empty((T, nA, N), **f32) if store_trajectory else None
        self.logp = torch.empty((T, N), **f32)
        self.val = torch.empty((T + 1, N), **f32)
        self.rew = torch.empty((T, N), **f32)
        self.done = torch.empty((T, N), dtype=torch.uint8, device=dev)
        n_w = weight_count(A.lib(), env.kind)
        self.weights = torch.empty(n_w, **f32)
        assert self.weights.data_ptr() % 16 == 0
        self._packer = _PolicyPacker(policy, env.nS, actor)
        assert self._packer.n_out == n_w, (self._packer.n_out, n_w)
        if store_trajectory:
            self.obs[0].copy_(env.observe(layout="soa", device_out=True))   # (get_state's bits on an env without sensor noise)
        # The weight repack before every rollout: one gather launch behind the C ABI (rmav_pack_policy).  As ~8 dependent torch
        # launches (cat, gather, bf16 conversion, cat, copy) it cost ~38 us of a 0.21 ms rollout at 65 536 envs x 32 steps; a
        # hipGraph of those launches replayed no faster (the dependent-launch floor, not the host, is what they cost).
        self.native_pack = bool(native_pack)
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        # (the env's handle is read at call time: env.close() clears it, and a cached copy would hand a freed handle to the library)
        self.boot = self.trunc = None
        if bootstrap_truncated:
            if not getattr(env, "max_episode_steps", None):
                raise ValueError("bootstrap_truncated=True needs an env with max_episode_steps")
            self.boot = torch.empty((T, N), **f32)
            self.trunc = torch.empty((T, N), dtype=torch.uint8, device=dev)
        if norm is not None:
            fn, stats = A.lib().rmav_rollout_policy_norm, (C.c_void_p(norm.data_ptr()),)
            boot = (p(self.boot), p(self.trunc)) if bootstrap_truncated else (None, None)
        elif bootstrap_truncated:
            fn, stats, boot = A.lib().rmav_rollout_policy_boot, (), (p(self.boot), p(self.trunc))
        else:
            fn, stats, boot = A.lib().rmav_rollout_policy, (), ()
        traj = (p(self.act), p(self.obs[1:])) if store_trajectory else (None, None)
        outs = traj + (p(self.rew), p(self.done), p(self.logp), p(self.val))
        self._call = (fn, self.T, p(self.weights)) + stats + outs + boot + (getattr(A, precision),)

    def _pack(self):
        if self.native_pack:
            self._packer.pack_native(self.env, self.weights)
        else:
            self._packer.pack(out=self.weights)

    def collect(self, nsteps: Optional[int] = None):
        """One launch of ``nsteps`` steps (default, and at most, the collector's ``nsteps``: a shorter launch fills the first rows of
        the buffers and leaves its bootstrap value in ``val[nsteps]``)."""
        if self.env._h is None:
            raise self._A.RmavError(self._A.ERR_INVALID, "the env of this collector is closed")
        T = self.T if nsteps is None else int(nsteps)
        if not 0 < T <= self.T:
            raise ValueError(f"nsteps must be in [1, {self.T}]")
        self._pack()
        fn = self._call[0]
        self._A.check(self._A.lib().rmav_set_policy_action_rule(self.env._h, *self._rule))   # host only: this collector's rule, not the last one's
        self._A.check(fn(self.env._h, T, *self._call[2:]))
        return self

    def roll_over(self):
        if self.obs is not None:
            self.obs[0].copy_(self.obs[self.T])


def gae(rew, val, done, gamma: float = 0.99, lam: float = 0.95, boot=None):
    """Generalised advantage estimation on time-major tensors - the plain torch fp32 form (T small launches per
    call), kept as the reference the HIP kernel (``BatchedQuadrotor.gae`` -> ``rmav_gae``) is tested against and
    for CPU tensors; ``PPO.update`` uses the kernel.

    rew [T,N], val [T+1,N] (val[T] = bootstrap value), done [T,N] (1 = the episode ended with step t; the
    next obs is a fresh reset and must not be bootstrapped from).  Returns (adv [T,N], returns [T,N]).

    ``boot`` [T,N] (optional): V(s_final) where step t was truncated by the episode time limit, 0 elsewhere:
    delta_t = r_t + gamma ((1 - done_t) V_{t+1} + boot_t) - V_t, so a truncated step's target is r + gamma V(s_final) instead of r
    alone; the recursion still stops at every done.  ``None`` is the function without the term."""
    T = rew.shape[0]
    adv = torch.empty_like(rew)
    last = torch.zeros_like(rew[0])
    nonterm = 1.0 - done.to(rew.dtype)
    for t in range(T - 1, -1, -1):
        delta = rew[t] + gamma * val[t + 1] * nonterm[t] - val[t]
        if boot is not None:
            delta = delta + gamma * boot[t]
        last = delta + gamma * lam * nonterm[t] * last
        adv[t] = last
    return adv, adv + val[:T]


class _FusedOptState(NamedTuple):
    """What PPO(fused_optimizer=True) keeps on the device: Adam's two moments as flat buffers in the fused learner's order, their
    per-parameter views (installed as the torch optimiser's ``exp_avg`` / ``exp_avg_sq``), and the outputs of the two launches."""
    exp_avg: torch.Tensor
    exp_avg_sq: torch.Tensor
    exp_avg_views: list
    exp_avg_sq_views: list
    adv_norm: torch.Tensor   # rmav_adv_moments -> (mean, 1 / (std + 1e-8))
    stats: torch.Tensor      # rmav_ppo_adam -> (norm, coef)


class PPO:
    """Clipped-surrogate PPO (baselines ppo2 defaults: lr 3e-4, clip 0.2, 4 epochs x 4 minibatches,
    vf_coef 0.5, ent_coef 0, max_grad_norm 0.5, gamma 0.99, lambda 0.95)."""

    def __init__(self, policy: MlpPolicy, lr: float = 3e-4, clip: float = 0.2, epochs: int = 4, minibatches: int = 4,
                 vf_coef: float = 0.5, ent_coef: float = 0.0, max_grad_norm: float = 0.5, gamma: float = 0.99,
                 lam: float = 0.95, reward_scale: float = 1.0, ret_norm=None, fused_learner: bool = False, fused_optimizer: bool = False,
                 matrix_learner: bool = False):
        """``fused_learner=True``: every minibatch's loss and gradients come from the fused learner instead of torch autograd
        (``value_network="copy"``: ``rmav_ppo_grad``, one launch per net plus a fold, csrc/rmav_learner.hpp; ``"shared"``:
        ``rmav_ppo_grad_shared``, one launch for the trunk and both heads plus the fold, csrc/rmav_learner_shared.hpp); the
        all-reduce, the norm clip and Adam run unchanged on the ``p.grad`` it leaves.  An ``MlpPolicy(hidden=64)`` of either
        architecture with CUDA parameters and a collector that has an env handle; anything else is a ``ValueError``.  The default keeps
        the torch path, bit for bit.

        ``fused_optimizer=True`` (needs ``fused_learner=True``; anything else is a ``ValueError``): the rest of a minibatch runs in HIP
        too (csrc/rmav_optim.hpp).  The advantage moments come from ``rmav_adv_moments`` instead of a gather and two torch reductions;
        a data-parallel run all-reduces the flat gradient buffer itself (one ``dist.all_reduce``); and ``clip_grad_norm_`` +
        ``opt.step()`` become ONE launch, ``rmav_ppo_adam``.  The kernel's state IS ``self.opt``'s: ``exp_avg`` / ``exp_avg_sq`` of
        every parameter are views of two flat buffers (existing state is copied in first), ``step`` advances on the host, and
        ``lr`` / ``betas`` / ``eps`` are read from ``self.opt.param_groups[0]`` at every step - ``state_dict()`` /
        ``load_state_dict()``, learning-rate schedules and switching paths between updates keep working.  ``p.grad`` (views of the
        flat buffer) holds the UNCLIPPED gradient on this path - on a data-parallel run the ranks' sum - and ``update`` also returns
        ``grad_norm``, the pre-clip norm of the last minibatch.  The default keeps today's path, bit for bit.

        ``matrix_learner=True`` (needs ``fused_learner=True`` and an ``MlpPolicy(value_network="shared", hidden=64)``; anything else is
        a ``ValueError``): the minibatch's loss and gradients come from ``rmav_ppo_grad_shared_mfma`` (csrc/rmav_learner_mfma.hpp), the
        shared-trunk learner with every product on the fp32 matrix cores - the same precision class, another order of summation.  It
        works with ``fused_optimizer`` on or off.  The default keeps today's path, bit for bit.

        ``ret_norm`` (a :class:`~gym_reinmav_amd.ret_norm.RunningReturnNorm`): baselines' ``VecNormalize(ret=True)`` in front of
        GAE - ``update`` first merges the rollout's discounted returns into it, then computes the advantages from rewards scaled by
        the statistics that already include them (``ret_norm.py``); ``ro.rew`` stays raw.  ``self.adv`` / ``self.ret`` keep the
        ``[T, N]`` advantages / returns of the last ``update``."""
        self.policy = policy
        self.ret_norm = ret_norm
        self.adv = self.ret = None
        self.reward_scale = float(reward_scale)   # baselines' --reward_scale (gym_reinmav/run.py:76)
        self.opt = torch.optim.Adam(policy.parameters(), lr=lr, eps=1e-5)
        self.clip, self.epochs, self.minibatches = clip, epochs, minibatches
        self.vf_coef, self.ent_coef, self.max_grad_norm, self.gamma, self.lam = vf_coef, ent_coef, max_grad_norm, gamma, lam
        self.fused_learner = bool(fused_learner)
        self.fused_optimizer = bool(fused_optimizer)
        if self.fused_optimizer and not self.fused_learner:
            raise ValueError("fused_optimizer=True needs fused_learner=True: rmav_ppo_adam steps on the flat gradient the fused learner leaves")
        self.matrix_learner = bool(matrix_learner)
        if self.matrix_learner and not self.fused_learner:
            raise ValueError("matrix_learner=True needs fused_learner=True: it selects the fused learner's kernel (rmav_ppo_grad_shared_mfma)")
        if self.matrix_learner and not getattr(policy, "shared", False):
            raise ValueError('matrix_learner=True computes an MlpPolicy(value_network="shared", hidden=64): this policy is not a shared-trunk one')
        self._fused_opt = None   # a _FusedOptState: built by the first fused step
        self._fused = None   # (the 13 or 9 parameters in the ABI order, the flat gradient, its views): built by the first fused update
        if self.fused_learner:
            self._fused_params()

    # the ABI order of rmav_ppo_grad's parameters and of its flat gradient, by NAME (parameters() order is logstd first)
    _FUSED_NAMES = tuple(f"{net}.{k}.{w}" for net in ("pi", "vf") for k in range(3) for w in ("weight", "bias")) + ("logstd",)
    # ... and of rmav_ppo_grad_shared's: the trunk and the mean head, the value head, logstd
    _FUSED_NAMES_SHARED = tuple(f"pi.{k}.{w}" for k in range(3) for w in ("weight", "bias")) + ("vf.0.weight", "vf.0.bias", "logstd")

    def _fused_params(self):
        """The policy's parameters in the fused learner's order (that of its architecture); ValueError for a policy it does not compute."""
        pol = self.policy
        shared = bool(getattr(pol, "shared", False))
        names = self._FUSED_NAMES_SHARED if shared else self._FUSED_NAMES
        named = dict(pol.named_parameters())
        if sorted(named) != sorted(names):
            raise ValueError(f"fused_learner=True needs an MlpPolicy's parameters {names}, got {tuple(sorted(named))}")
        hidden = pol.pi[0].out_features
        if hidden != 64 or any(net[1].weight.shape != (64, 64) for net in ((pol.pi,) if shared else (pol.pi, pol.vf))):
            raise ValueError(f"fused_learner=True computes hidden=64 (the 2 x 64 baselines mlp), this policy has hidden={hidden}")
        ps = [named[n] for n in names]
        if not all(p.is_cuda for p in ps):
            what = 'this value_network="shared" policy\'s' if shared else "the policy's"
            raise ValueError(f"fused_learner=True runs on the GPU: {what} parameters are CPU tensors (move the policy to the env's device first)")
        if not all(p.dtype == torch.float32 and p.is_contiguous() for p in ps):
            raise ValueError("fused_learner=True needs contiguous fp32 parameters")
        return ps

    def _fused_step(self, env, obs, act, logp_old, val_old, adv, ret, idx):
        """One minibatch through rmav_ppo_grad (a shared-trunk policy: rmav_ppo_grad_shared): leaves every ``p.grad`` (views of one flat
        buffer) and returns the device ``stats``."""
        if self._fused is None:
            ps = self._fused_params()
            flat = torch.empty(sum(p.numel() for p in ps), dtype=torch.float32, device=ps[0].device)
            views, o = [], 0
            for p in ps:
                views.append(flat[o:o + p.numel()].view_as(p))
                o += p.numel()
            self._fused = (ps, flat, views, torch.empty(4, dtype=torch.float32, device=flat.device))
            if self.fused_optimizer:   # once: this path never rewrites p.grad
                for p, g in zip(ps, views):
                    p.grad = g
        ps, flat, views, stats = self._fused
        if self.fused_optimizer:   # (a data-parallel run keeps its per-rank moments on either path)
            adv_norm = env.adv_moments(adv, idx, out=self._fused_buffers().adv_norm)
        else:
            std, mean = torch.std_mean(adv[idx])   # the two reductions the launch does not do
            adv_norm = torch.stack((mean, 1.0 / (std + 1e-8)))
        grad_fn = env.ppo_grad_shared if getattr(self.policy, "shared", False) else env.ppo_grad
        if self.matrix_learner:
            grad_fn = env.ppo_grad_shared_mfma
        grad_fn(ps, obs, act, logp_old, val_old, adv, ret, adv_norm, clip=self.clip, vf_coef=self.vf_coef, ent_coef=self.ent_coef,
                idx=idx, obs_norm=getattr(self.policy, "obs_norm", None), out=(flat, stats))
        if not self.fused_optimizer:
            for p, g in zip(ps, views):
                p.grad = g
        return stats

    def _fused_buffers(self):
        """The fused optimiser's device buffers (a ``_FusedOptState``), allocated once; touches no optimiser state."""
        if self._fused_opt is None:
            ps = self._fused[0]
            dev = ps[0].device
            m, v = (torch.zeros(self._fused[1].numel(), dtype=torch.float32, device=dev) for _ in range(2))
            mv, vv, o = [], [], 0
            for p in ps:
                mv.append(m[o:o + p.numel()].view_as(p))
                vv.append(v[o:o + p.numel()].view_as(p))
                o += p.numel()
            self._fused_opt = _FusedOptState(m, v, mv, vv, torch.empty(2, dtype=torch.float32, device=dev),
                                             torch.empty(2, dtype=torch.float32, device=dev))
        return self._fused_opt

    def _fused_state(self):
        """Adam's moments as two flat buffers in the fused learner's order, their per-parameter views installed as ``self.opt``'s
        ``exp_avg`` / ``exp_avg_sq`` (whatever state the optimiser holds - its own steps', a loaded ``state_dict``'s - is copied in
        first).  Checked once per step by identity, so a ``load_state_dict`` between updates is picked up."""
        ps, buf = self._fused[0], self._fused_buffers()
        for p, pm, pv in zip(ps, buf.exp_avg_views, buf.exp_avg_sq_views):
            st = self.opt.state[p]
            if st.get("exp_avg") is pm and st.get("exp_avg_sq") is pv:
                continue
            with torch.no_grad():
                if "exp_avg" in st:
                    pm.copy_(st["exp_avg"])
                    pv.copy_(st["exp_avg_sq"])
                else:
                    pm.zero_()
                    pv.zero_()
            if "step" not in st:
                st["step"] = torch.tensor(0.0)   # as torch.optim.Adam initialises it: a host scalar
            st["exp_avg"], st["exp_avg_sq"] = pm, pv
        return buf

    def _fused_opt_step(self, env):
        """all-reduce (data-parallel), norm clip and Adam of one minibatch: one ``rmav_ppo_adam`` on the flat gradient -> its device
        ``(norm, coef)``."""
        ps, flat = self._fused[0], self._fused[1]
        buf = self._fused_state()
        group = self.opt.param_groups[0]
        if len(self.opt.param_groups) != 1 or group.get("amsgrad") or group.get("weight_decay") or group.get("maximize"):
            raise ValueError("fused_optimizer=True computes torch.optim.Adam with one parameter group and without amsgrad, weight decay or maximize")
        scale = 1.0
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(flat, op=dist.ReduceOp.SUM)   # the flat buffer itself: no cat, no copy back
            scale = 1.0 / dist.get_world_size()
        state = self.opt.state
        step = int(state[ps[0]]["step"]) + 1
        for p in ps:
            state[p]["step"] += 1
        env.ppo_adam(ps, flat, buf.exp_avg, buf.exp_avg_sq, step, lr=group["lr"], beta1=group["betas"][0], beta2=group["betas"][1], eps=group["eps"],
                     max_grad_norm=self.max_grad_norm if self.max_grad_norm is not None else math.inf, grad_scale=scale,
                     shared=bool(getattr(self.policy, "shared", False)), stats=buf.stats)
        return buf.stats

    def _allreduce_grads(self):
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return
        params = [p for p in self.policy.parameters() if p.grad is not None]
        flat = torch.cat([p.grad.reshape(-1) for p in params])
        dist.all_reduce(flat, op=dist.ReduceOp.SUM)
        flat /= dist.get_world_size()
        o = 0
        for p in params:
            n = p.grad.numel()
            p.grad.copy_(flat[o:o + n].view_as(p.grad))
            o += n

    def loss(self, obs, act, logp_old, val_old, adv, ret):
        """Clipped-surrogate loss of one minibatch (feature-major obs [nS, B], act [nA, B]; the rest [B]);
        the advantages are normalised over the minibatch as in baselines' ppo2.  -> (loss, pg, vf, ratio)."""
        a = (adv - adv.mean()) / (adv.std() + 1e-8)
        mean, v = self.policy(obs)
        logp = self.policy.log_prob(mean, act)
        ratio = torch.exp(logp - logp_old)
        pg = torch.max(-a * ratio, -a * torch.clamp(ratio, 1 - self.clip, 1 + self.clip)).mean()
        v_clip = val_old + torch.clamp(v - val_old, -self.clip, self.clip)
        vf = 0.5 * torch.max((v - ret) ** 2, (v_clip - ret) ** 2).mean()
        return pg + self.vf_coef * vf - self.ent_coef * self.policy.entropy(), pg, vf, ratio

    def update(self, ro: RolloutCollector) -> dict:
        T, N = ro.rew.shape
        rn = self.ret_norm
        if rn is not None:   # return statistics first: rollout k's rewards are scaled with statistics that include rollout k (ret_norm.py)
            rn.update(ro.rew, ro.done, env=getattr(ro, "env", None), reward_scale=self.reward_scale)
        if ro.rew.is_cuda:   # one HIP launch over the [T][N] trajectory (per-lane reverse scan, csrc/rmav_gae.hpp)
            adv, ret = ro.env.gae(ro.rew, ro.done, ro.val, self.gamma, self.lam, self.reward_scale, boot=getattr(ro, "boot", None), ret_norm=rn)
        else:
            if rn is not None:
                rew = rn.normalize(ro.rew, self.reward_scale)
            else:
                rew = ro.rew if self.reward_scale == 1.0 else ro.rew * self.reward_scale
            adv, ret = gae(rew, ro.val, ro.done, self.gamma, self.lam, boot=getattr(ro, "boot", None))
        self.adv, self.ret = adv, ret
        obs = ro.obs[:T].permute(1, 0, 2).reshape(ro.obs.shape[1], T * N)   # [nS, T*N] feature-major
        act = ro.act.permute(1, 0, 2).reshape(ro.act.shape[1], T * N)
        logp_old, val_old = ro.logp.reshape(-1), ro.val[:T].reshape(-1)
        adv, ret = adv.reshape(-1), ret.reshape(-1)
        stats = {}
        B = T * N
        mb = B // self.minibatches
        fused_env = None
        if self.fused_learner:
            fused_env = getattr(ro, "env", None)
            if fused_env is None or getattr(fused_env, "_h", None) is None:
                raise ValueError("fused_learner=True needs a collector with an env handle (ro.env: an open BatchedQuadrotor); this one has none")
            if not ro.rew.is_cuda:
                raise ValueError("fused_learner=True runs on the GPU: the collector's buffers are CPU tensors")
            logp_old, val_old = logp_old.contiguous(), val_old.contiguous()
        for _ in range(self.epochs):
            perm = torch.randperm(B, device=obs.device)
            for i in range(self.minibatches):
                idx = perm[i * mb:(i + 1) * mb]
                if fused_env is not None:   # loss, gradients and statistics of the minibatch from rmav_ppo_grad; nothing is gathered but adv
                    st = self._fused_step(fused_env, obs, act, logp_old, val_old, adv, ret, idx)
                    if self.fused_optimizer:
                        ost = self._fused_opt_step(fused_env)
                        stats = {"pg_loss": st[1], "vf_loss": st[2], "ratio_max": st[3], "grad_norm": ost[0]}
                        continue
                    self._allreduce_grads()
                    torch.nn.utils.clip_grad_norm_(self.policy.parameters(), self.max_grad_norm)
                    self.opt.step()
                    stats = {"pg_loss": st[1], "vf_loss": st[2], "ratio_max": st[3]}
                    continue
                loss, pg, vf, ratio = self.loss(obs[:, idx], act[:, idx], logp_old[idx], val_old[idx], adv[idx], ret[idx])
                self.opt.zero_grad(set_to_none=True)
                loss.backward()
                self._allreduce_grads()
                torch.nn.utils.clip_grad_norm_(self.policy.parameters(), self.max_grad_norm)
                self.opt.step()
                stats = {"pg_loss": pg.detach(), "vf_loss": vf.detach(), "ratio_max": ratio.detach().max()}
        # observation statistics: frozen while the rollout was collected and learned from, now they absorb its T x N observations
        # (every rank, same order; obs_norm.py explains the difference from baselines)
        norm = getattr(self.policy, "obs_norm", None)
        if norm is not None:
            norm.update(ro.obs[:T], layout="soa", env=ro.env)
        var_y = ret.var()
        stats["explained_variance"] = 1.0 - (ret - val_old).var() / (var_y + 1e-8)
        return {k: float(v) for k, v in stats.items()}


def sync_parameters(policy: MlpPolicy, src: int = 0):
    """Broadcast rank ``src``'s parameters (data-parallel start)."""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        for p in policy.parameters():
            dist.broadcast(p.data, src)

#!/usr/bin/env python3
"""Do two builds of librmav.so launch the same kernels and write the same bits?  (profiles/r10/launch_dispatch.md)

    rocprofv3 --kernel-trace --output-format csv -d TRACE_A -- python tools/launch_trace_ab.py run OUT_A     # RMAV_LIB_PATH = build A
    rocprofv3 --kernel-trace --output-format csv -d TRACE_B -- python tools/launch_trace_ab.py run OUT_B     # ... build B
    python tools/launch_trace_ab.py compare TRACE_A TRACE_B OUT_A OUT_B

`run` is a fixed sequence of C-ABI calls that puts a case on both sides of every rule the host launch layer decides by (batch-size
thresholds of the single step, two-wavefront capacity and slicing, store policies, chunk-major and pitched trajectories, time
limits, the five actors and their *_tl / *_boot / *_nrm kernels, pinned and scratch staging of host pointers, the tuning
overrides).  It writes every output array to OUT/<nnn>_<case>.<array>.npy - arrays above 4 MiB as their SHA-256 - and the return
code and rmav_last_error() of every call, refusals included, to OUT/calls.txt.
`compare` needs the ordered lists of (kernel, grid, workgroup, LDS bytes) of librmav's launches to be equal, and every file of
OUT_A to equal its twin in OUT_B byte for byte; exit status 1 otherwise."""
import csv
import ctypes as C
import glob
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "reinmav-gym_amd")]
BIG = 4 << 20
CAP = 131072          # two-wavefront capacity of every kind and action source: 16 384 x 8 pairs (csrc/rmav_abi.hip: split_pairs_max)


class Run:
    def __init__(self, out):
        import numpy as np
        import torch
        from gym_reinmav_amd import _abi as A

        self.np, self.torch, self.A, self.L, self.out = np, torch, A, A.lib(), out
        os.makedirs(out, exist_ok=True)
        self.log = open(os.path.join(out, "calls.txt"), "w")
        self.idx = 0
        rng = np.random.default_rng(5)
        self.ACT = torch.from_numpy(rng.uniform(0.0, 10.0, size=1 << 26).astype(np.float32)).cuda()      # caller actions of every case
        self.W = torch.from_numpy((0.05 * rng.standard_normal(1 << 20)).astype(np.float32)).cuda()       # policy weights, any layout
        self.act_host = self.ACT[: 1 << 22].cpu().numpy()

    # ---- plumbing
    def Z(self, n, dtype=None):
        return self.torch.zeros(int(n), dtype=dtype or self.torch.float32, device="cuda")

    def H(self, n, dtype=None):
        return self.np.zeros(int(n), dtype or self.np.float32)

    def P(self, t):
        return None if t is None else C.c_void_p(t.data_ptr() if self.torch.is_tensor(t) else t.ctypes.data)

    def make(self, kind, n, limit=0, track=True):
        A, h = self.A, C.c_void_p()
        k = A.KIND_BY_NAME[kind]
        flags = A.F_AUTO_RESET | (A.F_TRACK_EPISODES if track else 0)
        assert self.L.rmav_create(C.byref(h), k, n, 0, 7, 0, flags, None, None) == A.OK, self.L.rmav_last_error()
        if limit:
            assert self.L.rmav_set_time_limit(h, limit) == A.OK
        return h, A.STATE_DIM[k], A.ACTION_DIM[k]

    def tune(self, h, **kv):
        for k, v in kv.items():
            assert self.L.rmav_set_tuning(h, self.A.TUNE[k], v) == self.A.OK

    def done(self, tag, rc, **arrays):
        """one call: its return code and message, and its output arrays"""
        self.torch.cuda.synchronize()
        self.idx += 1
        self.log.write(f"{self.idx:03d} {tag}\t{rc}\t{self.L.rmav_last_error().decode() if rc else ''}\n")
        for name, t in arrays.items():
            if t is None or rc != self.A.OK:
                continue
            a = t.cpu().numpy() if self.torch.is_tensor(t) else t
            if a.nbytes > BIG:
                a = self.np.frombuffer(hashlib.sha256(self.np.ascontiguousarray(a)).digest(), self.np.uint8)
            self.np.save(os.path.join(self.out, f"{self.idx:03d}_{tag}.{name}.npy"), a)

    def close(self, tag, h, ns, n):
        s = self.Z(ns * n)
        self.torch.cuda.synchronize()
        self.done(tag + "_state", self.L.rmav_get_state(h, self.P(s), self.A.DEVICE, self.A.SOA), state=s)
        assert self.L.rmav_destroy(h) == self.A.OK
        print(f"{self.idx:4d} {tag}", flush=True)

    # ---- the calls, device pointers
    def rollout(self, tag, h, ns, na, n, T, mode, layout=0, pitch=0, chunk=0, fused=1):
        A, P, L = self.A, self.P, self.L
        cols = -(-n // chunk) * chunk if chunk else (pitch or n)
        ain = self.ACT[: T * na * cols] if mode == A.ACT_BUFFER else None
        aout = None if mode == A.ACT_BUFFER else self.Z(T * na * cols)
        obs, rew, dn = self.Z(T * ns * cols), self.Z(T * cols), self.Z(T * cols, self.torch.uint8)
        self.torch.cuda.synchronize()
        if chunk:
            rc = L.rmav_rollout_chunked(h, T, mode, P(ain), P(aout), P(obs), P(rew), P(dn), chunk)
        elif pitch:
            rc = L.rmav_rollout_pitched(h, T, mode, P(ain), P(aout), P(obs), P(rew), P(dn), pitch, fused)
        else:
            rc = L.rmav_rollout(h, T, mode, P(ain), P(aout), P(obs), P(rew), P(dn), A.DEVICE, layout, fused)
        self.done(tag, rc, act=aout, obs=obs, rew=rew, done=dn)

    def steps(self, tag, h, ns, na, n, final=True, control=True, layout=1, host=False):
        """step, step_final, step_control, control_step, control, reset, get_state (AoS) - on device buffers or host arrays"""
        A, P, L = self.A, self.P, self.L
        mem = A.HOST if host else A.DEVICE
        new = self.H if host else self.Z
        u8 = self.np.uint8 if host else self.torch.uint8
        act = self.act_host[: na * n] if host else self.ACT[: na * n]
        obs, rew, dn, fin, tr, nxt = new(ns * n), new(n), new(n, u8), new(ns * n), new(n, u8), new(na * n)
        self.torch.cuda.synchronize()
        self.done(tag + "_step", L.rmav_step(h, P(act), P(obs), P(rew), P(dn), mem, layout), obs=obs, rew=rew, done=dn)
        if final:
            self.done(tag + "_final", L.rmav_step_final(h, P(act), P(obs), P(rew), P(dn), P(fin), P(tr), mem, layout), obs=obs, rew=rew,
                      done=dn, final=fin, trunc=tr)
        if control:
            self.done(tag + "_stepctl", L.rmav_step_control(h, P(act), P(obs), P(rew), P(dn), P(nxt), mem, layout), obs=obs, rew=rew, done=dn, nxt=nxt)
            self.done(tag + "_ctlstep", L.rmav_control_step(h, P(nxt), P(obs), P(rew), P(dn), mem, layout), obs=obs, rew=rew, done=dn, act=nxt)
            self.done(tag + "_control", L.rmav_control(h, P(nxt), mem, layout), act=nxt)
        self.done(tag + "_getstate", L.rmav_get_state(h, P(obs), mem, A.AOS), state=obs)
        self.done(tag + "_reset", L.rmav_reset(h, P(obs), mem, layout), obs=obs)

    def policy(self, tag, h, ns, na, n, T, prec, boot=False, stats=None, trunc=True):
        P, L, u8 = self.P, self.L, self.torch.uint8
        act, obs, rew, dn = self.Z(T * na * n), self.Z(T * ns * n), self.Z(T * n), self.Z(T * n, u8)
        logp, val = self.Z(T * n), self.Z((T + 1) * n)
        bo, tr = (self.Z(T * n), self.Z(T * n, u8) if trunc else None) if boot else (None, None)
        self.torch.cuda.synchronize()
        if stats is not None:
            rc = L.rmav_rollout_policy_norm(h, T, P(self.W), P(stats), P(act), P(obs), P(rew), P(dn), P(logp), P(val), P(bo), P(tr), prec)
        elif boot:
            rc = L.rmav_rollout_policy_boot(h, T, P(self.W), P(act), P(obs), P(rew), P(dn), P(logp), P(val), P(bo), P(tr), prec)
        else:
            rc = L.rmav_rollout_policy(h, T, P(self.W), P(act), P(obs), P(rew), P(dn), P(logp), P(val), prec)
        self.done(tag, rc, act=act, obs=obs, rew=rew, done=dn, logp=logp, val=val, boot=bo, trunc=tr)
        if rc == self.A.OK and n <= 65536:   # the learner-side pass behind it
            adv, ret, sums = self.Z(T * n), self.Z(T * n), self.Z(2, self.torch.float64)
            self.torch.cuda.synchronize()
            if boot:
                rc = L.rmav_gae_boot(h, T, P(rew), P(dn), P(val), P(bo), 0.99, 0.95, 1.0, P(adv), P(ret), P(sums))
            else:
                rc = L.rmav_gae(h, T, P(rew), P(dn), P(val), 0.99, 0.95, 1.0, P(adv), P(ret), P(sums))
            self.done(tag + "_gae", rc, adv=adv, ret=ret, sums=sums)


QUADS = ("quad2d", "quad2d_sl", "quad3d", "quad3d_sl")
MODES = (("buf", 0), ("rnd", 1), ("ctl", 2))


def run(out):
    r = Run(out)
    A, L, P = r.A, r.L, r.P
    # ---- single steps: k_step's thresholds are 196 608 and 786 432 envs (step_store, step_lazy, step_block)
    for n in (65536, 196544, 196608, 786368, 786432):
        for limit in (0, 16):
            h, ns, na = r.make("quad3d", n, limit)
            r.steps(f"step_q3d_{n}_L{limit}", h, ns, na, n, control=n == 65536 or n == 786432)
            r.close(f"step_q3d_{n}_L{limit}", h, ns, n)
    for kind in QUADS + ("reinmav",):
        h, ns, na = r.make(kind, 65536, track=kind != "quad2d")
        r.steps(f"step_{kind}", h, ns, na, 65536, final=kind != "reinmav", control=kind != "reinmav", layout=A.SOA)
        r.close(f"step_{kind}", h, ns, 65536)
    for limit in (0, 16):
        h, ns, na = r.make("quad3d_sl", 65536, limit)
        for kv in (dict(block=64), dict(block=128), dict(block=-1, step_lazy=1), dict(step_lazy=0, step_store=1), dict(step_store=2), dict(step_store=0)):
            r.tune(h, **kv)
            r.steps(f"step_tune_L{limit}_" + "_".join(f"{k}{v}" for k, v in kv.items()), h, ns, na, 65536, control=False)
        r.close(f"step_tune_L{limit}", h, ns, 65536)
    h, ns, na = r.make("quad3d", 1048576)
    r.tune(h, step_lazy=0, block=256)
    r.steps("step_q3d_1M_eager", h, ns, na, 1048576, final=False, control=False)
    r.close("step_q3d_1M_eager", h, ns, 1048576)

    # ---- fused rollouts: every kind x action source; 65 536 and 131 072 (two wavefronts), just above the capacity (one wavefront)
    for kind in QUADS + ("reinmav",):
        for n, Ts in ((65536, (1, 4, 64)), (131072, (4, 64)), (CAP + 64, (4, 16, 64))):
            h, ns, na = r.make(kind, n)
            for T in Ts:
                for mname, mode in MODES:
                    if T == 64 and n != 65536 and mname != "rnd":   # (the long launches of the big batches: one action source)
                        continue
                    r.rollout(f"roll_{kind}_{n}_T{T}_{mname}", h, ns, na, n, T, mode)
            r.close(f"roll_{kind}_{n}", h, ns, n)
    # two rounds of the two-wavefront kernel: slung-load kinds, random actions, 1.75 .. 2 x the capacity; 1.5 x stays one launch
    for kind in QUADS:
        for n in (196608, 245760):
            h, ns, na = r.make(kind, n)
            r.rollout(f"rounds_{kind}_{n}_rnd", h, ns, na, n, 16, A.ACT_RANDOM)
            r.rollout(f"rounds_{kind}_{n}_ctl", h, ns, na, n, 4, A.ACT_CONTROLLER)
            if n == 245760:
                for kv in (dict(slice=0), dict(slice=1), dict(slice=-1, split=1), dict(split=0)):
                    r.tune(h, **kv)
                    r.rollout(f"rounds_{kind}_{n}_" + "_".join(f"{k}{v}" for k, v in kv.items()), h, ns, na, n, 4, A.ACT_RANDOM)
            r.close(f"rounds_{kind}_{n}", h, ns, n)
    # time-limited handles: the one-wavefront kernels, both sides of the 192 MB store rule (quad2d 138 MB, quad3d 250 MB at 64 steps)
    for kind in QUADS:
        h, ns, na = r.make(kind, 65536, 16)
        for T in (1, 4, 64):
            for mname, mode in MODES:
                r.rollout(f"tl_{kind}_T{T}_{mname}", h, ns, na, 65536, T, mode)
        r.rollout(f"tl_{kind}_unfused", h, ns, na, 65536, 3, A.ACT_RANDOM, fused=0)
        r.close(f"tl_{kind}", h, ns, 65536)
    # feature-major with N off the 16-env granule and its pitched twin; batch-major below and above the 448 MB rule; chunk-major
    for limit in (0, 16):
        t = f"L{limit}"
        h, ns, na = r.make("quad3d", 65599, limit)
        r.rollout(f"odd_{t}_soa", h, ns, na, 65599, 64, A.ACT_RANDOM)
        r.rollout(f"odd_{t}_pitched", h, ns, na, 65599, 64, A.ACT_RANDOM, pitch=int(L.rmav_trajectory_pitch(h)))
        r.rollout(f"odd_{t}_pitched_buf", h, ns, na, 65599, 8, A.ACT_BUFFER, pitch=int(L.rmav_trajectory_pitch(h)))
        r.close(f"odd_{t}", h, ns, 65599)
        for n, T in ((65536, 64), (CAP + 64, 32), (CAP + 64, 64)):
            h, ns, na = r.make("quad3d", n, limit)
            r.rollout(f"aos_{t}_{n}_T{T}", h, ns, na, n, T, A.ACT_RANDOM, layout=A.AOS)
            if T == 32:
                for sp in (0, 3, 1):
                    r.tune(h, store_policy=sp)
                    r.rollout(f"aos_{t}_{n}_T{T}_sp{sp}", h, ns, na, n, T, A.ACT_CONTROLLER, layout=A.AOS)
            r.close(f"aos_{t}_{n}_T{T}", h, ns, n)
        for n in (100000, 150000):   # 2 and 3 chunks of 65 536, the last one partial
            h, ns, na = r.make("quad3d", n, limit)
            for mname, mode in MODES:
                r.rollout(f"chunk_{t}_{n}_{mname}", h, ns, na, n, 8, mode, chunk=65536)
            r.rollout(f"chunk_{t}_{n}_one", h, ns, na, n, 8, A.ACT_RANDOM, chunk=196608)
            r.close(f"chunk_{t}_{n}", h, ns, n)
    h, ns, na = r.make("quad3d_sl", 65536)
    for kv in (dict(split=0), dict(split=-1, split_group=2), dict(split_group=8), dict(split_group=-1, store_policy=0), dict(store_policy=1),
               dict(store_policy=2), dict(store_policy=2, split=0), dict(store_policy=-1, block=128, split=0)):
        r.tune(h, **kv)
        for mname, mode in MODES:
            r.rollout("tune_" + "_".join(f"{k}{v}" for k, v in kv.items()) + "_" + mname, h, ns, na, 65536, 8, mode)
    r.close("tune", h, ns, 65536)

    # ---- policy rollouts: the pairs-per-workgroup rule changes at 98 304 envs
    T = 4
    for n in (65536, 131072):
        stats = r.torch.zeros(int(L.rmav_obs_norm_bytes()), dtype=r.torch.uint8, device="cuda")
        for limit in (0, 16):
            h, ns, na = r.make("quad3d", n, limit)
            t = f"pol_{n}_L{limit}"
            r.done(t + "_norm_init", L.rmav_obs_norm_init(h, P(stats), 5.0, 1e-8, 1e-4), stats=stats)
            for forced in (-1, 1, 3):
                r.tune(h, pair_group=forced)
                for prec in range(5):
                    r.policy(f"{t}_g{forced}_p{prec}", h, ns, na, n, T, prec)
                    r.policy(f"{t}_g{forced}_p{prec}_boot", h, ns, na, n, T, prec, boot=True, trunc=prec != 3)
                    r.policy(f"{t}_g{forced}_p{prec}_norm", h, ns, na, n, T, prec, boot=limit > 0, stats=stats)
            r.tune(h, pair_group=-1, policy_pair=0)
            r.policy(f"{t}_bf16_1w", h, ns, na, n, T, A.POLICY_BF16_MFMA)
            r.close(t, h, ns, n)
    for kind in QUADS:
        h, ns, na = r.make(kind, 65536)
        for prec in range(5):
            r.policy(f"pol_{kind}_p{prec}", h, ns, na, 65536, T, prec)
        r.close(f"pol_{kind}", h, ns, 65536)

    # ---- host pointers: the completion-word path (<= 64 envs), the pinned block, device scratch
    for kind, n in (("quad3d", 64), ("quad3d", 1000), ("quad3d", 65536), ("quad2d_sl", 48), ("reinmav", 64), ("reinmav", 65536)):
        for limit in ((0,) if kind == "reinmav" else (0, 16)):
            h, ns, na = r.make(kind, n, limit)
            t = f"host_{kind}_{n}_L{limit}"
            for layout in (A.AOS, A.SOA):
                r.steps(f"{t}_lay{layout}", h, ns, na, n, final=kind != "reinmav", control=kind != "reinmav", layout=layout, host=True)
            for mname, mode in MODES:
                ain = r.act_host[: 4 * na * n] if mode == A.ACT_BUFFER else None
                aout, obs, rew, dn = r.H(4 * na * n), r.H(4 * ns * n), r.H(4 * n), r.H(4 * n, r.np.uint8)
                for fused in (1, 0):
                    rc = L.rmav_rollout(h, 4, mode, P(ain), P(aout), P(obs), P(rew), P(dn), A.HOST, A.SOA, fused)
                    r.done(f"{t}_roll_{mname}_f{fused}", rc, act=aout, obs=obs, rew=rew, done=dn)
            assert L.rmav_set_stream(h, None) == A.OK   # a fresh stream of the handle's own
            r.steps(f"{t}_restream", h, ns, na, n, final=False, control=False, host=True)
            r.close(t, h, ns, n)

    # ---- refusals (tests/test_gpu_bootstrap.py, test_gpu_obs_norm.py, test_gpu_time_limit.py, test_gpu_boundary.py): code and message
    n, T = 256, 4
    stats = r.torch.zeros(int(L.rmav_obs_norm_bytes()) + 16, dtype=r.torch.uint8, device="cuda")
    good, bad = stats[:-16], stats[4:-12]
    env, lim, rm = r.make("quad3d", n)[0], r.make("quad3d", n, 8)[0], r.make("reinmav", 64)[0]
    # (some of the combinations below are valid calls: every buffer has the size its argument needs)
    w, x, u, lp, bout = r.W, r.Z((T + 1) * n), r.Z(T * n, r.torch.uint8), r.Z(T * n), r.Z(T * n)
    for k in range(-1, 7):
        r.done(f"refuse_weight_count_{k}", min(int(L.rmav_policy_weight_count(k)), 0))
    r.done("refuse_norm_init_ok", L.rmav_obs_norm_init(env, P(good), 10.0, 1e-8, 1e-4))
    for name, hh in (("env", env), ("lim", lim), ("rm", rm)):
        for prec in (0, 1, 2, 3, 4, 9, -1):
            r.done(f"refuse_policy_{name}_p{prec}_T0", L.rmav_rollout_policy(hh, 0, P(w), None, None, None, None, P(lp), P(x), prec))
            r.done(f"refuse_policy_{name}_p{prec}_nologp", L.rmav_rollout_policy(hh, T, P(w), None, None, None, None, None, P(x), prec))
            r.done(f"refuse_policy_{name}_p{prec}_unaligned", L.rmav_rollout_policy(hh, T, C.c_void_p(w.data_ptr() + 4), None, None, None, None, P(lp), P(x), prec))
            for bo in (bout, None):
                b = "boot" if bo is not None else "noboot"
                r.done(f"refuse_boot_{name}_p{prec}_{b}", L.rmav_rollout_policy_boot(hh, T, P(w), None, None, None, None, P(lp), P(x), P(bo), None, prec))
                r.done(f"refuse_boot_{name}_p{prec}_{b}_T0", L.rmav_rollout_policy_boot(hh, 0, P(w), None, None, None, None, P(lp), None, P(bo), None, prec))
                for st, sname in ((good, "good"), (bad, "bad"), (None, "none")):
                    for tr in (u, None):
                        tag = f"refuse_norm_{name}_p{prec}_{b}_{sname}_{'trunc' if tr is not None else 'notrunc'}"
                        r.done(tag, L.rmav_rollout_policy_norm(hh, T, P(w), P(st), None, None, None, None, P(lp), P(x), P(bo), P(tr), prec))
                r.done(f"refuse_norm_{name}_p{prec}_{b}_nologp", L.rmav_rollout_policy_norm(hh, T, P(w), P(good), None, None, None, None, None, P(x), P(bo), None, prec))
                r.done(f"refuse_norm_{name}_p{prec}_{b}_T0", L.rmav_rollout_policy_norm(hh, 0, P(w), P(good), None, None, None, None, P(lp), P(x), P(bo), None, prec))
        z = C.c_void_p(0)
        r.done(f"refuse_gae_{name}_T0", L.rmav_gae(hh, 0, P(x), P(u), P(x), 0.99, 0.95, 1.0, P(x), P(x), z))
        r.done(f"refuse_gae_{name}_norew", L.rmav_gae(hh, T, z, P(u), P(x), 0.99, 0.95, 1.0, P(x), P(x), z))
        r.done(f"refuse_gaeboot_{name}_T0", L.rmav_gae_boot(hh, 0, P(x), P(u), P(x), P(x), 0.99, 0.95, 1.0, P(x), P(x), z))
        r.done(f"refuse_gaeboot_{name}_noboot", L.rmav_gae_boot(hh, T, P(x), P(u), P(x), z, 0.99, 0.95, 1.0, P(x), P(x), z))
        r.done(f"refuse_stepfinal_{name}", L.rmav_step_final(hh, None, P(x), P(x), P(u), P(x), P(u), A.DEVICE, A.AOS))
        r.done(f"refuse_stepctl_{name}", L.rmav_step_control(hh, P(x), P(x), None, None, None, A.DEVICE, A.AOS))
        if name == "rm":
            r.done("refuse_stepctl_reinmav", L.rmav_step_control(hh, P(x), P(x), None, None, P(x), A.DEVICE, A.AOS))
        r.done(f"refuse_control_{name}_null", L.rmav_control(hh, None, A.DEVICE, A.AOS))
        r.done(f"refuse_reset_{name}_layout", L.rmav_reset(hh, None, A.DEVICE, 7))
        r.done(f"refuse_rollout_{name}_mode", L.rmav_rollout(hh, T, 5, None, None, None, None, None, A.DEVICE, A.SOA, 1))
        r.done(f"refuse_rollout_{name}_noact", L.rmav_rollout(hh, T, A.ACT_BUFFER, None, None, None, None, None, A.DEVICE, A.SOA, 1))
        r.done(f"refuse_pitched_{name}", L.rmav_rollout_pitched(hh, T, A.ACT_RANDOM, None, None, None, None, None, 8, 1))
        r.done(f"refuse_chunked_{name}_T1", L.rmav_rollout_chunked(hh, 1, A.ACT_RANDOM, None, None, None, None, None, 64))
        r.done(f"refuse_chunked_{name}_odd", L.rmav_rollout_chunked(hh, T, A.ACT_RANDOM, None, None, None, None, None, 100))
        r.done(f"refuse_limit_{name}", L.rmav_set_time_limit(hh, -1))
    r.done("refuse_gae_nullhandle", L.rmav_gae(None, T, P(x), P(u), P(x), 0.99, 0.95, 1.0, P(x), P(x), None))
    for hh in (env, lim, rm):
        assert L.rmav_destroy(hh) == A.OK
    r.log.close()
    print(f"{r.idx} calls recorded in {out}")


def launches(trace_dir):
    """ordered (kernel, grid, workgroup, LDS bytes) of librmav's launches in a rocprofv3 --kernel-trace directory"""
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows = [x for x in rows if "rmav" in x["Kernel_Name"]]
    rows.sort(key=lambda x: int(x.get("Dispatch_Id") or x["Start_Timestamp"]))

    def dims(x, key):
        return tuple(int(x[k]) for k in (key + "_X", key + "_Y", key + "_Z")) if key + "_X" in x else x[key]

    return [(x["Kernel_Name"], dims(x, "Grid_Size"), dims(x, "Workgroup_Size"), int(x["LDS_Block_Size"])) for x in rows]


def compare(trace_a, trace_b, out_a, out_b):
    bad = 0
    a, b = launches(trace_a), launches(trace_b)
    diff = [i for i, (p, q) in enumerate(zip(a, b)) if p != q]
    print(f"launches: {len(a)} vs {len(b)}, {len(set(x[0] for x in a))} distinct kernels, {len(diff)} differ")
    for i in diff[:10]:
        print(f"  launch {i}:\n    A {a[i]}\n    B {b[i]}")
    bad += len(a) != len(b) or bool(diff) or not a
    fa, fb = sorted(os.listdir(out_a)), sorted(os.listdir(out_b))
    differ = [f for f in fa if f in fb and open(os.path.join(out_a, f), "rb").read() != open(os.path.join(out_b, f), "rb").read()]
    print(f"files: {len(fa)} vs {len(fb)}, {len(differ)} differ (calls.txt holds every return code and message)")
    for f in differ[:20]:
        print("  differs: " + f)
    bad += fa != fb or bool(differ) or not fa
    print("EQUAL" if not bad else "DIFFERENT")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 6 and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:]))
    else:
        raise SystemExit(__doc__)

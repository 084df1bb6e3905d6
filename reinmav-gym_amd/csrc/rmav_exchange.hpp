// rmav_exchange.hpp - the kernels of the episode statistics exchange (include/rmav_comm.h).  rmav_comm_abi.hip only: they are
// ordinary external definitions, one translation unit each.
#pragma once

#include "rmav_kernels.hpp"   // EnvRec, wall_clock64

namespace rmav {

// ---- episode statistics exchange (the path's one collective) ------------------------------------------------
// send = [2][cmax] int32: returns (bit pattern) then lengths of this rank's `count` envs, zero padded to cmax
__global__ __launch_bounds__(256) void k_pack_stats(const float *__restrict__ last_ret, const EnvRec *__restrict__ rec,
                                                    int64_t count, int64_t cmax, int32_t *__restrict__ send) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cmax) return;
    send[i] = i < count ? __float_as_int(last_ret[i]) : 0;
    send[cmax + i] = i < count ? rec[i].last_len : 0;
}
// one thread: publish `seq` in a signal word another HIP stream waits on with hipStreamWaitValue32 (the kernel boundary
// in front of this launch has released the payload).  Folding this into k_pack_stats - every workgroup releases and takes
// a ticket, the last one signals - measured SLOWER (exchange cost per 131 072-env rollout +15..19 us instead of +9..15:
// 512 agent-scope releases each write the L2 back) - profiles/r02/handover_chunk.md.
__global__ void k_signal(uint32_t *flag, uint32_t seq) {
    __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// The communicator's stream waits here until every wavefront of the armed rollout launch has published `seq` (or a later
// post's) in its arrival word: one workgroup polling `count` words with agent-scope loads.  hipStreamWaitValue32 is a
// spinning one-wavefront kernel of the runtime as well (__amd_rocclr_streamOpsWait in the kernel trace); this one waits
// for the rollout kernel's own wavefronts, so the compute stream needs no pack and no signal kernel.
// Bounded, so that a communicator stream can never spin for ever (it would block every other rank's collective too):
//   * `after_start_ticks` (2 s of the constant 100 MHz clock) from the moment the armed launch's first workgroup published
//     `seq` in *started - NOT from when this waiter began: an armed rollout may sit behind seconds of queued compute-stream work
//     (a PPO update, another job on the GPU), and a clock that started here gave up on launches that had not begun yet
//     (ADVICE r03);
//   * `total_ticks` (10 min) overall, against a launch that never runs at all (device fault after a successful enqueue).
// On giving up the waiter POISONS this rank's payload - return = NaN, length = -1 for every env - writes `seq` into
// *timeout_seq (pinned host memory, one word per buffer pair: rmav_allgather_stats_wait / _result report RMAV_ERR_TIMEOUT for
// THAT post only) and lets the stream go on: the collective is still issued, so the peers neither hang nor mistake the
// half-written snapshot for statistics.
__global__ __launch_bounds__(256) void k_wait_arrivals(const uint32_t *arrive, uint32_t count, uint32_t seq, const uint32_t *started,
                                                       unsigned long long after_start_ticks, unsigned long long total_ticks,
                                                       uint32_t *timeout_seq, int32_t *send, int64_t cmax) {
    const unsigned long long t0 = wall_clock64();
    unsigned long long t_start = 0;   // per thread: when THIS thread first saw the launch begun (the give-up decision is made uniform below)
    for (;;) {
        int ok = 1;
        for (uint32_t i = threadIdx.x; i < count; i += 256u)
            ok &= (int32_t)(__hip_atomic_load(arrive + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - seq) >= 0;
        if (__syncthreads_and(ok)) break;
        const unsigned long long now = wall_clock64();
        // (started == nullptr: a kernel family that publishes no start word - only the overall bound applies)
        const int begun = started ? __syncthreads_or((int32_t)(__hip_atomic_load(started, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - seq) >= 0) : 0;
        // (signed differences: the threads read the clock a few ticks apart, and an unsigned `now - t_start` of a thread that read
        // it just BEFORE the one whose reading became t_start would wrap around to "expired")
        int expired = (long long)(now - t0) > (long long)total_ticks;
        if (begun) {
            if (t_start == 0) t_start = now | 1ull;
            expired |= (long long)(now - t_start) > (long long)after_start_ticks;
        }
        if (__syncthreads_or(expired)) {
            for (int64_t i = threadIdx.x; i < cmax; i += 256) {
                send[i] = 0x7fc00000;      // NaN
                send[cmax + i] = -1;
            }
            if (threadIdx.x == 0) __hip_atomic_store(timeout_seq, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            break;
        }
        __builtin_amdgcn_s_sleep(32);
    }
}
// recv = [world][2][cmax] -> returns_out / lengths_out [n_total] in global env order (rank r owns
// base + (r < rem) envs starting at r * base + min(r, rem))
__global__ __launch_bounds__(256) void k_unpack_stats(const int32_t *__restrict__ recv, int64_t n_total, int32_t world,
                                                      int64_t cmax, float *__restrict__ ret_out, int32_t *__restrict__ len_out) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_total) return;
    const int64_t base = n_total / world, rem = n_total % world;
    // owner of global env g: the first `rem` ranks hold base + 1 envs
    const int64_t cut = rem * (base + 1);
    int64_t r, local;
    if (g < cut) {
        r = g / (base + 1);
        local = g - r * (base + 1);
    } else {
        r = rem + (g - cut) / base;
        local = (g - cut) - (r - rem) * base;
    }
    const int32_t *src = recv + r * 2 * cmax;
    ret_out[g] = __int_as_float(src[local]);
    len_out[g] = src[cmax + local];
}

}  // namespace rmav

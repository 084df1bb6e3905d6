// rmav_core_kernels.hpp - the small kernels behind the accessors of include/rmav.h: the per-env records (EnvRec), the draw of a
// handle's parameter ranges, ReinmavEnv's control() and the layout conversions.  rmav_abi.hip only: they are ordinary (or
// internal-linkage) definitions, which a second translation unit would duplicate.
#pragma once

#include "rmav_kernels.hpp"

namespace rmav {

// running episode lengths for rmav_episode_buffers: clock - ep_start
__global__ __launch_bounds__(256) void k_cur_length(int32_t *out, const EnvRec *rec, uint32_t clock, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (int32_t)(clock - rec[i].ep_start);
}

// the episode clock moved by `delta` (rmav_seed, rmav_set_step_count): every running episode's start moves with it
__global__ __launch_bounds__(256) void k_shift_ep_start(EnvRec *rec, uint32_t delta, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) rec[i].ep_start += delta;
}

// The constants of every env's RUNNING episode - reset index = resets drawn so far - 1 - for the parameters of dr.mask:
// rmav_set_env_param_range's initial draw, and rmav_reset's redraw behind k_reset.
__global__ __launch_bounds__(kBlock) void k_range_draw(const RangeArgs dr, const EnvRec *rec, int64_t n, uint64_t seed, uint64_t env_base) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v[3] = {0.0f, 0.0f, 0.0f};
    range_draw(dr, seed, env_base + (uint64_t)i, rec[i].reset_cnt - 1u, v);
#pragma unroll
    for (int w = 0; w < 3; ++w)
        if ((dr.mask >> w) & 1u) dr.pe[w][i] = v[w];
}

// One 32-bit field of the per-env records <-> a dense array (rmav_get_sbd / rmav_set_sbd, the reset counters, last lengths: the
// accessors of the C ABI; not on any hot path).  field = word index in EnvRec: 0 sbd, 1 reset_cnt, 2 ep_start, 3 last_len.
__global__ __launch_bounds__(256) void k_rec_get(uint32_t *out, const EnvRec *rec, int field, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = reinterpret_cast<const uint32_t *>(rec)[4 * i + field];
}
__global__ __launch_bounds__(256) void k_rec_set(EnvRec *rec, const uint32_t *in, int field, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) reinterpret_cast<uint32_t *>(rec)[4 * i + field] = in[i];
}
// field < 0: every record = `value`; otherwise that field of every record = value's
__global__ __launch_bounds__(256) void k_rec_fill(EnvRec *rec, EnvRec value, int field, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (field < 0) rec[i] = value;
    else reinterpret_cast<uint32_t *>(rec)[4 * i + field] = reinterpret_cast<const uint32_t *>(&value)[field];
}

// ReinmavEnv: the built-in controller's command (F, Mx, My, Mz) at the env's current (state, t)
[[maybe_unused]] static __global__ __launch_bounds__(kBlock) void k_control_reinmav(const float *state, const double *env_time, int64_t n,
                                                            float *act_out, uint32_t flags, const ReinmavP p) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s[13], fm[4];
#pragma unroll
    for (int c = 0; c < 13; ++c) s[c] = state[(int64_t)c * n + i];
    double R[3][3];
    {
        const double q[4] = {s[6], s[7], s[8], s[9]};
        reinmav_quat2mat(q, R);
    }
    reinmav_controller(p, s, R, env_time[i], fm);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (flags & F_AOS) act_out[i * 4 + c] = (float)fm[c];
        else act_out[(int64_t)c * n + i] = (float)fm[c];
    }
}

// [dim][n] <-> [n][dim]
[[maybe_unused]] static __global__ __launch_bounds__(kBlock) void k_soa_to_aos(const float *src, float *dst, int64_t n, int dim) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int c = 0; c < dim; ++c) dst[i * dim + c] = src[(int64_t)c * n + i];
}
[[maybe_unused]] static __global__ __launch_bounds__(kBlock) void k_aos_to_soa(const float *src, float *dst, int64_t n, int dim) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int c = 0; c < dim; ++c) dst[(int64_t)c * n + i] = src[i * dim + c];
}

}  // namespace rmav

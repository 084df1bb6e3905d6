// rmav_ret_norm.hpp - return normalisation (the reward half of baselines' VecNormalize, restated in include/rmav_ppo.h) on the
// device: the forward scan that turns a [T][N] reward trajectory into the moments of the per-env discounted return
// R_t = gamma R_{t-1} + s r_t, their merge into ONE scalar RunningMeanStd, the elementwise scaling, and GAE with that scaling
// applied to every reward as it is loaded (k_gae_norm: k_gae / k_gae_boot of rmav_gae.hpp with one multiply and one clamp in front).
//
// The moments reuse the machinery of rmav_obs_norm.hpp (shifted_moment, chan, fold_partials, rstd_entry): per lane sum (R - K) and
// sum (R - K)^2 in fp64 with K = the lane's first return, Chan's pairwise combination above that in a fixed order - the merge into
// the running state included - no floating-point atomics: the same input gives the same bits.  k_gae_norm is a wrapper of
// gae_body (rmav_gae.hpp) that hands it ret_norm_apply.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "rmav_gae.hpp"
#include "rmav_obs_norm.hpp"

namespace rmav {

// The caller-owned statistics buffer (rmav_ret_norm_bytes() = sizeof, 16-byte aligned; include/rmav_ppo.h documents the fields)
struct RetNormStats {
    double count;
    double mean;
    double m2;
    double eps;
    float clip;
    float pad0[3];
    float rstd_f;   // <- the table the kernels read starts here (byte 48): rstd_f | clip_f | pad
    float clip_f;
    float pad1[2];
};
static_assert(sizeof(RetNormStats) == 64 && offsetof(RetNormStats, clip) == 32 && offsetof(RetNormStats, rstd_f) == 48 &&
                  offsetof(RetNormStats, clip_f) == 52,
              "layout documented in include/rmav_ppo.h");
constexpr int kRetMomentWords = 3;   // a batch record: count, mean, m2

// THE arithmetic of reward normalisation, fp32, uncontracted, in this order (include/rmav_ppo.h): scale, multiply, clamp
__device__ __forceinline__ float ret_norm_apply(float r, float rew_scale, float rstd, float clip) {
    const float z = (rew_scale * r) * rstd;
    return __builtin_amdgcn_fmed3f(z, -clip, clip);
}

// Stage 1.  One env per lane walks its column FORWARDS: R = gamma R + s r_t enters the lane's moments, then R = 0 where the
// episode ended with step t.  carry [N]: R before the first step, in; R after the last one, out.  4 + 1 bytes read per sample;
// the loads of a chunk of kGaeUnroll steps do not depend on the recurrence and are issued ahead of it, as in k_gae.
// partial [gridDim.x] moments.
__global__ __launch_bounds__(256) void k_ret_moments(const float *__restrict__ rew, const uint8_t *__restrict__ done,
                                                     float *__restrict__ carry, int64_t n, int32_t T, float rew_scale, float gamma,
                                                     Moment *__restrict__ partial) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double k0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (i < n) {
        float R = carry[i];
        int32_t t = 0;
        {   // step 0 fixes the shift K (T >= 1: the launcher sends T = 0 straight to the fold)
            R = fmaf(gamma, R, rew_scale * rew[i]);
            k0 = (double)R;
            if (done[i]) R = 0.0f;
            t = 1;
        }
        auto take = [&](float r, uint8_t d) {
            R = fmaf(gamma, R, rew_scale * r);
            const double x = (double)R - k0;
            s1 += x;
            s2 = fma(x, x, s2);
            if (d) R = 0.0f;
        };
        // head: bring T - t to a multiple of the unroll factor
        for (; t < T && ((T - t) % kGaeUnroll) != 0; ++t) {
            const int64_t o = (int64_t)t * n + i;
            take(rew[o], done[o]);
        }
        for (; t < T; t += kGaeUnroll) {
            float r[kGaeUnroll];
            uint8_t d[kGaeUnroll];
#pragma unroll
            for (int j = 0; j < kGaeUnroll; ++j) {
                const int64_t o = (int64_t)(t + j) * n + i;
                r[j] = rew[o];
                d[j] = done[o];
            }
#pragma unroll
            for (int j = 0; j < kGaeUnroll; ++j) take(r[j], d[j]);
        }
        carry[i] = R;
    }
    const Moment m = block_chan(shifted_moment(i < n ? (double)T : 0.0, k0, s1, s2));
    if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

// Stage 2.  One block folds the partials into batch_out = (count, mean, m2); nblk = 0 leaves the empty record.
__global__ __launch_bounds__(256) void k_ret_moments_fold(const Moment *__restrict__ partial, int32_t nblk, double *__restrict__ batch_out) {
    const Moment m = fold_partials(partial, nblk);
    if (threadIdx.x == 0) {
        batch_out[0] = m.n;
        batch_out[1] = m.mean;
        batch_out[2] = m.m2;
    }
}

// the fp32 table from the running state
__device__ __forceinline__ void ret_norm_table(RetNormStats *st, double count, double m2, double eps, float clip) {
    st->rstd_f = rstd_entry(count, m2, eps);
    st->clip_f = clip;
}

__global__ __launch_bounds__(64) void k_ret_norm_init(RetNormStats *st, float clip, double eps, double count0) {
    if (threadIdx.x != 0) return;
    st->count = count0;
    st->mean = 0.0;
    st->m2 = count0;   // var = 1
    st->eps = eps;
    st->clip = clip;
    st->pad0[0] = st->pad0[1] = st->pad0[2] = 0.0f;
    st->pad1[0] = st->pad1[1] = 0.0f;
    ret_norm_table(st, count0, count0, eps, clip);
}

// running state <- running state merged with n_batches records, in order (k_obs_norm_merge for one scalar: chan() per record).
// chan() takes a running count of exactly 0 as "no sample yet" and returns the record as it is; _init refuses count0 <= 0, so only a
// buffer written by the caller can hold one.
__global__ __launch_bounds__(64) void k_ret_norm_merge(RetNormStats *st, const double *__restrict__ batch, int32_t n_batches) {
    if (threadIdx.x != 0) return;
    Moment run{st->count, st->mean, st->m2};
    for (int32_t b = 0; b < n_batches; ++b) {
        const double *rec = batch + (int64_t)b * kRetMomentWords;
        if (!(rec[0] > 0.0)) continue;
        run = chan(run, Moment{rec[0], rec[1], rec[2]});
    }
    st->count = run.n;
    st->mean = run.mean;
    st->m2 = run.m2;
    ret_norm_table(st, run.n, run.m2, st->eps, st->clip);
}

// out = clamp((rew_scale * in) * rstd_f, -clip, clip), one element per thread; out == in allowed
__global__ __launch_bounds__(256) void k_ret_normalize(const RetNormStats *__restrict__ st, const float *in, float *out, int64_t count,
                                                       float rew_scale) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= count) return;
    out[q] = ret_norm_apply(in[q], rew_scale, st->rstd_f, st->clip_f);
}

// k_gae (BOOT = false) / k_gae_boot (BOOT = true) with the reward normalised as it is loaded:
//   z_t = clamp((rew_scale r_t) * rstd_f, -clip, clip);   delta_t = z_t + gamma ((1 - done_t) V_{t+1} [+ boot_t]) - V_t
// rstd_f / clip_f come from the statistics buffer (one uniform load per wavefront), so the learner never reads the scale back, and
// the normalised rewards never make a round trip through memory: the bytes are k_gae's / k_gae_boot's.  z - v is what their
// fmaf(r, 1, -v) rounds to, so on rewards normalised by k_ret_normalize (rew_scale = 1 there) they give these bits.
template <bool BOOT>
__global__ __launch_bounds__(256) void k_gae_norm(const float *__restrict__ rew, const uint8_t *__restrict__ done,
                                                  const float *__restrict__ val, const float *__restrict__ boot,
                                                  const RetNormStats *__restrict__ st, float *__restrict__ adv, float *__restrict__ ret,
                                                  int64_t n, int32_t T, float gamma, float lam, float rew_scale,
                                                  double *__restrict__ partial) {
    const float rstd = st->rstd_f, clip = st->clip_f;
    gae_body<BOOT>(rew, done, val, boot, adv, ret, n, T, gamma, lam,
                   [=](float r, float v) { return ret_norm_apply(r, rew_scale, rstd, clip) - v; }, partial);
}

}  // namespace rmav

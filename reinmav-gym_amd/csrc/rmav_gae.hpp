// rmav_gae.hpp - generalised advantage estimation over the time-major [T][N] trajectory a fused rollout leaves
// in HBM (the PPO2 caller loop of gym_reinmav/run.py:63-68; baselines ppo2 Runner.run() computes
//   delta_t = r_t + gamma V_{t+1} (1 - done_t) - V_t ,   A_t = delta_t + gamma lambda (1 - done_t) A_{t+1}
// backwards over the nsteps it collected, returns = A + V).
//
// One env per lane, like the dynamics kernels: lane i walks its own column backwards, so every access of a
// time step is one coalesced 256-byte (64-byte for `done`) wave transaction and the recurrence lives in two
// registers.  9 bytes read + 8 written per sample: a pure HBM stream.  The loads of a chunk of kGaeUnroll
// steps do not depend on the recurrence, so they are all issued before the first one is consumed.
// The kernels also leave sum / sum-of-squares of the advantages (per-block partials in fp64, folded by
// k_gae_fold) for the advantage normalisation of the learner.
//
// The scan is written once, gae_body; k_gae, k_gae_boot and k_gae_norm (rmav_ret_norm.hpp) are wrappers that hand it their reward
// term.  The block reduction of the sums is written once too, block_sum2.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace rmav {

constexpr int kGaeUnroll = 8;

// The block's (sum, sum of squares) in fp64 -> out[0..1], by thread 0: lanes by shuffles, the block's nwaves <= 4 wavefronts
// through LDS, in a fixed order.
__device__ __forceinline__ void block_sum2(double d1, double d2, int nwaves, double *__restrict__ out) {
    __shared__ double sh[2][4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        d1 += __shfl_down(d1, off, 64);
        d2 += __shfl_down(d2, off, 64);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sh[0][w] = d1;
        sh[1][w] = d2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a1 = 0.0, a2 = 0.0;
        for (int k = 0; k < nwaves; ++k) {
            a1 += sh[0][k];
            a2 += sh[1][k];
        }
        out[0] = a1;
        out[1] = a2;
    }
}

// THE reverse scan, behind every kernel of the family.  reward_term(r, v) = the reward as it enters delta, minus V_t: the one
// expression the kernels differ in.  BOOT adds the bootstrap term of truncated steps (one more coalesced load stream `boot`):
//   delta_t = reward_term(r_t, V_t) + gamma ((1 - done_t) V_{t+1} [+ boot_t])
// It enters as one fma around the term, so boot = 0 gives the values of BOOT = false.
template <bool BOOT, typename RewardTerm>
__device__ __forceinline__ void gae_body(const float *__restrict__ rew, const uint8_t *__restrict__ done, const float *__restrict__ val,
                                         const float *__restrict__ boot, float *__restrict__ adv, float *__restrict__ ret, int64_t n,
                                         int32_t T, float gamma, float lam, RewardTerm reward_term, double *__restrict__ partial) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float s1 = 0.0f, s2 = 0.0f;
    if (i < n) {
        float v_next = val[(int64_t)T * n + i];
        float last = 0.0f;
        const float gl = gamma * lam;
        int32_t t = T - 1;
        auto step = [&](int64_t o, float r, float v, float nt, float b) {
            const float term = reward_term(r, v);
            const float delta = fmaf(gamma * nt, v_next, BOOT ? fmaf(gamma, b, term) : term);
            last = fmaf(gl * nt, last, delta);
            adv[o] = last;
            ret[o] = last + v;
            s1 += last;
            s2 = fmaf(last, last, s2);
            v_next = v;
        };
        // head: bring t + 1 to a multiple of the unroll factor
        for (; t >= 0 && ((t + 1) % kGaeUnroll) != 0; --t) {
            const int64_t o = (int64_t)t * n + i;
            step(o, rew[o], val[o], done[o] ? 0.0f : 1.0f, BOOT ? boot[o] : 0.0f);
        }
        for (; t >= 0; t -= kGaeUnroll) {
            float r[kGaeUnroll], v[kGaeUnroll], nt[kGaeUnroll], b[kGaeUnroll];
#pragma unroll
            for (int j = 0; j < kGaeUnroll; ++j) {
                const int64_t o = (int64_t)(t - j) * n + i;
                r[j] = rew[o];
                v[j] = val[o];
                b[j] = BOOT ? boot[o] : 0.0f;
                nt[j] = done[o] ? 0.0f : 1.0f;
            }
#pragma unroll
            for (int j = 0; j < kGaeUnroll; ++j) step((int64_t)(t - j) * n + i, r[j], v[j], nt[j], b[j]);
        }
    }
    if (partial) block_sum2((double)s1, (double)s2, (int)(blockDim.x >> 6), partial + 2 * blockIdx.x);   // uniform branch
}

// delta_t = rew_scale r_t + gamma (1 - done_t) V_{t+1} - V_t: 9 bytes read + 8 written per sample
__global__ __launch_bounds__(256) void k_gae(const float *__restrict__ rew, const uint8_t *__restrict__ done,
                                             const float *__restrict__ val, float *__restrict__ adv,
                                             float *__restrict__ ret, int64_t n, int32_t T, float gamma, float lam,
                                             float rew_scale, double *__restrict__ partial) {
    gae_body<false>(rew, done, val, nullptr, adv, ret, n, T, gamma, lam, [=](float r, float v) { return fmaf(r, rew_scale, -v); }, partial);
}

// k_gae with the bootstrap term of truncated steps (rmav_gae_boot): boot_t = V(s_final) where the time limit ended the episode at
// step t (the state before the auto-reset; rmav_rollout_policy_boot leaves it), 0 elsewhere; the recursion still stops at every
// done.  13 bytes read + 8 written per sample.
__global__ __launch_bounds__(256) void k_gae_boot(const float *__restrict__ rew, const uint8_t *__restrict__ done,
                                                  const float *__restrict__ val, const float *__restrict__ boot,
                                                  float *__restrict__ adv, float *__restrict__ ret, int64_t n, int32_t T, float gamma,
                                                  float lam, float rew_scale, double *__restrict__ partial) {
    gae_body<true>(rew, done, val, boot, adv, ret, n, T, gamma, lam, [=](float r, float v) { return fmaf(r, rew_scale, -v); }, partial);
}

// one block: sums_out[0..1] = (sum A, sum A^2) over all blocks' partials
__global__ __launch_bounds__(256) void k_gae_fold(const double *__restrict__ partial, int nblocks, double *__restrict__ sums_out) {
    double a1 = 0.0, a2 = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += blockDim.x) {
        a1 += partial[2 * b];
        a2 += partial[2 * b + 1];
    }
    block_sum2(a1, a2, 4, sums_out);
}

// x <- (x - mean) * rstd, 16 bytes per lane, grid-stride; count4 = count / 4 full quads, the tail by scalar lanes
__global__ __launch_bounds__(256) void k_affine(float *__restrict__ x, int64_t count, float mean, float rstd) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n4 = count >> 2;
    float4 *x4 = reinterpret_cast<float4 *>(x);
    for (int64_t q = tid; q < n4; q += stride) {
        float4 v = x4[q];
        v.x = (v.x - mean) * rstd;
        v.y = (v.y - mean) * rstd;
        v.z = (v.z - mean) * rstd;
        v.w = (v.w - mean) * rstd;
        x4[q] = v;
    }
    for (int64_t q = (n4 << 2) + tid; q < count; q += stride) x[q] = (x[q] - mean) * rstd;
}

}  // namespace rmav

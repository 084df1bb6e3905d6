// rmav_optim.hpp - what a PPO minibatch does around the fused learner (rmav_learner.hpp / rmav_learner_shared.hpp), on the device:
// the advantage moments the learner takes as adv_norm (rmav_adv_moments) and the optimiser step on its flat gradient - scale, global
// norm, clip and Adam in one launch (rmav_ppo_adam).  include/rmav_ppo.h states both expressions; tests/optim_ref.py restates them.
//
// k_adv_moments / k_adv_moments_fold reuse the machinery of rmav_obs_norm.hpp as rmav_ret_norm.hpp does: per-lane sums of (x - K) and
// (x - K)^2 in fp64 (K = sample 0 for every lane: x - K is exact in fp64 for fp32 data), shifted_moment, block_chan, one Moment per
// workgroup in the caller's workspace, fold_partials in workgroup order.  Sample j sits in lane j mod 256 of workgroup (j / 256) mod
// groups, groups = min(ceil(batch / 256), kAdvMaxGroups), whether it came through idx or not, and a lane adds its samples in order:
// geometry and order depend on batch alone.
//
// k_ppo_adam is ONE workgroup (the largest layout is 10 825 floats): a workgroup can meet itself at a barrier, so the norm every
// element's update needs costs no second launch, no atomics and no grid-wide meeting point.  The tensors' pointers and the prefix
// offsets of the flat layout go by value (AdamArgs, as TrunkArgs); an element finds its tensor by an unrolled compare-and-select
// chain, never by indexing the argument struct with a runtime value (that would put it in scratch).
//
// Included by rmav_ppo_abi.hip alone, BEHIND rmav_obs_norm.hpp (Moment, shifted_moment, block_chan, fold_partials).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace rmav {

// ---- advantage moments --------------------------------------------------------------------------------------------------------------
constexpr int kAdvMaxGroups = 128;   // above 32 768 samples a lane adds more than one

inline int adv_groups(int64_t batch) {
    const int64_t tiles = (batch + 255) / 256;
    return (int)(tiles < kAdvMaxGroups ? tiles : kAdvMaxGroups);
}

// Stage 1.  partial [gridDim.x] moments of the samples adv[idx[j]] (idx null: adv[j]), j < batch.
__global__ __launch_bounds__(256) void k_adv_moments(const int64_t *__restrict__ idx, const float *__restrict__ adv, int64_t batch,
                                                     Moment *__restrict__ partial) {
    const double k0 = (double)adv[idx ? idx[0] : 0];   // the shift: the first sample (batch >= 1)
    const int64_t stride = (int64_t)gridDim.x * 256;
    double cnt = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll 4
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < batch; j += stride) {
        const double d = (double)adv[idx ? idx[j] : j] - k0;
        cnt += 1.0;
        s1 += d;
        s2 = fma(d, d, s2);
    }
    const Moment m = block_chan(shifted_moment(cnt, k0, s1, s2));
    if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

// Stage 2.  One block folds the partials; the last step is fp32, as the torch expression 1 / (std + 1e-8) on fp32 tensors is.
// batch = 1: m2 / 0 = NaN, as torch.std_mean gives.
__global__ __launch_bounds__(256) void k_adv_moments_fold(const Moment *__restrict__ partial, int32_t nblk, int64_t batch,
                                                          float *__restrict__ out) {
    const Moment m = fold_partials(partial, nblk);
    if (threadIdx.x == 0) {
        const float std = (float)sqrt(m.m2 / (double)(batch - 1));
        out[0] = (float)m.mean;
        out[1] = 1.0f / (std + 1e-8f);
    }
}

// ---- norm clip + Adam ---------------------------------------------------------------------------------------------------------------
constexpr int kAdamThreads = 1024;
constexpr int kAdamMaxTensors = 13;   // rmav_ppo_grad's layout; rmav_ppo_grad_shared's has 9

struct AdamArgs {
    const float *grad;               // [n], read only
    float *m, *v;                    // exp_avg, exp_avg_sq [n]
    float *stats;                    // (norm, coef) or null
    float *p[kAdamMaxTensors];       // the parameter tensors; unused slots null
    int32_t off[kAdamMaxTensors];    // first flat index of tensor k; unused slots INT32_MAX (never selected)
    int32_t n;
    float grad_scale, max_norm;
    float omb1, beta2, omb2;         // 1 - beta1, beta2, 1 - beta2 (the differences taken in fp32 on the host)
    float step_size, bc2_sqrt, eps;  // (float)(lr / (1 - beta1^step)), (float)sqrt(1 - beta2^step): fp64 on the host, rounded once
};

// THE arithmetic, fp32 and uncontracted unless marked, one line per operation (include/rmav_ppo.h restates it)
__global__ __launch_bounds__(kAdamThreads) void k_ppo_adam(const AdamArgs A) {
    __shared__ double wave_sum[kAdamThreads / 64];
    const int t = threadIdx.x;
    // ---- sum g^2 over the flat buffer: strided per-thread partials in fp64, wavefronts by shuffle, the 16 wavefront sums in order ----
    double acc = 0.0;
    for (int32_t i = t; i < A.n; i += kAdamThreads) {
        const double g = (double)(A.grad[i] * A.grad_scale);
        acc = fma(g, g, acc);   // (g * g is exact in fp64)
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((t & 63) == 0) wave_sum[t >> 6] = acc;
    __syncthreads();
    double total = 0.0;
#pragma unroll
    for (int w = 0; w < kAdamThreads / 64; ++w) total += wave_sum[w];   // every thread, the same order: the same bits
    const float norm = (float)sqrt(total);
    const float ratio = A.max_norm / (norm + 1e-6f);
    const float coef = ratio >= 1.0f ? 1.0f : ratio;   // min(1, ratio) that keeps a NaN, as torch.clamp(max=1) does
    if (t == 0 && A.stats) {
        A.stats[0] = norm;
        A.stats[1] = coef;
    }
    // ---- the update, one element per thread and pass ---------------------------------------------------------------------------------
    for (int32_t i = t; i < A.n; i += kAdamThreads) {
        float *base = A.p[0];
        int32_t first = 0;
#pragma unroll
        for (int k = 1; k < kAdamMaxTensors; ++k) {
            const bool in = i >= A.off[k];
            base = in ? A.p[k] : base;
            first = in ? A.off[k] : first;
        }
        float *p = base + (i - first);
        const float g = A.grad[i] * A.grad_scale;
        const float gh = g * coef;
        float m = A.m[i], v = A.v[i];
        const float d = gh - m;
        const float td = A.omb1 * d;
        m = m + td;
        const float a = A.beta2 * v;
        const float b = gh * gh;
        const float c = A.omb2 * b;
        v = a + c;
        const float s = sqrtf(v);
        const float q = s / A.bc2_sqrt;
        const float den = q + A.eps;
        const float r = m / den;
        const float u = A.step_size * r;
        A.m[i] = m;
        A.v[i] = v;
        *p = *p - u;
    }
}

}  // namespace rmav

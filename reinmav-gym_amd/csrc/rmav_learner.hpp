// rmav_learner.hpp - the fused PPO learner (rmav_ppo_grad, include/rmav_ppo.h): clipped-surrogate loss of one minibatch and its
// gradient with respect to every parameter of an MlpPolicy(value_network="copy", hidden=64), in fp32: one launch per net plus a fold.
//
// What torch does per minibatch (ppo.py: PPO.loss + backward) is ~40 passes over [64][B] fp32 intermediates.  Here a workgroup walks
// tiles of 64 samples; the activations, the deltas and the weights of the net at hand live in LDS, the weight-gradient accumulators in
// registers across all of the workgroup's tiles, and nothing but the inputs ((nS + nA + 4) floats per sample) is read from HBM.
//
// VARIANT BUILT: every product runs on the vector ALU from LDS; the matrix-core path (mlp_mfma32's layout forward and backward, the
// sample index as K for the weight gradients) is not built.  DESIGN.md section 4 and profiles/r23/learner.md say what this one measures.  All five layers of work have the same shape, a [64 x K] . [K x 64]
// product whose output a thread owns as a 4 x 4 register block fed by two 16-byte LDS reads per 16 FMAs:
//     forward     H  = tanh(W . IN + b)            K = inputs,  operands  W^T [k][row]  and  IN [k][sample]
//     backward    D' = (W^T . D) * (1 - H^2)       K = 64,      operands  W   [k][row]  and  D  [k][sample]
//     gradients   dW = D . IN^T                    K = samples, operands  D [row][s] and IN [row][s]  (both read along s)
// The nets run one after the other (policy, then value; one launch each: both nets' pointers in one kernel spilled scalar registers): a net's weights (W1^T, W2^T, W2, W3, biases: 38 KB) are staged once per
// workgroup, and the observation tile is loaded once per net (nS floats per sample, against ~16 k FMAs per sample and net).
//
// LDS rows have a pitch of 68 floats and a thread owns the rows {rb + 16 r} (r = 0..3) of a 64-row operand, not four consecutive
// ones: the 16 row addresses a quarter-wavefront reads then fall 4 banks apart (68 k mod 64 = 4 k) - no conflict on the 16-byte reads
// along s.  The weights are stored with column pos(j) = 4 (j mod 16) + j / 16, which makes those four rows one 16-byte read.
//
// DETERMINISM: no atomics.  Sample j sits in lane j mod 64 of tile j / 64 whether it came through idx or not; tile t belongs to
// workgroup t mod groups with groups = min(tiles, kLrnMaxGroups); a thread adds its tiles in order; per-workgroup partials go to the
// caller's workspace and k_learner_fold adds them in workgroup order.  Geometry and order depend on (kind, batch) alone.
// Tail lanes of the last tile read a valid column (the last sample's) and get delta = 0, so they add exact zeros.
//
// The statements learner_net shares with k_trunk_grad (rmav_learner_shared.hpp) are text fragments both include, rmav_learner_stage.inc,
// _fwd.inc, _pg.inc, _vf.inc and _bwd.inc: as inline functions they changed the ISA of both.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace rmav {

constexpr int kLrnTile = 64;         // samples per tile
constexpr int kLrnPitch = 68;        // LDS row pitch of the activation tiles (floats)
constexpr int kLrnThreads = 256;
constexpr int kLrnMaxGroups = 512;   // two workgroups per CU
constexpr int kLrnParams = 13;       // pi: W1 b1 W2 b2 W3 b3 | vf: the same six | logstd
constexpr int kLrnStats = 4;         // a workgroup's partial record behind its gradient: sum pg, sum vf, max ratio, pad

// (the flat gradient's layout, the ABI order of include/rmav_ppo.h, is host code: flat_layout in rmav_ppo_abi.hip)
inline int learner_groups(int64_t batch) {
    const int64_t tiles = (batch + kLrnTile - 1) / kLrnTile;
    return (int)(tiles < kLrnMaxGroups ? tiles : kLrnMaxGroups);
}

// The arguments of ONE net's launch (k_learner_grad<VALUE>): the net's six parameters and where their gradients go
struct LearnerArgs {
    const int64_t *idx;       // [batch] or null
    const float *obs, *act;   // [ns][obs_pitch], [na][act_pitch]
    int64_t obs_pitch, act_pitch;
    const float *logp_old, *val_old, *adv, *ret;
    const float *adv_norm;    // (mean, 1 / (std + 1e-8)) on the device
    const float *norm_tab;    // mean_f [16] | rstd_f [16] | clip_f of an observation-statistics buffer, or null
    float *partial;           // [groups][pstride]
    float clip, vf_coef;
    int32_t batch, ns, na, pstride;
    const float *p[6];        // W1 b1 W2 b2 W3 b3 of the net
    const float *logstd;
    int32_t goff[6];          // offsets of their gradients in a workgroup's partial record
    int32_t off_logstd, off_stats;
};

struct alignas(16) LearnerLds {
    float x[16 * kLrnPitch];
    float h1[64 * kLrnPitch];    // tanh of layer 1, later delta 1 in place
    float h2[64 * kLrnPitch];    // tanh of layer 2, later delta 2 in place
    float w2t[64 * 64];          // [k = input][pos(output)]
    float w2n[64 * 64];          // [k = output][pos(input)]
    float w1t[16 * 64];          // [k = input][pos(output)], rows >= ns zero
    float w3[4 * 64];            // [output][k], rows >= n_out zero
    float b1[64], b2[64], b3[4];
    float logstd[4];
    float out[4 * kLrnTile];     // [output][sample]
    float d3[4 * kLrnTile];      // delta of the output layer, rows >= n_out zero
};
static_assert(sizeof(LearnerLds) <= 80 * 1024, "two workgroups per CU");

__device__ __forceinline__ int lrn_pos(int j) { return 4 * (j & 15) + (j >> 4); }
__device__ __forceinline__ float4 lds4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

// acc[r][q] += sum_k a[k][4 rb + r] * b[k][4 cb + q]: a with row pitch 64 (pos-ordered weights), b with the tile pitch
__device__ __forceinline__ void lrn_gemm(const float *__restrict__ a, const float *__restrict__ b, int K, int rb, int cb, float (&acc)[4][4]) {
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
        const float4 w = lds4(a + k * 64 + 4 * rb), v = lds4(b + k * kLrnPitch + 4 * cb);
        const float wr[4] = {w.x, w.y, w.z, w.w}, vq[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[r][q] = fmaf(wr[r], vq[q], acc[r][q]);
    }
}

// One net of the learner over this workgroup's tiles.  VALUE = false: the policy net (n_out = na; loss terms pg, logstd), true: the
// value net (n_out = 1; loss term vf).  p: the net's six parameter pointers, goff: offsets of its six gradients in the flat layout.
template <bool VALUE>
__device__ __forceinline__ void learner_net(const LearnerArgs &A, LearnerLds &S, float *__restrict__ part) {
    const float *const *p = A.p;
    const int32_t *goff = A.goff;
    const int t = threadIdx.x, rb = t >> 4, cb = t & 15;
    const int ns = A.ns, n_out = VALUE ? 1 : A.na;
    // ---- stage the net's weights ------------------------------------------------------------------------------------------------------
#include "rmav_learner_stage.inc"
    {
        const int o = t >> 6, k = t & 63;
        S.w3[t] = o < n_out ? p[4][o * 64 + k] : 0.0f;
        S.d3[t] = 0.0f;
        if (t < 64) {
            S.b1[t] = p[1][t];
            S.b2[t] = p[3][t];
        }
        if (t < 4) {
            S.b3[t] = t < n_out ? p[5][t] : 0.0f;
            S.logstd[t] = t < A.na ? A.logstd[t] : 0.0f;
        }
    }
    __syncthreads();

    float g2[4][4] = {}, g1[4] = {}, g3 = 0.0f, gb2[4] = {}, gb1[4] = {};   // this thread's share of dW2, dW1, dW3, db2, db1
    // per-sample lane (wave 0): db3, dlogstd, the loss sums (one of the two per net: two names, since the policy and the value term
    // are shared text, rmav_learner_pg.inc and rmav_learner_vf.inc)
    float gb3[4] = {}, gls[4] = {}, sum_pg = 0.0f, sum_vf = 0.0f, max_ratio = 0.0f;
    const float inv_b = 1.0f / (float)A.batch;
    const int64_t tiles = ((int64_t)A.batch + kLrnTile - 1) / kLrnTile;

    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
#include "rmav_learner_fwd.inc"
        {   // output layer: thread (o, s), wavefront-uniform o
            const int o = t >> 6;
            if (o < n_out) {
                float acc = S.b3[o];
#pragma unroll 8
                for (int k = 0; k < 64; ++k) acc = fmaf(S.w3[o * 64 + k], S.h2[k * kLrnPitch + s], acc);
                S.out[o * kLrnTile + s] = acc;
            }
        }
        __syncthreads();
        // ---- the loss of sample s and the delta of the output layer (wave 0) ----------------------------------------------------------
        if (t < 64) {
            if constexpr (!VALUE) {
                const int na = A.na;
#include "rmav_learner_pg.inc"
            } else {
                constexpr int vrow = 0;   // the value net's one output row, and its bias gradient
                float &gbv = gb3[0];
#include "rmav_learner_vf.inc"
            }
        }
        __syncthreads();
        // ---- dW3 += d3 . h2^T: thread (o, k) ------------------------------------------------------------------------------------------
        {
            const int o = t >> 6, k = t & 63;
            if (o < n_out) {
                for (int s4 = 0; s4 < kLrnTile; s4 += 4) {
                    const float4 d = lds4(&S.d3[o * kLrnTile + s4]), h = lds4(&S.h2[k * kLrnPitch + s4]);
                    g3 = fmaf(d.x, h.x, g3);
                    g3 = fmaf(d.y, h.y, g3);
                    g3 = fmaf(d.z, h.z, g3);
                    g3 = fmaf(d.w, h.w, g3);
                }
            }
        }
        __syncthreads();
        // ---- delta 2 = (W3^T d3) * (1 - h2^2), in place ------------------------------------------------------------------------------
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = rb + 16 * r;
            float4 *hp = reinterpret_cast<float4 *>(&S.h2[row * kLrnPitch + 4 * cb]);
            const float4 h = *hp;
            float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                const float w = S.w3[o * 64 + row];
                const float4 d = lds4(&S.d3[o * kLrnTile + 4 * cb]);
                g[0] = fmaf(w, d.x, g[0]);
                g[1] = fmaf(w, d.y, g[1]);
                g[2] = fmaf(w, d.z, g[2]);
                g[3] = fmaf(w, d.w, g[3]);
            }
            const float4 dl = make_float4(g[0] * fmaf(-h.x, h.x, 1.0f), g[1] * fmaf(-h.y, h.y, 1.0f), g[2] * fmaf(-h.z, h.z, 1.0f),
                                          g[3] * fmaf(-h.w, h.w, 1.0f));
            *hp = dl;
            gb2[r] += (dl.x + dl.y) + (dl.z + dl.w);
        }
        __syncthreads();
#include "rmav_learner_bwd.inc"
    }

    // ---- this workgroup's partial gradient of the net ---------------------------------------------------------------------------------
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int c = 0; c < 4; ++c) part[goff[2] + (rb + 16 * r) * 64 + cb + 16 * c] = g2[r][c];
        if (cb < ns) part[goff[0] + (rb + 16 * r) * ns + cb] = g1[r];
    }
    if ((t >> 6) < n_out) part[goff[4] + t] = g3;
    // the bias sums of the 16 threads that share a row, and of the 64 sample lanes, through LDS in a fixed order (h2 is free now)
    float *red = S.h2;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        red[(rb + 16 * r) * 16 + cb] = gb2[r];
        red[1024 + (rb + 16 * r) * 16 + cb] = gb1[r];
    }
    if (t < 64) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            red[2048 + c * 64 + t] = gb3[c];
            red[2048 + (4 + c) * 64 + t] = gls[c];
        }
        red[2048 + 8 * 64 + t] = VALUE ? sum_vf : sum_pg;
        red[2048 + 9 * 64 + t] = max_ratio;
    }
    __syncthreads();
    if (t < 128) {   // db2 (t < 64), db1
        const float *src = red + 16 * t;
        float acc = 0.0f;
        for (int k = 0; k < 16; ++k) acc += src[k];
        part[goff[t < 64 ? 3 : 1] + (t & 63)] = acc;
    } else if (t < 128 + 10) {
        const int q = t - 128;   // 0..3 db3, 4..7 dlogstd, 8 the loss sum, 9 the largest ratio
        const float *src = red + 2048 + 64 * q;
        float acc = 0.0f;
        for (int k = 0; k < 64; ++k) acc = q == 9 ? fmaxf(acc, src[k]) : acc + src[k];
        if (q < 4) {
            if (q < n_out) part[goff[5] + q] = acc;
        } else if (q < 8) {
            if (!VALUE && q - 4 < A.na) part[A.off_logstd + q - 4] = acc;
        } else if (q == 8) {
            part[A.off_stats + (VALUE ? 1 : 0)] = acc;
        } else if (!VALUE) {
            part[A.off_stats + 2] = acc;
        }
    }
}

// VALUE = false: the policy net (its gradients, dlogstd, sum pg and max ratio of the workgroup's samples), true: the value net (its
// gradients and sum vf).  Two launches with the same geometry fill disjoint parts of the same partial records.
template <bool VALUE>
__global__ __launch_bounds__(kLrnThreads) void k_learner_grad(const LearnerArgs A) {
    __shared__ LearnerLds S;
    learner_net<VALUE>(A, S, A.partial + (int64_t)blockIdx.x * A.pstride);
}

// grad_out[p] = sum over the workgroups' partials in workgroup order (- ent_coef on logstd); block 0 also folds the statistics:
// stats_out = loss, pg, vf, max ratio
__global__ __launch_bounds__(256) void k_learner_fold(const float *__restrict__ partial, int32_t groups, int32_t pstride, int32_t n_params,
                                                      int32_t off_logstd, int32_t na, int32_t batch, float vf_coef, float ent_coef,
                                                      const float *__restrict__ logstd, float *__restrict__ grad_out,
                                                      float *__restrict__ stats_out) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < n_params) {
        float acc = 0.0f;
        for (int g = 0; g < groups; ++g) acc += partial[(int64_t)g * pstride + p];
        if (p >= off_logstd) acc -= ent_coef;
        grad_out[p] = acc;
    }
    if (blockIdx.x != 0) return;   // uniform
    __shared__ float sh[3][256];
    float pg = 0.0f, vf = 0.0f, rmax = 0.0f;
    for (int g = threadIdx.x; g < groups; g += 256) {
        const float *rec = partial + (int64_t)g * pstride + n_params;
        pg += rec[0];
        vf += rec[1];
        rmax = fmaxf(rmax, rec[2]);
    }
    sh[0][threadIdx.x] = pg;
    sh[1][threadIdx.x] = vf;
    sh[2][threadIdx.x] = rmax;
    __syncthreads();
    if (threadIdx.x == 0) {
        pg = vf = rmax = 0.0f;
        for (int k = 0; k < 256; ++k) {
            pg += sh[0][k];
            vf += sh[1][k];
            rmax = fmaxf(rmax, sh[2][k]);
        }
        const float inv_b = 1.0f / (float)batch;
        pg *= inv_b;
        vf = 0.5f * vf * inv_b;
        float ent = 0.0f;
        for (int c = 0; c < na; ++c) ent += logstd[c] + 1.4189385332046727f;   // log(2 pi e) / 2
        stats_out[0] = pg + vf_coef * vf - ent_coef * ent;
        stats_out[1] = pg;
        stats_out[2] = vf;
        stats_out[3] = rmax;
    }
}

}  // namespace rmav

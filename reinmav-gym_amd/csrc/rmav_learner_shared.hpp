// rmav_learner_shared.hpp - the fused PPO learner of the shared-trunk policy (rmav_ppo_grad_shared, include/rmav_ppo.h): clipped-
// surrogate loss of one minibatch and its gradient with respect to every parameter of an MlpPolicy(value_network="shared", hidden=64),
// in fp32: ONE net launch plus the fold of rmav_learner.hpp.
//
// The policy is one 2 x 64 tanh trunk with two heads on its latent h2: the mean head pi.2 (nA rows) and the scalar value head vf.0.
// k_trunk_grad is learner_net (rmav_learner.hpp) with an output layer of nA + 1 rows - rows 0 .. nA-1 the mean head, row nA the value
// head - and both loss terms in one pass: the tile walk, the LDS pitch (68), the pos() weight order, the 4 x 4 register blocks, the
// fixed-order bias reductions and the per-sample-lane quantities are the copy kernel's.  What differs:
//     one trunk     the weights are staged once, the observation tile is loaded and normalised once, layers 1 and 2 run forward once
//     two heads     wave 0 computes the policy term AND the value term of sample s and both output deltas (the expressions,
//                   sub-gradient rules and `live` masking of learner_net<false> and learner_net<true>)
//     summed delta  delta 2 = (W3^T d_mean + w_v d_v) * (1 - h2^2): the trunk gets the sum of both heads' deltas, the value head's
//                   carrying vf_coef; delta 1, dW2, dW1 and the bias sums follow from it as in the copy kernel
// Up to five output rows: four map onto the four wavefronts (o = t >> 6) as in the copy kernel, the fifth (quad3d, quad3d_sl, reinmav:
// the value row) gets a pass of its own on wave 0.  A workgroup writes one partial record of n_params + 4 floats (statistics words:
// sum pg, sum vf, max ratio, pad) and k_learner_fold, unchanged, adds the records: it is generic in n_params / off_logstd, and logstd
// stays last.  Every product runs on the vector ALU from LDS; no matrix instruction, no atomics.
//
// DETERMINISM: the paragraph of rmav_learner.hpp holds word for word (same tile walk, same partial records, same fold).
//
// Included by rmav_ppo_abi.hip alone, BEHIND rmav_learner.hpp: lrn_gemm, lrn_pos, lds4, learner_groups, k_learner_fold and the
// constants are that header's (it has one includer, which tests/test_learner_build.py counts, so this file does not include it).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace rmav {

constexpr int kTrkParams = 9;   // pi.W1 pi.b1 pi.W2 pi.b2 pi.W3 pi.b3 | vf.W vf.b | logstd
constexpr int kTrkRows = 5;     // output rows held in LDS: at most 4 means + the value

// The kernel derives the offsets of the flat gradient (flat_layout in rmav_ppo_abi.hip) from (ns, na) when it writes its record: nine
// offsets as kernel arguments would sit in scalar registers across the tile loop.
struct TrunkArgs {
    const int64_t *idx;       // [batch] or null
    const float *obs, *act;   // [ns][obs_pitch], [na][act_pitch]
    int64_t obs_pitch, act_pitch;
    const float *logp_old, *val_old, *adv, *ret;
    const float *adv_norm;    // (mean, 1 / (std + 1e-8)) on the device
    const float *norm_tab;    // mean_f [16] | rstd_f [16] | clip_f of an observation-statistics buffer, or null
    float *partial;           // [groups][n_params + kLrnStats]
    float clip, vf_coef;
    int32_t batch, ns, na;
    const float *p[kTrkParams];
};

struct alignas(16) TrunkLds {
    float x[16 * kLrnPitch];
    float h1[64 * kLrnPitch];    // tanh of layer 1, later delta 1 in place
    float h2[64 * kLrnPitch];    // tanh of layer 2, later delta 2 in place
    float w2t[64 * 64];          // [k = input][pos(output)]
    float w2n[64 * 64];          // [k = output][pos(input)]
    float w1t[16 * 64];          // [k = input][pos(output)], rows >= ns zero
    float w3[kTrkRows * 64];     // [output][k]: the mean head, then the value head; rows > na zero
    float out[kTrkRows * kLrnTile];   // [output][sample]
    float d3[kTrkRows * kLrnTile];    // delta of the output layer, rows > na zero
    float b1[64], b2[64];
    float logstd[4];
    float b3[kTrkRows];
};
static_assert(sizeof(TrunkLds) <= 80 * 1024, "two workgroups per CU");

__global__ __launch_bounds__(kLrnThreads) void k_trunk_grad(const TrunkArgs A) {
    __shared__ TrunkLds S;
    const int t = threadIdx.x, rb = t >> 4, cb = t & 15;
    const int ns = A.ns, na = A.na, n_out = na + 1;
    const float *const *p = A.p;
    // ---- stage the trunk and both heads -------------------------------------------------------------------------------------------------
#include "rmav_learner_stage.inc"
    for (int e = t; e < kTrkRows * 64; e += kLrnThreads) {
        const int o = e >> 6, k = e & 63;
        S.w3[e] = o < na ? A.p[4][o * 64 + k] : (o == na ? A.p[6][k] : 0.0f);
        S.d3[e] = 0.0f;
    }
    if (t < 64) {
        S.b1[t] = A.p[1][t];
        S.b2[t] = A.p[3][t];
    }
    if (t < kTrkRows) S.b3[t] = t < na ? A.p[5][t] : (t == na ? A.p[7][0] : 0.0f);
    if (t < 4) S.logstd[t] = t < na ? A.p[8][t] : 0.0f;
    __syncthreads();

    float g2[4][4] = {}, g1[4] = {}, gb2[4] = {}, gb1[4] = {};   // this thread's share of dW2, dW1, db2, db1
    float g3 = 0.0f, g3x = 0.0f;                                 // ... of dW3: row t >> 6, and (wave 0) row 4
    // per-sample lane (wave 0): db3 of the mean head, db of the value head (its own scalar: a register array indexed by na costs a
    // mask per row, and those spilled scalar registers), dlogstd, the loss sums
    float gb3[4] = {}, gbv = 0.0f, gls[4] = {}, sum_pg = 0.0f, sum_vf = 0.0f, max_ratio = 0.0f;
    const float inv_b = 1.0f / (float)A.batch;
    const int64_t tiles = ((int64_t)A.batch + kLrnTile - 1) / kLrnTile;

    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
#include "rmav_learner_fwd.inc"
        // ---- the output layer: thread (o, s), wavefront-uniform o; the fifth row is wave 0's second pass -----------------------------
        for (int o = t >> 6; o < n_out; o += 4) {
            float acc = S.b3[o];
#pragma unroll 8
            for (int k = 0; k < 64; ++k) acc = fmaf(S.w3[o * 64 + k], S.h2[k * kLrnPitch + s], acc);
            S.out[o * kLrnTile + s] = acc;
        }
        __syncthreads();
        // ---- both loss terms of sample s and the deltas of both heads (wave 0) -------------------------------------------------------
        if (t < 64) {
            {   // the policy term: learner_net<false>
#include "rmav_learner_pg.inc"
            }
            {   // the value term: learner_net<true>, on row na
                const int vrow = na;
#include "rmav_learner_vf.inc"
            }
        }
        __syncthreads();
        // ---- dW3 += d3 . h2^T: thread (o, k); row 4 on wave 0 -------------------------------------------------------------------------
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
            if (o + 4 < n_out) {
                for (int s4 = 0; s4 < kLrnTile; s4 += 4) {
                    const float4 d = lds4(&S.d3[4 * kLrnTile + s4]), h = lds4(&S.h2[k * kLrnPitch + s4]);
                    g3x = fmaf(d.x, h.x, g3x);
                    g3x = fmaf(d.y, h.y, g3x);
                    g3x = fmaf(d.z, h.z, g3x);
                    g3x = fmaf(d.w, h.w, g3x);
                }
            }
        }
        __syncthreads();
        // ---- delta 2 = (W3^T d_mean + w_v d_v) * (1 - h2^2), in place: the sum over all output rows (rows > na are zero) -----------
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = rb + 16 * r;
            float4 *hp = reinterpret_cast<float4 *>(&S.h2[row * kLrnPitch + 4 * cb]);
            const float4 h = *hp;
            float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int o = 0; o < kTrkRows; ++o) {
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

    // ---- this workgroup's partial record: offsets of the flat layout from (ns, na) ------------------------------------------------------
    const int off_b1 = 64 * ns, off_w2 = off_b1 + 64, off_b2 = off_w2 + 64 * 64, off_w3 = off_b2 + 64, off_b3 = off_w3 + 64 * na;
    const int off_wv = off_b3 + na, off_bv = off_wv + 64, off_logstd = off_bv + 1, off_stats = off_logstd + na;
    float *__restrict__ part = A.partial + (int64_t)blockIdx.x * (off_stats + kLrnStats);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int c = 0; c < 4; ++c) part[off_w2 + (rb + 16 * r) * 64 + cb + 16 * c] = g2[r][c];
        if (cb < ns) part[(rb + 16 * r) * ns + cb] = g1[r];
    }
    {
        const int o = t >> 6, k = t & 63;
        if (o < na) part[off_w3 + t] = g3;
        else if (o == na) part[off_wv + k] = g3;
        if (o + 4 == na) part[off_wv + k] = g3x;
    }
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
            red[2048 + (kTrkRows + c) * 64 + t] = gls[c];
        }
        red[2048 + 4 * 64 + t] = gbv;
        red[2048 + 9 * 64 + t] = sum_pg;
        red[2048 + 10 * 64 + t] = sum_vf;
        red[2048 + 11 * 64 + t] = max_ratio;
    }
    __syncthreads();
    if (t < 128) {   // db2 (t < 64), db1
        const float *src = red + 16 * t;
        float acc = 0.0f;
        for (int k = 0; k < 16; ++k) acc += src[k];
        part[(t < 64 ? off_b2 : off_b1) + (t & 63)] = acc;
    } else if (t < 128 + 12) {
        const int q = t - 128;   // 0..3 db3 of the mean head, 4 db of the value head, 5..8 dlogstd, 9 sum pg, 10 sum vf, 11 the largest ratio
        const float *src = red + 2048 + 64 * q;
        float acc = 0.0f;
        for (int k = 0; k < 64; ++k) acc = q == 11 ? fmaxf(acc, src[k]) : acc + src[k];
        if (q < 4) {
            if (q < na) part[off_b3 + q] = acc;
        } else if (q == 4) {
            part[off_bv] = acc;
        } else if (q < 9) {
            if (q - kTrkRows < na) part[off_logstd + q - kTrkRows] = acc;
        } else {
            part[off_stats + q - 9] = acc;
        }
    }
}

}  // namespace rmav

// rmav_learner_mfma.hpp - the fused PPO learner of the shared-trunk policy on the fp32 matrix cores (rmav_ppo_grad_shared_mfma,
// include/rmav_ppo.h): the loss of k_trunk_grad (rmav_learner_shared.hpp) and its gradient with respect to the same 9 tensors, in the
// same partial-record format, with every [64 x K] . [K x samples] product and every weight gradient on v_mfma_f32_32x32x2_f32.  That
// instruction is bit for bit a k-ordered fmaf chain, so the result stays in the precision class of the vector-ALU learner; only the
// order of summation differs.
//
// GEOMETRY.  A wavefront owns a tile of 32 samples: lane (n = l & 31, h = l >> 5) is sample column n.  A workgroup is 4 wavefronts =
// one STEP of 128 samples; step s belongs to workgroup s mod groups, groups = min(steps, kMatMaxGroups), and inside a step tile w is
// wavefront w's.  LDS: the staged weights (38.7 KB per workgroup) and per wavefront two [64 units][32 + 4] transposition tiles, the
// observation tile and the output deltas (21.5 KB): 124.5 KB, one workgroup per CU, one wavefront per SIMD (a second one does not
// overlap with fp32 MFMA: rmav_policy_mfma32.hpp).
//
// FORWARD (the scheme of rmav_policy_mfma32.hpp).  Weights are the A operand, activations the B operand; accumulator register r of row
// tile T holds unit 32 T + row(r, h), row(r, h) = (r & 3) + 8 (r >> 2) + 4 h, of column n, which after tanhf IS the B operand of slice
// (T, r) of the next layer.  The A layouts are built while staging from the raw torch tensors:
//     layer 1, slice s:         lane (m, h) holds W1[32 T + m][2 s + h], zero beyond nS
//     layer 2, slice (Tin, r):  lane (m, h) holds W2[32 To + m][32 Tin + row(r, h)]
// The output layer (rows 0..3 the mean head, zero beyond nA; row 4 the value head) runs on the vector ALU: a lane forms the dot product
// over the 32 units it holds and exchanges it with lane l ^ 32 (v_permlane32_swap), the h = 0 half added first in both lanes - both
// half-lanes of a column then hold mean, v and the output deltas of their sample, bit for bit the same.
//
// BACKWARD.  delta 2 = (W3'^T d3) * (1 - h2^2) elementwise in accumulator layout (5 FMAs per register); delta 1 = (W2^T delta 2) *
// (1 - h1^2) is 64 matrix instructions whose A operand, slice (Tj, r), is lane (m, h) = W2[32 Tj + row(r, h)][32 Ti + m] and whose B
// operand is delta 2's accumulator register r.
//
// WEIGHT GRADIENTS.  The sample index is K, so the operands are wanted unit-per-lane: a wavefront writes h1, h2, delta 2, delta 1, x
// and d3 to its LDS tiles as [unit][32 samples + 4] and lane (m, h) reads samples 16 h .. 16 h + 15 of unit m back in four 16-byte
// reads.  Slice q pairs sample q (k = 0) with sample 16 + q (k = 1) in both operands.  dW2: 2 x 2 tiles x 16 slices, dW1: 2 x 16 (B
// columns beyond nS zero), dW3': 2 x 16 (A rows beyond the five output rows zero); db1 / db2 are the lane's sums of the 16 values it
// has just read.  Two unit tiles serve four quantities: h2's is overwritten by delta 2 once dW3' has read it, h1's by delta 1 once dW2
// has.  The 128 accumulator registers persist across the wavefront's tiles; at the end the four wavefronts' accumulators are added
// through LDS in wavefront order into the workgroup's ONE record, which k_learner_fold (rmav_learner.hpp) folds unchanged.
//
// The loss term restates rmav_learner_pg.inc / rmav_learner_vf.inc on registers (those fragments read S.out / write S.d3 and belong to
// the two vector-ALU headers): the same fp32 expressions, sub-gradient rules, `live` masking, tanhf / expf and normalisation clamp.
//
// DETERMINISM: no atomics.  Sample j sits in lane j mod 32 of wavefront (j / 32) mod 4 of step j / 128 whether it came through idx or
// not; a wavefront adds its tiles in order; the record is the wavefronts' sum in wavefront order; the fold adds the records in
// workgroup order.  Geometry and order depend on (kind, batch) alone.  A lane beyond batch - a whole wavefront of them included -
// reads the last sample's column and gets d3 = 0, so it adds exact zeros.
//
// Included by rmav_ppo_abi.hip alone, BEHIND rmav_learner_shared.hpp: TrunkArgs, kTrkRows, kLrnStats and k_learner_fold are the
// learner headers', f32x16_t, bias_frag and xor32 rmav_policy_mfma.hpp's (the unit's ladder header brings it).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace rmav {

constexpr int kMatTile = 32;          // samples per wavefront tile
constexpr int kMatStep = 128;         // samples per workgroup step: 4 wavefront tiles
constexpr int kMatThreads = 256;
constexpr int kMatMaxGroups = 256;    // one workgroup per CU
constexpr int kMatPitch = 36;         // row pitch of the transposition tiles (floats): 16-byte rows

inline int matrix_groups(int64_t batch) {
    const int64_t steps = (batch + kMatStep - 1) / kMatStep;
    return (int)(steps < kMatMaxGroups ? steps : kMatMaxGroups);
}

// float offsets inside the kernel's LDS
struct MatLayout {
    static constexpr int A1 = 0;                 // [T 2][sq 2][lane 64][4]: layer-1 slices 4 sq .. 4 sq + 3 of the lane
    static constexpr int A2 = A1 + 1024;         // [To 2][Tin 2][rq 4][lane 64][4]: layer 2
    static constexpr int A2T = A2 + 4096;        // [Ti 2][Tj 2][rq 4][lane 64][4]: W2^T for delta 1
    static constexpr int W3 = A2T + 4096;        // [h 2][output 5][Tin 2][r 16]: the heads' rows over the units lane half h holds
    static constexpr int B1 = W3 + 2 * kTrkRows * 32;
    static constexpr int B2 = B1 + 64;
    static constexpr int B3 = B2 + 64;           // [5] (+ 3 pad)
    static constexpr int LOGSTD = B3 + 8;        // [4] (+ 4 pad)
    static constexpr int WAVE = LOGSTD + 8;      // the four wavefronts' tiles
    // ... inside a wavefront's tiles
    static constexpr int HA = 0;                               // [64][pitch]: h1, later delta 1
    static constexpr int HB = HA + 64 * kMatPitch;             // [64][pitch]: h2, later delta 2
    static constexpr int X = HB + 64 * kMatPitch;              // [16][pitch]: the observations, rows >= nS zero
    static constexpr int D3 = X + 16 * kMatPitch;              // [5][pitch]: the output deltas
    static constexpr int WAVE_FLOATS = D3 + kTrkRows * kMatPitch;
    static constexpr int TOTAL = WAVE + 4 * WAVE_FLOATS;
};
static_assert(MatLayout::WAVE % 4 == 0 && MatLayout::WAVE_FLOATS % 4 == 0, "16-byte tiles");
static_assert(MatLayout::TOTAL * sizeof(float) <= 160 * 1024, "one workgroup per CU");
static_assert(MatLayout::TOTAL >= 4 * 1024, "the end-of-kernel sums reuse the front of the LDS: 4 wavefronts x 16 registers x 64 lanes");

__device__ __forceinline__ int mat_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// tile[(32 T + row(r, h))][n] = acc[T][r]: the accumulator layout, transposed to unit-per-row
__device__ __forceinline__ void mat_put(float *tile, const f32x16_t (&acc)[2], int n, int h) {
#pragma unroll
    for (int T = 0; T < 2; ++T)
#pragma unroll
        for (int r = 0; r < 16; ++r) tile[(32 * T + mat_row(r, h)) * kMatPitch + n] = acc[T][r];
}

// samples 16 h .. 16 h + 15 of one row of a tile -> v[16]; returns their sum in a fixed order
__device__ __forceinline__ float mat_get(const float *row16, float (&v)[16]) {
    float sum = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 a = *reinterpret_cast<const float4 *>(row16 + 4 * q);
        v[4 * q + 0] = a.x; v[4 * q + 1] = a.y; v[4 * q + 2] = a.z; v[4 * q + 3] = a.w;
        sum += (a.x + a.y) + (a.z + a.w);
    }
    return sum;
}

__device__ __forceinline__ void mat_zero(float (&v)[16]) {
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = 0.0f;
}

// acc += A . B over the 32 samples: slice q pairs sample q with sample 16 + q
__device__ __forceinline__ void mat_mma16(const float (&a)[16], const float (&b)[16], f32x16_t &acc) {
#pragma unroll
    for (int q = 0; q < 16; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], b[q], acc, 0, 0, 0);
}

// One accumulator tile of the four wavefronts, added in wavefront order, to the workgroup's record.  KIND 0: dW2 rows 32 ta .., columns
// 32 tb ..; 1: dW1 rows 32 ta ..; 2: the heads' weights, units 32 tb .. (rows 0 .. na-1 the mean head, row 4 the value head)
template <int KIND>
__device__ __forceinline__ void mat_fold(float *red, const f32x16_t &acc, int ta, int tb, float *__restrict__ part, int ns, int na, int off_w2,
                                         int off_w3, int off_wv) {
    const int t = threadIdx.x;
#pragma unroll
    for (int r = 0; r < 16; ++r) red[(t >> 6) * 1024 + r * 64 + (t & 63)] = acc[r];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = t + kMatThreads * i, row = mat_row(e >> 6, (e >> 5) & 1), n = e & 31;
        float sum = red[e];
        sum += red[1024 + e];
        sum += red[2048 + e];
        sum += red[3072 + e];
        if constexpr (KIND == 0) {
            part[off_w2 + (32 * ta + row) * 64 + 32 * tb + n] = sum;
        } else if constexpr (KIND == 1) {
            if (n < ns) part[(32 * ta + row) * ns + n] = sum;
        } else {
            if (row < na) part[off_w3 + row * 64 + 32 * tb + n] = sum;
            else if (row == kTrkRows - 1) part[off_wv + 32 * tb + n] = sum;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(kMatThreads) void k_matrix_grad(const TrunkArgs A) {
    using L = MatLayout;
    __shared__ __attribute__((aligned(16))) float S[L::TOTAL];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, n = lane & 31, h = lane >> 5;
    const int ns = A.ns, na = A.na;
    // ---- stage the trunk and both heads in operand order ------------------------------------------------------------------------------
    for (int e = t; e < 4096; e += kMatThreads) {
        const int j = e & 3, l = (e >> 2) & 63, rq = (e >> 8) & 3, tb = (e >> 10) & 1, ta = e >> 11;
        const int m = l & 31, k = mat_row(4 * rq + j, l >> 5);
        S[L::A2 + e] = A.p[2][(32 * ta + m) * 64 + 32 * tb + k];    // (To, Tin) = (ta, tb)
        S[L::A2T + e] = A.p[2][(32 * tb + k) * 64 + 32 * ta + m];   // (Ti, Tj) = (ta, tb)
    }
    for (int e = t; e < 1024; e += kMatThreads) {
        const int j = e & 3, l = (e >> 2) & 63, sq = (e >> 8) & 1, T = e >> 9;
        const int c = 2 * (4 * sq + j) + (l >> 5);
        S[L::A1 + e] = c < ns ? A.p[0][(32 * T + (l & 31)) * ns + c] : 0.0f;
    }
    for (int e = t; e < 2 * kTrkRows * 32; e += kMatThreads) {
        const int i = e & 31, o = (e >> 5) % kTrkRows, hh = e / (kTrkRows * 32);
        const int k = 32 * (i >> 4) + mat_row(i & 15, hh);
        S[L::W3 + e] = o < 4 ? (o < na ? A.p[4][o * 64 + k] : 0.0f) : A.p[6][k];
    }
    if (t < 64) {
        S[L::B1 + t] = A.p[1][t];
        S[L::B2 + t] = A.p[3][t];
    }
    if (t < 8) S[L::B3 + t] = t < 4 ? (t < na ? A.p[5][t] : 0.0f) : (t == 4 ? A.p[7][0] : 0.0f);
    if (t < 4) S[L::LOGSTD + t] = t < na ? A.p[8][t] : 0.0f;
    __syncthreads();

    f32x16_t g2[2][2], g1[2], g3[2];   // dW2 [Tj][Ti], dW1 [Tj], the heads' dW [Ti]: this wavefront's sums over its tiles
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int r = 0; r < 16; ++r) g2[a][0][r] = g2[a][1][r] = g1[a][r] = g3[a][r] = 0.0f;
    }
    float gb2[2] = {}, gb1[2] = {};   // db2, db1 of unit 32 T + n over the samples of half h
    // per-sample lane (both halves hold the same; the h = 0 copy is summed): db3 of the mean head, db of the value head, dlogstd, the loss sums
    float gb3[4] = {}, gbv = 0.0f, gls[4] = {}, sum_pg = 0.0f, sum_vf = 0.0f, max_ratio = 0.0f;
    const float inv_b = 1.0f / (float)A.batch;
    const int64_t steps = ((int64_t)A.batch + kMatStep - 1) / kMatStep;

    for (int64_t step = blockIdx.x; step < steps; step += gridDim.x) {
        uint32_t base = 0;
        asm volatile("" : "+v"(base));   // keep LLVM from hoisting the weight reads out of the tile loop (384 registers of them)
        const float *W = S + base;
        float *tiles = S + base + L::WAVE + wave * L::WAVE_FLOATS;
        float *ha = tiles + L::HA, *hb = tiles + L::HB, *xt = tiles + L::X, *dt = tiles + L::D3;
        // ---- this lane's sample; a tail lane reads the last sample's column -----------------------------------------------------------
        const int64_t j = step * kMatStep + wave * kMatTile + n;
        const bool live = j < A.batch;
        const int64_t jc = live ? j : (int64_t)A.batch - 1;
        const int64_t col = A.idx ? A.idx[jc] : jc;
        // ---- the lane's half of the observation: component 2 s + h is the B operand of layer-1 slice s ---------------------------------
        float xb[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int c = 2 * s + h;
            float x = 0.0f;
            if (c < ns) {
                x = A.obs[(int64_t)c * A.obs_pitch + col];
                if (A.norm_tab) {   // THE arithmetic of include/rmav_ppo.h, uncontracted
                    const float lim = A.norm_tab[32];
                    x = (x - A.norm_tab[c]) * A.norm_tab[16 + c];
                    x = fminf(fmaxf(x, -lim), lim);
                }
            }
            xb[s] = x;
            xt[c * kMatPitch + n] = x;
        }
        // ---- forward: layer 1, 16 matrix instructions ----------------------------------------------------------------------------------
        f32x16_t h1[2], h2[2];
#pragma unroll
        for (int T = 0; T < 2; ++T) h1[T] = bias_frag(W + L::B1 + 32 * T, (uint32_t)h);
#pragma unroll
        for (int sq = 0; sq < 2; ++sq) {
            const float4 a40 = *reinterpret_cast<const float4 *>(W + L::A1 + ((0 * 2 + sq) * 64 + lane) * 4);
            const float4 a41 = *reinterpret_cast<const float4 *>(W + L::A1 + ((1 * 2 + sq) * 64 + lane) * 4);
            const float a0[4] = {a40.x, a40.y, a40.z, a40.w}, a1[4] = {a41.x, a41.y, a41.z, a41.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                h1[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[q], xb[4 * sq + q], h1[0], 0, 0, 0);
                h1[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[q], xb[4 * sq + q], h1[1], 0, 0, 0);
            }
        }
#pragma unroll
        for (int T = 0; T < 2; ++T)
#pragma unroll
            for (int r = 0; r < 16; ++r) h1[T][r] = tanhf(h1[T][r]);
        mat_put(ha, h1, n, h);
        // ---- layer 2: 64 matrix instructions fed straight from the accumulators --------------------------------------------------------
#pragma unroll
        for (int T = 0; T < 2; ++T) h2[T] = bias_frag(W + L::B2 + 32 * T, (uint32_t)h);
#pragma unroll
        for (int Tin = 0; Tin < 2; ++Tin)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const float4 a40 = *reinterpret_cast<const float4 *>(W + L::A2 + (((0 * 2 + Tin) * 4 + rq) * 64 + lane) * 4);
                const float4 a41 = *reinterpret_cast<const float4 *>(W + L::A2 + (((1 * 2 + Tin) * 4 + rq) * 64 + lane) * 4);
                const float a0[4] = {a40.x, a40.y, a40.z, a40.w}, a1[4] = {a41.x, a41.y, a41.z, a41.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    h2[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[q], h1[Tin][4 * rq + q], h2[0], 0, 0, 0);
                    h2[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[q], h1[Tin][4 * rq + q], h2[1], 0, 0, 0);
                }
            }
#pragma unroll
        for (int T = 0; T < 2; ++T)
#pragma unroll
            for (int r = 0; r < 16; ++r) h2[T][r] = tanhf(h2[T][r]);
        mat_put(hb, h2, n, h);
        // ---- the output layer on the vector ALU: the 32 units this lane holds, then the other half's from lane l ^ 32 -----------------
        float out[kTrkRows];
#pragma unroll
        for (int o = 0; o < kTrkRows; ++o) {
            float acc = 0.0f;
#pragma unroll
            for (int i4 = 0; i4 < 8; ++i4) {
                const float4 w = *reinterpret_cast<const float4 *>(W + L::W3 + (h * kTrkRows + o) * 32 + 4 * i4);
                acc = fmaf(w.x, h2[i4 >> 2][4 * (i4 & 3) + 0], acc);
                acc = fmaf(w.y, h2[i4 >> 2][4 * (i4 & 3) + 1], acc);
                acc = fmaf(w.z, h2[i4 >> 2][4 * (i4 & 3) + 2], acc);
                acc = fmaf(w.w, h2[i4 >> 2][4 * (i4 & 3) + 3], acc);
            }
            const float other = xor32(acc);
            const float lo = h ? other : acc, hi = h ? acc : other;
            out[o] = (lo + hi) + W[L::B3 + o];
        }
        // ---- both loss terms of sample n and the deltas of both heads (the expressions of rmav_learner_pg.inc and rmav_learner_vf.inc) --
        float d3[kTrkRows];
        {
            float ss = 0.0f, sum_ls = 0.0f, z[4], inv_std[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                z[c] = inv_std[c] = 0.0f;
                if (c < na) {
                    inv_std[c] = expf(-W[L::LOGSTD + c]);
                    z[c] = (A.act[(int64_t)c * A.act_pitch + col] - out[c]) * inv_std[c];
                    ss = fmaf(z[c], z[c], ss);
                    sum_ls += W[L::LOGSTD + c];
                }
            }
            const float logp = -0.5f * ss - sum_ls - 0.5f * (float)na * kLog2Pi;
            const float ratio = expf(logp - A.logp_old[col]);
            const float a = (A.adv[col] - A.adv_norm[0]) * A.adv_norm[1];
            const float lo = 1.0f - A.clip, hi = 1.0f + A.clip;
            const float t1 = -a * ratio, t2 = -a * fminf(fmaxf(ratio, lo), hi);
            const bool inside = ratio >= lo && ratio <= hi;
            // autograd: max() hands the gradient to the larger argument and halves it on a tie; clamp's is 1 on the closed interval
            float g_ratio = 0.0f;
            if (t1 > t2 || (t1 == t2 && inside)) g_ratio = -a;
            else if (t1 == t2) g_ratio = -0.5f * a;
            const float gl = live ? g_ratio * ratio * inv_b : 0.0f;   // d loss / d logp of this sample
            if (live) {
                sum_pg += fmaxf(t1, t2);
                max_ratio = fmaxf(max_ratio, ratio);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                d3[c] = 0.0f;
                if (c < na) {
                    const float d = gl * z[c] * inv_std[c];   // d logp / d mean_c = z_c / std_c
                    d3[c] = d;
                    gb3[c] += d;
                    gls[c] = fmaf(gl, fmaf(z[c], z[c], -1.0f), gls[c]);   // d logp / d logstd_c = z_c^2 - 1
                }
            }
        }
        {
            const float v = out[kTrkRows - 1], vo = A.val_old[col], rt = A.ret[col];
            const float dv = v - vo;
            const float vc = vo + fminf(fmaxf(dv, -A.clip), A.clip);
            const float u1 = v - rt, u2 = vc - rt;
            const float e1 = u1 * u1, e2 = u2 * u2;
            const bool inside = dv >= -A.clip && dv <= A.clip;
            float gv;   // d max(e1, e2) / d v
            if (e1 > e2) gv = 2.0f * u1;
            else if (e1 < e2) gv = inside ? 2.0f * u2 : 0.0f;
            else gv = u1 + (inside ? u2 : 0.0f);
            const float d = live ? A.vf_coef * 0.5f * gv * inv_b : 0.0f;
            if (live) sum_vf += fmaxf(e2, e1);   // (max is symmetric: the bits of rmav_learner_vf.inc's)
            d3[kTrkRows - 1] = d;
            gbv += d;
        }
        if (h == 0) {
#pragma unroll
            for (int o = 0; o < kTrkRows; ++o) dt[o * kMatPitch + n] = d3[o];
        }
        __builtin_amdgcn_wave_barrier();
        // ---- the heads' dW += d3 . h2^T: A rows beyond the five output rows zero --------------------------------------------------------
        {
            float av[16], bv[16];
            mat_zero(av);
            if (n < kTrkRows) mat_get(dt + n * kMatPitch + 16 * h, av);
#pragma unroll
            for (int Ti = 0; Ti < 2; ++Ti) {
                mat_get(hb + (32 * Ti + n) * kMatPitch + 16 * h, bv);
                mat_mma16(av, bv, g3[Ti]);
            }
        }
        // ---- delta 2 = (W3'^T d3) * (1 - h2^2) in accumulator layout, in place ------------------------------------------------------------
#pragma unroll
        for (int T = 0; T < 2; ++T)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float g = 0.0f;
#pragma unroll
                for (int o = 0; o < kTrkRows; ++o) g = fmaf(W[L::W3 + (h * kTrkRows + o) * 32 + 16 * T + r], d3[o], g);
                const float hv = h2[T][r];
                h2[T][r] = g * fmaf(-hv, hv, 1.0f);
            }
        // ---- delta 1 = (W2^T delta 2) * (1 - h1^2): 64 matrix instructions, delta 2's registers the B operand ----------------------------
        f32x16_t d1[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) d1[0][r] = d1[1][r] = 0.0f;
#pragma unroll
        for (int Tj = 0; Tj < 2; ++Tj)
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const float4 a40 = *reinterpret_cast<const float4 *>(W + L::A2T + (((0 * 2 + Tj) * 4 + rq) * 64 + lane) * 4);
                const float4 a41 = *reinterpret_cast<const float4 *>(W + L::A2T + (((1 * 2 + Tj) * 4 + rq) * 64 + lane) * 4);
                const float a0[4] = {a40.x, a40.y, a40.z, a40.w}, a1[4] = {a41.x, a41.y, a41.z, a41.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    d1[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[q], h2[Tj][4 * rq + q], d1[0], 0, 0, 0);
                    d1[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[q], h2[Tj][4 * rq + q], d1[1], 0, 0, 0);
                }
            }
#pragma unroll
        for (int T = 0; T < 2; ++T)
#pragma unroll
            for (int r = 0; r < 16; ++r) d1[T][r] *= fmaf(-h1[T][r], h1[T][r], 1.0f);
        mat_put(hb, h2, n, h);   // delta 2 over h2 (the heads' dW has read it)
        __builtin_amdgcn_wave_barrier();
        // ---- dW2 += delta 2 . h1^T, db2 -----------------------------------------------------------------------------------------------
#pragma unroll
        for (int Tj = 0; Tj < 2; ++Tj) {
            float av[16], bv[16];
            gb2[Tj] += mat_get(hb + (32 * Tj + n) * kMatPitch + 16 * h, av);
#pragma unroll
            for (int Ti = 0; Ti < 2; ++Ti) {
                mat_get(ha + (32 * Ti + n) * kMatPitch + 16 * h, bv);
                mat_mma16(av, bv, g2[Tj][Ti]);
            }
        }
        mat_put(ha, d1, n, h);   // delta 1 over h1 (dW2 has read it)
        __builtin_amdgcn_wave_barrier();
        // ---- dW1 += delta 1 . x^T, db1: B columns beyond the 16 observation rows zero (rows >= nS are zero in the tile) -------------------
        {
            float av[16], bv[16];
            mat_zero(bv);
            if (n < 16) mat_get(xt + n * kMatPitch + 16 * h, bv);
#pragma unroll
            for (int Tj = 0; Tj < 2; ++Tj) {
                gb1[Tj] += mat_get(ha + (32 * Tj + n) * kMatPitch + 16 * h, av);
                mat_mma16(av, bv, g1[Tj]);
            }
        }
        __builtin_amdgcn_wave_barrier();   // (the next tile overwrites the tiles)
    }

    // ---- this workgroup's partial record: the four wavefronts' sums in wavefront order; offsets of the flat layout from (ns, na) ---------
    const int off_b1 = 64 * ns, off_w2 = off_b1 + 64, off_b2 = off_w2 + 64 * 64, off_w3 = off_b2 + 64, off_b3 = off_w3 + 64 * na;
    const int off_wv = off_b3 + na, off_bv = off_wv + 64, off_logstd = off_bv + 1, off_stats = off_logstd + na;
    float *__restrict__ part = A.partial + (int64_t)blockIdx.x * (off_stats + kLrnStats);
    float *red = S;   // (weights and tiles are free now)
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int b = 0; b < 2; ++b) mat_fold<0>(red, g2[a][b], a, b, part, ns, na, off_w2, off_w3, off_wv);
        mat_fold<1>(red, g1[a], a, 0, part, ns, na, off_w2, off_w3, off_wv);
        mat_fold<2>(red, g3[a], 0, a, part, ns, na, off_w2, off_w3, off_wv);
    }
    // the bias sums of the 8 (wavefront, half) lanes that share a unit, and of the 4 x 32 sample lanes, in a fixed order
#pragma unroll
    for (int T = 0; T < 2; ++T) {
        red[(32 * T + n) * 8 + 2 * wave + h] = gb2[T];
        red[512 + (32 * T + n) * 8 + 2 * wave + h] = gb1[T];
    }
    if (h == 0) {
        float *dst = red + 1024 + 32 * wave + n;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            dst[c * 128] = gb3[c];
            dst[(kTrkRows + c) * 128] = gls[c];
        }
        dst[4 * 128] = gbv;
        dst[9 * 128] = sum_pg;
        dst[10 * 128] = sum_vf;
        dst[11 * 128] = max_ratio;
    }
    __syncthreads();
    if (t < 128) {   // db2 (t < 64), db1
        const float *src = red + 8 * t;
        float acc = 0.0f;
        for (int k = 0; k < 8; ++k) acc += src[k];
        part[(t < 64 ? off_b2 : off_b1) + (t & 63)] = acc;
    } else if (t < 128 + 12) {
        const int q = t - 128;   // 0..3 db3 of the mean head, 4 db of the value head, 5..8 dlogstd, 9 sum pg, 10 sum vf, 11 the largest ratio
        const float *src = red + 1024 + 128 * q;
        float acc = 0.0f;
        for (int w = 0; w < 4; ++w) {   // a wavefront's 32 lanes in order, then the wavefronts in order
            float sub = 0.0f;
            for (int k = 0; k < 32; ++k) sub = q == 11 ? fmaxf(sub, src[32 * w + k]) : sub + src[32 * w + k];
            acc = q == 11 ? fmaxf(acc, sub) : acc + sub;
        }
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

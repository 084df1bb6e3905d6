// rmav_obs_norm.hpp - running observation statistics (baselines' VecNormalize / RunningMeanStd, restated in include/rmav_ppo.h)
// on the device: batch moments of a stored observation array, their merge into the running state, and the elementwise
// normalisation.  The fused rollouts read only the fp32 tables at the end of the buffer (NormArgs, rmav_kernels.hpp).
//
// Each rule is written once and rmav_ret_norm.hpp uses the same ones: chan() combines two moments (threads, wavefronts, blocks AND
// the merge of a batch record into the running state), shifted_moment() turns a thread's sums into a moment, fold_partials() is the
// second stage of both moments launches, rstd_entry() the scale both tables hold.
//
// Moments are (n, mean, M2 = sum (x - mean)^2) triples in fp64 from the first per-thread value on: a thread accumulates
// sum (x - K) and sum (x - K)^2 with K = the first value it sees (x - K is exact in fp64 for fp32 data, and |x - K| is of the
// order of the spread, so the conversion to (mean, M2) does not cancel), and everything above a thread - lanes of a wavefront,
// wavefronts of a block, blocks of the grid, batches into the running state - is Chan's pairwise combination in a fixed order.
// No floating-point atomics: the same input gives the same bits.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace rmav {

typedef float nf32x4_t __attribute__((ext_vector_type(4)));
constexpr int kNormFeat = 16;   // features of the statistics buffer (the widest kind has 16 state components)

// The caller-owned statistics buffer (rmav_obs_norm_bytes() = sizeof, 16-byte aligned; include/rmav_ppo.h documents the fields)
struct ObsNormStats {
    double count;
    double mean[kNormFeat];
    double m2[kNormFeat];
    double eps;
    float clip;
    float pad0[3];
    float mean_f[kNormFeat];   // <- the tables the kernels read start here (byte 288): mean_f | rstd_f | clip_f | pad
    float rstd_f[kNormFeat];
    float clip_f;
    float pad1[3];
};
static_assert(sizeof(ObsNormStats) == 432 && offsetof(ObsNormStats, mean_f) == 288, "layout documented in include/rmav_ppo.h");
static_assert(offsetof(ObsNormStats, rstd_f) - offsetof(ObsNormStats, mean_f) == sizeof(float) * kNormFeat &&
                  offsetof(ObsNormStats, clip_f) - offsetof(ObsNormStats, mean_f) == sizeof(float) * 2 * kNormFeat,
              "NormArgs::tab = mean_f[16] | rstd_f[16] | clip");
constexpr int kMomentWords = 1 + 2 * kNormFeat;   // a batch record: count, mean[16], m2[16]

struct Moment {
    double n, mean, m2;
};
// Chan et al.: the moments of the union of two samples (a first, then b)
__device__ __forceinline__ Moment chan(const Moment a, const Moment b) {
    const double tot = a.n + b.n;
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    const double d = b.mean - a.mean;
    return Moment{tot, a.mean + d * b.n / tot, a.m2 + b.m2 + d * d * a.n * b.n / tot};
}
__device__ __forceinline__ Moment wave_chan(Moment m) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        Moment o;
        o.n = __shfl_down(m.n, off, 64);
        o.mean = __shfl_down(m.mean, off, 64);
        o.m2 = __shfl_down(m.m2, off, 64);
        m = chan(m, o);
    }
    return m;
}
// the block's moment in thread 0 (256 threads)
__device__ __forceinline__ Moment block_chan(Moment m) {
    __shared__ Moment sh[4];
    m = wave_chan(m);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) m = chan(chan(sh[0], sh[1]), chan(sh[2], sh[3]));
    return m;
}
// a thread's moment from its count and its sums of (x - K), (x - K)^2; no sample: the empty moment
__device__ __forceinline__ Moment shifted_moment(double cnt, double k0, double s1, double s2) {
    if (!(cnt > 0.0)) return Moment{0.0, 0.0, 0.0};
    return Moment{cnt, k0 + s1 / cnt, s2 - s1 * s1 / cnt};
}
// nblk partials -> one moment in thread 0 (one block of 256 threads)
__device__ __forceinline__ Moment fold_partials(const Moment *__restrict__ partial, int32_t nblk) {
    Moment m{0.0, 0.0, 0.0};
    for (int32_t b = threadIdx.x; b < nblk; b += 256) m = chan(m, partial[b]);
    return block_chan(m);
}
// THE table entry both normalisers scale by: 1 / sqrt(var + eps) of the running state, rounded to fp32 once
__device__ __forceinline__ float rstd_entry(double count, double m2, double eps) { return (float)(1.0 / sqrt(m2 / count + eps)); }

// Element (row r, feature c, env i) of an observation array sits at r * row + c * feat + i * elem floats:
//   SoA [n_rows][nS][pitch]: row = nS * pitch, feat = pitch, elem = 1;   AoS [n_rows * N][nS]: row = N * nS, feat = 1, elem = nS
struct ObsShape {
    int64_t n, row, feat, elem;
    int32_t n_rows, ns;
};

// Stage 1.  grid (x, nS): block (bx, c) takes feature c of env group bx % xenv and the rows bx / xenv, + rgroups, ... - VEC: 16-byte
// loads along N (SoA with a 16-byte aligned base and pitch % 4 == 0; the last quad of a row may reach into the row's padding, which
// is inside the allocation, and is masked).  partial [nS][gridDim.x] moments.
template <bool VEC>
__global__ __launch_bounds__(256) void k_obs_moments(const float *__restrict__ obs, const ObsShape sh, int32_t xenv, int32_t rgroups,
                                                     Moment *__restrict__ partial) {
    const int32_t c = blockIdx.y, ex = blockIdx.x % xenv, r0 = blockIdx.x / xenv;
    const int64_t i = ((int64_t)ex * 256 + threadIdx.x) * (VEC ? 4 : 1);
    double cnt = 0.0, k0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (i < sh.n && r0 < sh.n_rows) {
        const float *p = obs + (int64_t)c * sh.feat + i * sh.elem;
        k0 = (double)p[(int64_t)r0 * sh.row];
        auto take = [&](float v) {
            const double d = (double)v - k0;
            cnt += 1.0;
            s1 += d;
            s2 = fma(d, d, s2);
        };
#pragma unroll 4
        for (int32_t r = r0; r < sh.n_rows; r += rgroups) {
            if constexpr (VEC) {
                const nf32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const nf32x4_t *>(p + (int64_t)r * sh.row));
                take(v[0]);
                if (i + 1 < sh.n) take(v[1]);
                if (i + 2 < sh.n) take(v[2]);
                if (i + 3 < sh.n) take(v[3]);
            } else {
                take(p[(int64_t)r * sh.row]);
            }
        }
    }
    const Moment m = block_chan(shifted_moment(cnt, k0, s1, s2));
    if (threadIdx.x == 0) partial[(int64_t)c * gridDim.x + blockIdx.x] = m;
}

// Stage 2.  Block c folds feature c's partials into batch_out = (count, mean[16], m2[16]); blocks c >= nS write zeros.
__global__ __launch_bounds__(256) void k_obs_moments_fold(const Moment *__restrict__ partial, int32_t nblk, int32_t ns, double *__restrict__ batch_out) {
    const int32_t c = blockIdx.x;
    const bool used = c < ns;
    const Moment m = fold_partials(partial + (used ? (int64_t)c * nblk : 0), used ? nblk : 0);
    if (threadIdx.x == 0) {
        if (c == 0) batch_out[0] = m.n;
        batch_out[1 + c] = m.mean;
        batch_out[1 + kNormFeat + c] = m.m2;
    }
}

// the fp32 tables from the running state (thread c < 16); features >= ns stay at mean 0, scale 1
__device__ __forceinline__ void obs_norm_tables(ObsNormStats *st, int c, int ns, double count, double mean, double m2, double eps, float clip) {
    st->mean_f[c] = c < ns ? (float)mean : 0.0f;
    st->rstd_f[c] = c < ns ? rstd_entry(count, m2, eps) : 1.0f;
    if (c == 0) st->clip_f = clip;
}

__global__ __launch_bounds__(64) void k_obs_norm_init(ObsNormStats *st, int32_t ns, float clip, double eps, double count0) {
    const int c = threadIdx.x;
    if (c >= kNormFeat) return;
    if (c == 0) {
        st->count = count0;
        st->eps = eps;
        st->clip = clip;
        st->pad0[0] = st->pad0[1] = st->pad0[2] = 0.0f;
        st->pad1[0] = st->pad1[1] = st->pad1[2] = 0.0f;
    }
    st->mean[c] = 0.0;
    st->m2[c] = count0;   // var = 1
    obs_norm_tables(st, c, ns, count0, 0.0, count0, eps, clip);
}

// running state <- running state merged with n_batches records, in order: the update rule of RunningMeanStd in terms of
// M2 = var * count is chan(); empty (or NaN-count) records are skipped, features >= ns keep var = 1.  chan() takes a running count
// of exactly 0 as "no sample yet" and returns the record as it is; _init refuses count0 <= 0, so only a buffer written by the caller
// can hold one.
__global__ __launch_bounds__(64) void k_obs_norm_merge(ObsNormStats *st, const double *__restrict__ batch, int32_t n_batches, int32_t ns) {
    const int c = threadIdx.x;
    if (c >= kNormFeat) return;
    Moment run{st->count, st->mean[c], st->m2[c]};
    const double eps = st->eps;
    const float clip = st->clip;
    for (int32_t b = 0; b < n_batches; ++b) {
        const double *rec = batch + (int64_t)b * kMomentWords;
        const double bc = rec[0];
        if (!(bc > 0.0)) continue;
        if (c < ns) {
            run = chan(run, Moment{bc, rec[1 + c], rec[1 + kNormFeat + c]});
        } else {
            run.n += bc;
            run.m2 = run.n;   // var = 1
        }
    }
    __syncthreads();   // every thread has read the old count
    if (c == 0) st->count = run.n;
    st->mean[c] = run.mean;
    st->m2[c] = run.m2;
    obs_norm_tables(st, c, ns, run.n, run.mean, run.m2, eps, clip);
}

// THE arithmetic of observation normalisation, fp32, uncontracted, in this order (include/rmav_ppo.h): subtract, multiply, clamp
__device__ __forceinline__ float obs_norm_apply(float x, float mean, float rstd, float clip) {
    const float z = (x - mean) * rstd;
    return __builtin_amdgcn_fmed3f(z, -clip, clip);
}

// out = clamp((in - mean_f) * rstd_f, -clip, clip), one element per thread; out == in allowed
__global__ __launch_bounds__(256) void k_obs_normalize(const ObsNormStats *__restrict__ st, const float *in, float *out, const ObsShape sh) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t per_row = sh.n * sh.ns;
    if (q >= per_row * sh.n_rows) return;
    const int64_t r = q / per_row, w = q - r * per_row;
    // consecutive threads walk memory: SoA (elem == 1) env-fastest, AoS feature-fastest
    const int32_t c = sh.elem == 1 ? (int32_t)(w / sh.n) : (int32_t)(w % sh.ns);
    const int64_t i = sh.elem == 1 ? w % sh.n : w / sh.ns;
    const int64_t o = r * sh.row + (int64_t)c * sh.feat + i * sh.elem;
    out[o] = obs_norm_apply(in[o], st->mean_f[c], st->rstd_f[c], st->clip_f);
}

}  // namespace rmav

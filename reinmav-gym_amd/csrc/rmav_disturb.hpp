// rmav_disturb.hpp - the wind / gust disturbance (rmav_set_disturbance; include/rmav.h): what the *_ds kernels take and THE draw
// functions, host and device (tests/disturb_host compiles them for the CPU and compares them bit for bit with the numpy restatement).
//     wind   w_i = fma(span_i, u(W_i), lo_i)            one Philox block per env and episode: c2 = the episode's reset index, c3 = 5 << 24
//     gust   q_i = fma(g_i + g_i, u(G_i), -g_i)         one block per env and gust block b = t / hold: c2 = low word of b,
//                                                       c3 = (6 << 24) | (bits 32..47 of b) << 8
//     d_i = w_i + q_i                                   fp32, uncontracted, in this order
// and every gv_i of Env<K>::step reads gv_i + (R)d_i.  An all-zero spec gives w = fma(0, u, 0) = +0, q = fma(0, u, -0) = +0, d = +0.
#pragma once

#include "rmav_math.hpp"

namespace rmav {

// rmav_disturbance_spec with the wind as (lo, hi - lo): the span is ONE fp32 subtraction on the host, as RangeArgs::span
struct DisturbSpec {
    float lo[3], span[3];
    float gust[3];
    int32_t hold;      // agent steps per gust block
};
// Trailing kernel argument of the *_ds kernels: the spec by value and where the launch's first step stands in the gust sequence - the
// host divides once per launch.  The kernel bodies read spec(), b0 and phase0 only.
struct DisturbArgs {
    DisturbSpec v;
    uint64_t b0;       // gust block of the launch's first step: t0 / hold
    int32_t phase0;    // ... and that step's place in it: t0 % hold
    int32_t _pad;
    RMAV_HD const DisturbSpec &spec() const { return v; }
};

// ... and what the disturbed POLICY kernels read in its place: the spec through the handle's device copy (rmav_env_s::disturb_dev, rewritten
// in stream order by k_set_disturbance) - 2 scalar registers instead of 10 in kernels at their scalar-register limit - and the launch's place
// in the gust sequence by value.  The bodies read spec(), b0 and phase0 of either.
struct DisturbRef {
    const DisturbSpec *p;
    uint64_t b0;
    int32_t phase0;
    __device__ __forceinline__ const DisturbSpec &spec() const { return *p; }
};

// components of gv the kind reads: 2 for the 2-D kinds, 3 for the 3-D kinds
template <int K> constexpr int disturb_dim() { return (K == QUAD2D || K == QUAD2D_SL) ? 2 : 3; }

// the wind of the episode whose fresh state was drawn with reset index `reset_idx` (the index the env-constants stream uses)
template <int D> RMAV_HD void wind_draw(const DisturbSpec &ds, uint64_t seed, uint64_t env_id, uint32_t reset_idx, float (&w)[D]) {
    uint32_t r[4];
    philox4x32_10((uint32_t)env_id, (uint32_t)(env_id >> 32), reset_idx, 5u << 24, (uint32_t)seed, (uint32_t)(seed >> 32), r);
#pragma unroll
    for (int i = 0; i < D; ++i) w[i] = rfma(ds.span[i], u01(r[i]), ds.lo[i]);
}
// the gust of block b
template <int D> RMAV_HD void gust_draw(const DisturbSpec &ds, uint64_t seed, uint64_t env_id, uint64_t b, float (&q)[D]) {
    uint32_t r[4];
    philox4x32_10((uint32_t)env_id, (uint32_t)(env_id >> 32), (uint32_t)b, (6u << 24) | ((uint32_t)((b >> 32) & 0xFFFFu) << 8), (uint32_t)seed,
                  (uint32_t)(seed >> 32), r);
#pragma unroll
    for (int i = 0; i < D; ++i) q[i] = rfma(ds.gust[i] + ds.gust[i], u01(r[i]), -ds.gust[i]);
}
// gv + d for one lane: p_shared's gravity with the disturbance added in the kind's arithmetic type
template <int D, typename R> RMAV_HD void disturb_apply(ParamsT<R> &pl, const ParamsT<R> &p_shared, const float (&w)[D], const float (&q)[D]) {
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const float d = w[i] + q[i];
        pl.gv[i] = p_shared.gv[i] + (R)d;
    }
}

}  // namespace rmav

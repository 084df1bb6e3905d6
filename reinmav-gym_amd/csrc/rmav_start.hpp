// rmav_start.hpp - start-state ranges: the per-component reset distribution of a quadrotor handle (rmav_set_start_state; include/rmav.h):
// what the *_ss kernels take and THE map statement, host and device (tests/start_host compiles it for the CPU and compares it bit for
// bit with the numpy restatement, tests/start_ref.py).
//     s_c = fma(h_c, v_c, m_c)                                  fp32, one fma
//     h_c = (hi_c - lo_c) / 2, m_c = (hi_c + lo_c) / 2          derived by the host in fp64, each rounded to fp32 once
// v_c is what reset_state<K> draws - the "reset" stream, same counters, same words, v_c in [-1, 1) - so the identity spec (lo = -1, hi = 1:
// h = 1, m = 0) gives fma(1, v, 0) = v, the bits of a handle without a spec (v = -0.0 does not occur: v = fma(2^-23, x, -1) is +0.0 at x = 2^23).
#pragma once

#include <cstdint>

#ifndef RMAV_HD
#define RMAV_HD __host__ __device__ __forceinline__
#endif

namespace rmav {

// (h, m) of one component for the range [lo, hi]: fp64 from the spec's fp32 values, rounded to fp32 once each
inline void start_coeffs(float lo, float hi, float &h, float &m) {
    h = (float)(((double)hi - (double)lo) * 0.5);
    m = (float)(((double)hi + (double)lo) * 0.5);
}

// The coefficients of all (padded) components: the step kernels, the one-wavefront rollouts and k_reset_ss take them by value (StartArgs);
// the policy kernels read the handle's device copy (StartDev, rmav_kernels.hpp).
struct StartCoef {
    float h[16], m[16];
};
// Trailing kernel argument of the *_ss kernels.  al_on: whether the handle has actuator lag (wave-uniform).  The kernels are cut from the
// lagged bodies; with al_on = 0 they neither load nor store the filter state (ActuatorArgs::m may be NULL) and hand the command itself to
// the dynamics - the filter is gated, not run with alpha = 1, so that a -0.0 action keeps its sign as on a handle without a start spec.
struct StartArgs {
    StartCoef c;
    uint32_t al_on;
    uint32_t _pad;
};
static_assert(sizeof(StartCoef) == 128 && sizeof(StartArgs) == 136, "32 floats and the flag");

// THE map statement: component c of a fresh state from what reset_state<K> drew for it
RMAV_HD float start_map(float h, float v, float m) { return __builtin_fmaf(h, v, m); }

#if defined(__HIPCC__) || defined(__HIP_DEVICE_COMPILE__)
// ... of all NS components of a lane, in place.  A reset touches about 1.3 % of the lanes per step, so the 2 NS coefficients are read HERE,
// where they are used: each index is opaque to the optimiser, which therefore cannot hoist the reads out of the step loop and hold them in
// registers through it (the trick of norm_tab, rmav_kernels.hpp; with the reads visible the one-wavefront slung-load rollouts spill 60 to 80
// more scalar registers).  By value they are scalar loads from the kernel-argument segment, through
// a pointer scalar loads from the handle's device copy.
template <int NS> __device__ __forceinline__ void start_apply(const StartCoef &c, float (&s)[NS]) {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        uint32_t o = 0u;
        asm volatile("" : "+s"(o));
        s[i] = start_map(c.h[o + (uint32_t)i], s[i], c.m[o + (uint32_t)i]);
    }
}
#endif

}  // namespace rmav

// rmav_term.hpp - termination rules: the per-axis position box, the tilt limit and the finiteness test of a quadrotor handle
// (rmav_set_termination; include/rmav.h): what the *_tc kernels take and THE rule, host and device (tests/term_host compiles it for the CPU
// and compares every decision with the numpy restatement, tests/term_ref.py).  On the stored post-step fp32 state s, in fp32, nothing
// contracted but the fmas written here:
//     nonfinite = any c < nS: !(|s_c| < inf)
//     outside   = any body B, any axis i < dim: !(B_i >= pos_lo_i) || !(B_i <= pos_hi_i)       bodies: the quadrotor s[0:dim] and - the
//                 slung-load kinds - the load (s[5:7] / s[10:13])
//     tilted    = 2-D kinds: |s[2]| > tilt                                                     tilt = max_tilt (the angle is never wrapped)
//                 3-D kinds: fma(w,w, fma(z,z, -fma(x,x, y*y))) < tilt * fma(w,w, fma(x,x, fma(y,y, z*z)))
//                            (w,x,y,z) = s[3:7], tilt = (float)cos((double)max_tilt), -inf for no limit: the world-z component of the body's
//                            z axis against cos(max_tilt), both sides times |q|^2 - no division, no reciprocal square root
//     rule      = nonfinite || outside || tilted
// The comparisons are written so that a NaN on either side decides "ends" for the box and "does not fire" for the tilt; nonfinite catches
// the latter.  The kernels OR the rule into the termination flag of every dynamics sub-step, directly behind Env<K>::step.
#pragma once

#include <cstdint>

#ifndef RMAV_HD
#define RMAV_HD __host__ __device__ __forceinline__
#endif

namespace rmav {

// Trailing kernel argument of the *_tc kernels: the seven thresholds, by value in the step kernels and the one-wavefront rollouts, through
// the handle's device copy (TermDev, rmav_kernels.hpp) in the policy kernels.  tilt: max_tilt itself for the 2-D kinds, cos(max_tilt) for the
// 3-D kinds (term_tilt below: the host rounds it once).
struct TermArgs {
    float v[8];   // pos_lo at 0 .. 2, pos_hi at 3 .. 5, tilt at 6, padding (0)
    RMAV_HD float pos_lo(int i) const { return v[i]; }
    RMAV_HD float pos_hi(int i) const { return v[3 + i]; }
    RMAV_HD float tilt() const { return v[6]; }
};
static_assert(sizeof(TermArgs) == 32, "seven thresholds and the padding");

// the kinds by number (rmav_math.hpp's enum: quad2d, quad2d_sl, quad3d, quad3d_sl) - this header stands alone for the host test program
template <int K> struct TermDims {
    static_assert(K >= 0 && K <= 3, "the four quadrotor kinds");
    static constexpr int DIM = (K < 2) ? 2 : 3;
    static constexpr int NS = (K == 0) ? 5 : (K == 1) ? 9 : (K == 2) ? 10 : 16;
    static constexpr int LOAD = (K == 1) ? 5 : (K == 3) ? 10 : -1;   // first component of the load's position, -1: no load
};

// the seventh threshold from the spec's max_tilt (radians in [0, pi] or +inf): fp64 cosine, rounded to fp32 once
inline float term_tilt(int kind, float max_tilt) {
    if (kind < 2) return max_tilt;
    if (!(max_tilt < __builtin_inff())) return -__builtin_inff();
    return (float)__builtin_cos((double)max_tilt);
}

// THE rule
template <int K> RMAV_HD bool term_rule(const float (&s)[TermDims<K>::NS], const TermArgs &t) {
    constexpr int NS = TermDims<K>::NS, DIM = TermDims<K>::DIM, LOAD = TermDims<K>::LOAD;
    bool fire = false;
#pragma unroll
    for (int c = 0; c < NS; ++c) fire = fire || !(__builtin_fabsf(s[c]) < __builtin_inff());
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
        fire = fire || !(s[i] >= t.pos_lo(i)) || !(s[i] <= t.pos_hi(i));
        if constexpr (LOAD >= 0) fire = fire || !(s[LOAD + i] >= t.pos_lo(i)) || !(s[LOAD + i] <= t.pos_hi(i));
    }
    if constexpr (DIM == 2) {
        fire = fire || (__builtin_fabsf(s[2]) > t.tilt());
    } else {
        const float w = s[3], x = s[4], y = s[5], z = s[6];
        const float up = __builtin_fmaf(w, w, __builtin_fmaf(z, z, -__builtin_fmaf(x, x, y * y)));
        const float n2 = __builtin_fmaf(w, w, __builtin_fmaf(x, x, __builtin_fmaf(y, y, z * z)));
        fire = fire || (up < t.tilt() * n2);
    }
    return fire;
}

}  // namespace rmav

// rmav_sensor.hpp - Gaussian sensor noise on the observations (rmav_set_sensor_noise; include/rmav.h): what the *_sn kernels take and THE
// draw, host and device (tests/sensor_host compiles the counter / words part for the CPU and compares it bit for bit with the numpy
// restatement, tests/sensor_ref.py).
//     o_c = fma(sigma_c, z_c, s_c)                      fp32; s the true state the observation reports
//     z[4j .. 4j+3]                                     one Philox block per env, step counter b and j = c >> 2:
//                                                       c2 = low word of b, c3 = (7 << 24) | (bits 32..47 of b) << 8 | j
//     Box-Muller on (r0, r1) and (r2, r3) exactly as the policy noise (gaussian4, rmav_policy.hpp): u1 = ((r >> 8) + 1) 2^-24,
//     u2 = (r' >> 8) 2^-24, rad = sqrtf(-2 logf(u1)), sincospif(2 u2), z = rad (cos, sin)
// b is the handle's step counter AFTER the operation that produced the observation.  sigma_c = 0 gives fma(0, z, s) = s (a -0.0 may
// come out as +0.0).  gaussian4's lines are restated here, not shared: no pre-existing kernel reads this header's functions.
#pragma once

#include "rmav_math.hpp"

namespace rmav {

// Trailing kernel argument of the *_sn kernels and of k_observe: rmav_sensor_noise_spec by value (components >= nS are zero and not read)
struct SensorArgs {
    float sigma[16];
};

// the four Philox words of block (b, j) of env env_id
RMAV_HD void sensor_words(uint64_t seed, uint64_t env_id, uint64_t b, uint32_t j, uint32_t (&r)[4]) {
    philox4x32_10((uint32_t)env_id, (uint32_t)(env_id >> 32), (uint32_t)b, (7u << 24) | ((uint32_t)((b >> 32) & 0xFFFFu) << 8) | j, (uint32_t)seed,
                  (uint32_t)(seed >> 32), r);
}
// ... and the two uniforms of pair p of such a block: u1 in (0, 1], u2 in [0, 1), both exact in fp32
RMAV_HD void sensor_uniforms(const uint32_t (&r)[4], int p, float &u1, float &u2) {
    u1 = (float)((r[2 * p] >> 8) + 1u) * (1.0f / 16777216.0f);
    u2 = u01(r[2 * p + 1]);
}

// z[4j .. 4j+3] of (env, b)
__device__ __forceinline__ void sensor_z4(uint64_t seed, uint64_t env_id, uint64_t b, uint32_t j, float (&z)[4]) {
    uint32_t r[4];
    sensor_words(seed, env_id, b, j, r);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        float u1, u2;
        sensor_uniforms(r, p, u1, u2);
        const float rad = __builtin_sqrtf(-2.0f * logf(u1));
        float sn, cs;
        sincospif(2.0f * u2, &sn, &cs);
        z[2 * p] = rad * cs;
        z[2 * p + 1] = rad * sn;
    }
}

// THE draw: z[0 .. NS-1] of (env, b), block by block
template <int NS> __device__ __forceinline__ void sensor_draw(uint64_t seed, uint64_t env_id, uint64_t b, float (&z)[NS]) {
#pragma unroll
    for (int j = 0; j < (NS + 3) / 4; ++j) {
        float z4[4];
        sensor_z4(seed, env_id, b, (uint32_t)j, z4);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (4 * j + i < NS) z[4 * j + i] = z4[i];
    }
}
// ... and the observation of the state s under it
template <int NS> __device__ __forceinline__ void sensor_apply(const SensorArgs &sn, const float (&z)[NS], const float (&s)[NS], float (&o)[NS]) {
#pragma unroll
    for (int c = 0; c < NS; ++c) o[c] = rfma(sn.sigma[c], z[c], s[c]);
}

// ... block by block, four components at a time, into the words dst[c * 64] of a pair kernel's LDS row: neither z nor the observation
// outlives a block in registers (the pair kernels sit at their register limits)
template <int NS>
__device__ __forceinline__ void sensor_store_row(const SensorArgs &sn, uint64_t seed, uint64_t env_id, uint64_t b, const float (&s)[NS], float *dst) {
#pragma unroll
    for (int j = 0; j < (NS + 3) / 4; ++j) {
        float z4[4];
        sensor_z4(seed, env_id, b, (uint32_t)j, z4);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (4 * j + i < NS) dst[(4 * j + i) * 64] = rfma(sn.sigma[4 * j + i], z4[i], s[4 * j + i]);
    }
}

}  // namespace rmav

// rmav_actuator.hpp - actuator lag: a first-order motor model between the commanded action and the dynamics (rmav_set_actuator;
// include/rmav.h): what the *_al kernels take and THE filter statement, host and device (tests/actuator_host compiles it for the CPU and
// compares it bit for bit with the numpy restatement, tests/actuator_ref.py).
//     m_c = fma(alpha_c, u_c, beta_c * m_c)             fp32; the product beta_c * m_c is rounded on its own, then one fma
//     alpha_c = 1 - exp(-dt / tau_c), beta_c = exp(-dt / tau_c)    derived by the host in fp64, each rounded to fp32 once
// per ordinary dynamics step (every sub-step of a frame skip); the dynamics read m, everything else reads the command u.  tau_c = 0 gives
// alpha = 1, beta = 0 and m_c = fma(1, u_c, 0 * m_c) = u_c (a -0.0 command may come out as +0.0).
#pragma once

#include <cmath>
#include <cstdint>

#ifndef RMAV_HD
#define RMAV_HD __host__ __device__ __forceinline__
#endif

namespace rmav {

// (alpha, beta) of one component for the time constant tau >= 0 (seconds) and the step dt: fp64, rounded to fp32 once each
inline void actuator_coeffs(double tau, double dt, float &alpha, float &beta) {
    if (!(tau > 0.0)) {
        alpha = 1.0f;
        beta = 0.0f;
        return;
    }
    const double e = std::exp(-dt / tau);
    alpha = (float)(1.0 - e);
    beta = (float)e;
}

// Trailing kernel argument of the *_al kernels: the coefficients and the episode's first m by value, the handle's [nA][N] array of m, and
// whether the handle has sensor noise (wave-uniform: the kernels are cut from the noisy bodies and skip the draw with one scalar branch per
// site when it is 0).  The policy kernels read the first twelve words through the handle's device copy (ActuatorDev).
struct ActuatorCoef {
    float alpha[4], beta[4], init[4];
};
struct ActuatorArgs {
    ActuatorCoef c;
    float *m;
    uint32_t sn_on;
    uint32_t _pad;
};

// THE filter statement: one dynamics step of component c
RMAV_HD float actuator_filter(float alpha, float beta, float m, float u) {
    const float bm = beta * m;   // (rounded on its own: the build contracts nothing, -ffp-contract=off)
    return __builtin_fmaf(alpha, u, bm);
}

// ... of all NA components of a lane
template <int NA> RMAV_HD void actuator_step(const ActuatorCoef &c, float (&m)[NA], const float (&u)[NA]) {
#pragma unroll
    for (int i = 0; i < NA; ++i) m[i] = actuator_filter(c.alpha[i], c.beta[i], m[i], u[i]);
}

}  // namespace rmav

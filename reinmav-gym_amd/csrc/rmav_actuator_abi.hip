// rmav_actuator_abi.hip - the launches of a handle with actuator lag (rmav_set_actuator; include/rmav.h): the single-step kernels k_step_al,
// the one-wavefront fused rollouts k_rollout_al, and the two small kernels that keep the handle's device data: k_actuator_fill (every env's
// m = init) and k_set_actuator (the policy kernels' copy of the coefficients).  A translation unit of its own, as rmav_sensor_abi.hip and
// for its reason; rmav_abi.hip decides what a call launches and comes here only for the launch itself.
#include "rmav_rung_launch.hpp"

using namespace rmav;

namespace rmav {

// m[c][i] = init[c] for every env i of the handle (vector stores)
__global__ __launch_bounds__(kBlock) void k_actuator_fill(float *m, int64_t n, int32_t na, const ActuatorCoef v) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (c < na) m[(int64_t)c * n + i] = v.init[c];
}

// the handle's device copy (ActuatorDev): alpha, beta, init - twelve words - then the calm disturbance spec - nine zeros and the hold - by
// vector stores
__global__ __launch_bounds__(64) void k_set_actuator(uint32_t *dst, const ActuatorCoef v, uint32_t calm_hold) {
    static_assert(sizeof(ActuatorDev) == 22 * sizeof(uint32_t) && offsetof(ActuatorDev, calm) == 48 && offsetof(DisturbSpec, hold) == 36, "12 + 9 + 1 words");
    uint32_t x = 0u;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        x = (threadIdx.x == i) ? __builtin_bit_cast(uint32_t, v.alpha[i]) : x;
        x = (threadIdx.x == 4u + i) ? __builtin_bit_cast(uint32_t, v.beta[i]) : x;
        x = (threadIdx.x == 8u + i) ? __builtin_bit_cast(uint32_t, v.init[i]) : x;
    }
    x = (threadIdx.x == 21u) ? calm_hold : x;
    if (threadIdx.x < 22u) dst[threadIdx.x] = x;
}

}  // namespace rmav

namespace {

struct Kernels {
    template <int K, int MODE, int ST, bool TL, bool RW> static auto rollout() { return k_rollout_al<K, MODE, TL, RW>; }
    template <int K, bool CTRL, bool TL, bool RW> static auto step() { return k_step_al<K, TL, RW>; }
};

}  // namespace

int rmav_launch_actuator_rollout(rmav_handle h, int mode, int st, const RolloutArgs &a) { return launch_rung_rollout<RUNG_ACTUATOR, Kernels>(h, mode, st, a); }

int rmav_launch_actuator_step(rmav_handle h, const RolloutArgs &a, bool ctrl, int bs, const FinalArgs &fa) { return launch_rung_step<RUNG_ACTUATOR, Kernels>(h, a, ctrl, bs, fa); }

int rmav_launch_actuator_fill(rmav_handle h) {
    hipLaunchKernelGGL(k_actuator_fill, dim3((unsigned)((h->n + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, h->actuator_m, h->n, (int32_t)kActionDim[h->kind],
                       actuator_coef(h));
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

int rmav_sync_actuator_dev(rmav_handle h) {
    hipLaunchKernelGGL(k_set_actuator, dim3(1), dim3(64), 0, h->stream, reinterpret_cast<uint32_t *>(h->actuator_dev), actuator_coef(h), (uint32_t)kCalmHold);
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

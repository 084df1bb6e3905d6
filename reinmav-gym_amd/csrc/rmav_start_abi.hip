// rmav_start_abi.hip - the launches of a handle with a start-state spec (rmav_set_start_state; include/rmav.h): the single-step kernels
// k_step_ss, the one-wavefront fused rollouts k_rollout_ss, the reset k_reset_ss, and the small kernel that keeps the handle's device copy
// of the coefficients, k_set_start_state.  A translation unit of its own, as rmav_actuator_abi.hip and for its reason; rmav_abi.hip decides
// what a call launches and comes here only for the launch itself.
#include "rmav_rung_launch.hpp"

using namespace rmav;

namespace rmav {

// the handle's device copy (StartDev): h, m - thirty-two words - then the calm disturbance spec - nine zeros and the hold - by vector stores
__global__ __launch_bounds__(64) void k_set_start_state(uint32_t *dst, const StartCoef v, uint32_t calm_hold) {
    static_assert(sizeof(StartDev) == 42 * sizeof(uint32_t) && offsetof(StartDev, calm) == 128 && offsetof(DisturbSpec, hold) == 36, "32 + 9 + 1 words");
    uint32_t x = 0u;
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i) {
        x = (threadIdx.x == i) ? __builtin_bit_cast(uint32_t, v.h[i]) : x;
        x = (threadIdx.x == 16u + i) ? __builtin_bit_cast(uint32_t, v.m[i]) : x;
    }
    x = (threadIdx.x == 41u) ? calm_hold : x;
    if (threadIdx.x < 42u) dst[threadIdx.x] = x;
}

}  // namespace rmav

namespace {

struct Kernels {
    template <int K, int MODE, int ST, bool TL, bool RW> static auto rollout() { return k_rollout_ss<K, MODE, TL, RW>; }
    template <int K, bool CTRL, bool TL, bool RW> static auto step() { return k_step_ss<K, TL, RW>; }
};

}  // namespace

int rmav_launch_start_rollout(rmav_handle h, int mode, int st, const RolloutArgs &a) { return launch_rung_rollout<RUNG_START, Kernels>(h, mode, st, a); }

int rmav_launch_start_step(rmav_handle h, const RolloutArgs &a, bool ctrl, int bs, const FinalArgs &fa) { return launch_rung_step<RUNG_START, Kernels>(h, a, ctrl, bs, fa); }

int rmav_launch_start_reset(rmav_handle h, float *obs_dev, int layout) {
    const uint32_t fl = (h->flags & F_TRACK) | (layout == RMAV_AOS ? F_AOS : 0u);
    const StartCoef c = start_coef(h);
    return dispatch_kind<QUAD_KINDS>(h->kind, [&](auto k) {
        hipLaunchKernelGGL((k_reset_ss<decltype(k)::value>), grid_for(h), dim3(block_size(h)), 0, h->stream, h->state, h->n, h->rec, h->ep_ret, (uint32_t)h->t,
                           obs_dev, h->seed, h->env_base, fl, c);
        HIP_TRY(hipGetLastError());
        return (int)RMAV_OK;
    });
}

int rmav_sync_start_dev(rmav_handle h) {
    hipLaunchKernelGGL(k_set_start_state, dim3(1), dim3(64), 0, h->stream, reinterpret_cast<uint32_t *>(h->start_dev), start_coef(h), (uint32_t)kCalmHold);
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

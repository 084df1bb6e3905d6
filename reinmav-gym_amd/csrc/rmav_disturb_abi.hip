// rmav_disturb_abi.hip - the launches of a handle with a wind / gust disturbance (rmav_set_disturbance; include/rmav.h): the single-step
// kernels k_step_ds, the one-wavefront fused rollouts k_rollout_ds and k_disturbance_now.  A translation unit of its own, as
// rmav_reward_abi.hip and for its reason; rmav_abi.hip decides what a call launches and comes here only for the launch itself.
#include "rmav_rung_launch.hpp"

using namespace rmav;

namespace rmav {

// the handle's device copy of the spec (the policy kernels read it by pointer): rewritten in stream order, by vector stores
__global__ __launch_bounds__(64) void k_set_disturbance(uint32_t *dst, const DisturbSpec v) {
    const uint32_t w[10] = {__builtin_bit_cast(uint32_t, v.lo[0]),   __builtin_bit_cast(uint32_t, v.lo[1]),   __builtin_bit_cast(uint32_t, v.lo[2]),
                            __builtin_bit_cast(uint32_t, v.span[0]), __builtin_bit_cast(uint32_t, v.span[1]), __builtin_bit_cast(uint32_t, v.span[2]),
                            __builtin_bit_cast(uint32_t, v.gust[0]), __builtin_bit_cast(uint32_t, v.gust[1]), __builtin_bit_cast(uint32_t, v.gust[2]),
                            (uint32_t)v.hold};
    static_assert(sizeof(DisturbSpec) == sizeof(w), "nine floats and the hold");
    uint32_t x = w[0];
#pragma unroll
    for (uint32_t i = 1; i < 10; ++i) x = (threadIdx.x == i) ? w[i] : x;
    if (threadIdx.x < 10u) dst[threadIdx.x] = x;
}

}  // namespace rmav

namespace {

struct Kernels {
    template <int K, int MODE, int ST, bool TL, bool RW> static auto rollout() { return k_rollout_ds<K, MODE, TL, RW>; }
    template <int K, bool CTRL, bool TL, bool RW> static auto step() { return k_step_ds<K, TL, RW>; }
};

}  // namespace

int rmav_launch_disturb_rollout(rmav_handle h, int mode, int st, const RolloutArgs &a) { return launch_rung_rollout<RUNG_DISTURB, Kernels>(h, mode, st, a); }

int rmav_launch_disturb_step(rmav_handle h, const RolloutArgs &a, bool ctrl, int bs, const FinalArgs &fa) { return launch_rung_step<RUNG_DISTURB, Kernels>(h, a, ctrl, bs, fa); }

int rmav_launch_disturbance_now(rmav_handle h, float *out_dev) {
    const DisturbArgs ds = disturb_args(h, h->t);
    const int rc = dispatch_kind<QUAD_KINDS>(h->kind, [&](auto k) {
        hipLaunchKernelGGL((k_disturbance_now<decltype(k)::value>), dim3((unsigned)((h->n + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, out_dev, h->n,
                           h->rec, h->seed, h->env_base, ds);
        return (int)RMAV_OK;
    });
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

int rmav_sync_disturb_dev(rmav_handle h) {
    hipLaunchKernelGGL(k_set_disturbance, dim3(1), dim3(64), 0, h->stream, reinterpret_cast<uint32_t *>(h->disturb_dev), disturb_args(h, 0).v);
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

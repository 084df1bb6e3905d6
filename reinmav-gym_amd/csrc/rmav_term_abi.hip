// rmav_term_abi.hip - the launches of a handle with a termination spec (rmav_set_termination; include/rmav.h): the single-step kernels
// k_step_tc, the one-wavefront fused rollouts k_rollout_tc, and the small kernel that keeps the handle's device copy of the thresholds,
// k_set_termination.  A translation unit of its own, as rmav_start_abi.hip and for its reason; rmav_abi.hip decides what a call launches
// and comes here only for the launch itself.
#include "rmav_rung_launch.hpp"

using namespace rmav;

namespace rmav {

// the handle's device copy (TermDev): the thresholds - eight words -, the identity start coefficients - sixteen ones, sixteen zeros -, then
// the calm disturbance spec - nine zeros and the hold - by vector stores
__global__ __launch_bounds__(64) void k_set_termination(uint32_t *dst, const TermArgs v, uint32_t calm_hold) {
    static_assert(sizeof(TermDev) == 50 * sizeof(uint32_t) && offsetof(TermDev, ident) == 32 && offsetof(TermDev, calm) == 160 && offsetof(DisturbSpec, hold) == 36,
                  "8 + 32 + 9 + 1 words");
    uint32_t x = 0u;
#pragma unroll
    for (uint32_t i = 0; i < 7; ++i) x = (threadIdx.x == i) ? __builtin_bit_cast(uint32_t, v.v[i]) : x;
    x = (threadIdx.x >= 8u && threadIdx.x < 24u) ? __builtin_bit_cast(uint32_t, 1.0f) : x;   // h = 1 (m = 0 behind it)
    x = (threadIdx.x == 49u) ? calm_hold : x;
    if (threadIdx.x < 50u) dst[threadIdx.x] = x;
}

}  // namespace rmav

namespace {

struct Kernels {
    template <int K, int MODE, int ST, bool TL, bool RW> static auto rollout() { return k_rollout_tc<K, MODE, TL, RW>; }
    template <int K, bool CTRL, bool TL, bool RW> static auto step() { return k_step_tc<K, TL, RW>; }
};

}  // namespace

int rmav_launch_term_rollout(rmav_handle h, int mode, int st, const RolloutArgs &a) { return launch_rung_rollout<RUNG_TERM, Kernels>(h, mode, st, a); }

int rmav_launch_term_step(rmav_handle h, const RolloutArgs &a, bool ctrl, int bs, const FinalArgs &fa) { return launch_rung_step<RUNG_TERM, Kernels>(h, a, ctrl, bs, fa); }

int rmav_sync_term_dev(rmav_handle h) {
    hipLaunchKernelGGL(k_set_termination, dim3(1), dim3(64), 0, h->stream, reinterpret_cast<uint32_t *>(h->term_dev), term_args(h), (uint32_t)kCalmHold);
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

// rmav_reward_abi.hip - the launches of a handle with a tracking reward (rmav_set_reward; include/rmav.h): the single-step kernels
// k_step_rw, the one-wavefront fused rollouts k_rollout_rw and the kernel that rewrites the handle's device copy of the spec.  A
// translation unit of its own, as rmav_skip_abi.hip and for its reason; rmav_abi.hip decides what a call launches and comes here only for
// the launch itself.  The tracking-reward policy rollouts are in rmav_policy_abi.hip.
#include "rmav_rung_launch.hpp"

using namespace rmav;

namespace rmav {

// the handle's device copy of the spec (the policy kernels read it by pointer): rewritten in stream order, by vector stores
__global__ __launch_bounds__(64) void k_set_reward(float *dst, const RewardArgs v) {
    const float w[12] = {v.goal[0], v.goal[1], v.goal[2], v.alive, v.w_pos, v.w_vel, v.w_act, v.act_ref[0], v.act_ref[1], v.act_ref[2], v.act_ref[3], v.terminal};
    static_assert(sizeof(RewardArgs) == sizeof(w), "twelve floats");
    float x = w[0];
#pragma unroll
    for (uint32_t i = 1; i < 12; ++i) x = (threadIdx.x == i) ? w[i] : x;
    if (threadIdx.x < 12u) dst[threadIdx.x] = x;
}

}  // namespace rmav

namespace {

struct Kernels {
    template <int K, int MODE, int ST, bool TL, bool RW> static auto rollout() { return k_rollout_rw<K, MODE, ST, TL>; }
    template <int K, bool CTRL, bool TL, bool RW> static auto step() { return k_step_rw<K, TL>; }
};

}  // namespace

int rmav_launch_reward_rollout(rmav_handle h, int mode, int st, const RolloutArgs &a) { return launch_rung_rollout<RUNG_REWARD, Kernels>(h, mode, st, a); }

int rmav_launch_reward_step(rmav_handle h, const RolloutArgs &a, bool ctrl, int bs, const FinalArgs &fa) { return launch_rung_step<RUNG_REWARD, Kernels>(h, a, ctrl, bs, fa); }

int rmav_sync_reward_dev(rmav_handle h) {
    hipLaunchKernelGGL(k_set_reward, dim3(1), dim3(64), 0, h->stream, reinterpret_cast<float *>(h->reward_dev), reward_args(h));
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

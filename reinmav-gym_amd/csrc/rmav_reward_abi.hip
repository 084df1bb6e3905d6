// rmav_reward_abi.hip - the launches of a handle with a tracking reward (rmav_set_reward; include/rmav.h): the single-step kernels
// k_step_rw, the one-wavefront fused rollouts k_rollout_rw and the kernel that rewrites the handle's device copy of the spec.  A
// translation unit of its own, as rmav_skip_abi.hip and for its reason; rmav_abi.hip decides what a call launches and comes here only for
// the launch itself.  The tracking-reward policy rollouts are in rmav_policy_abi.hip.
#include "rmav_handle.hpp"

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

template <int K, int MODE> int launch_km(rmav_handle h, int st, const RolloutArgs &a) {
    const KindParams<K> kp = kind_params<K>(h);
    const int64_t count = a.slice_count ? (int64_t)a.slice_count : h->n;
    const dim3 grid((unsigned)((count + block_size(h) - 1) / block_size(h))), block(block_size(h));
    const TimeLimitArgs tl = tl_args(h);
    const RangeArgs dr = range_args(h);
    const FrameSkipArgs fs = skip_args(h);
    const RewardArgs rw = reward_args(h);
    // (the ranged kernels' store policies: batch-major obs through the per-lane stores, ST_AOS_LDS runs the write-through kernel)
    return dispatch_store<ST_WRITE_THROUGH, ST_DEFAULT, ST_STREAM>(st, [&](auto s) {
        constexpr int ST = decltype(s)::value;
        if (h->time_limit > 0) hipLaunchKernelGGL((k_rollout_rw<K, MODE, ST, true>), grid, block, 0, h->stream, a, kp.p, kp.pc, tl, dr, fs, rw);
        else hipLaunchKernelGGL((k_rollout_rw<K, MODE, ST, false>), grid, block, 0, h->stream, a, kp.p, kp.pc, tl, dr, fs, rw);
        return (int)RMAV_OK;
    });
}

template <int K> void launch_step(rmav_handle h, const RolloutArgs &a, int bs, const FinalArgs &fa) {
    const KindParams<K> kp = kind_params<K>(h);
    const dim3 grid((unsigned)((h->n + bs - 1) / bs));
    const TimeLimitArgs tl = tl_args(h);
    const RangeArgs dr = range_args(h);
    const FrameSkipArgs fs = skip_args(h);
    const RewardArgs rw = reward_args(h);
    // k_step's preloaded leading arguments (StepHot in rmav_kernels.hpp), then the argument block
    if (h->time_limit > 0)
        hipLaunchKernelGGL((k_step_rw<K, true>), grid, dim3(bs), 0, h->stream, a.state, a.n, a.act_in, a.pitch, (uint32_t)bs, a.flags, a.ep_ret, a.rec, a,
                           kp.p, kp.pc, tl, fa, dr, fs, rw);
    else
        hipLaunchKernelGGL((k_step_rw<K, false>), grid, dim3(bs), 0, h->stream, a.state, a.n, a.act_in, a.pitch, (uint32_t)bs, a.flags, a.ep_ret, a.rec, a,
                           kp.p, kp.pc, tl, fa, dr, fs, rw);
}

}  // namespace

int rmav_launch_reward_rollout(rmav_handle h, int mode, int st, const RolloutArgs &a) {
    return dispatch_kind<QUAD_KINDS>(h->kind, [&](auto k) {
        constexpr int K = decltype(k)::value;
        switch (mode) {
        case ACT_BUFFER: return launch_km<K, ACT_BUFFER>(h, st, a);
        case ACT_RANDOM: return launch_km<K, ACT_RANDOM>(h, st, a);
        case ACT_CONTROLLER: return launch_km<K, ACT_CONTROLLER>(h, st, a);
        }
        return rmav_fail(RMAV_ERR_INVALID, "no tracking-reward kernel for action mode %d", mode);
    });
}

int rmav_launch_reward_step(rmav_handle h, const RolloutArgs &a, int bs, const FinalArgs &fa) {
    return dispatch_kind<QUAD_KINDS>(h->kind, [&](auto k) {
        launch_step<decltype(k)::value>(h, a, bs, fa);
        return (int)RMAV_OK;
    });
}

int rmav_sync_reward_dev(rmav_handle h) {
    hipLaunchKernelGGL(k_set_reward, dim3(1), dim3(64), 0, h->stream, reinterpret_cast<float *>(h->reward_dev), reward_args(h));
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

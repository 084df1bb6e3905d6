// rmav_disturb_abi.hip - the launches of a handle with a wind / gust disturbance (rmav_set_disturbance; include/rmav.h): the single-step
// kernels k_step_ds, the one-wavefront fused rollouts k_rollout_ds and k_disturbance_now.  A translation unit of its own, as
// rmav_reward_abi.hip and for its reason; rmav_abi.hip decides what a call launches and comes here only for the launch itself.
#include "rmav_handle.hpp"

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

// the handle's reward choice as std::integral_constant<bool, RW>: the kernels take it as a template parameter
template <typename F> int dispatch_reward(rmav_handle h, F &&f) {
    if (h->reward_on) return f(std::true_type{});
    return f(std::false_type{});
}

template <int K, int MODE> int launch_km(rmav_handle h, const RolloutArgs &a) {
    const KindParams<K> kp = kind_params<K>(h);
    const int64_t count = a.slice_count ? (int64_t)a.slice_count : h->n;
    const dim3 grid((unsigned)((count + block_size(h) - 1) / block_size(h))), block(block_size(h));
    const TimeLimitArgs tl = tl_args(h);
    const RangeArgs dr = range_args(h);
    const FrameSkipArgs fs = skip_args(h);
    const RewardArgs rw = reward_args(h);
    const DisturbArgs ds = disturb_args(h, a.t0);
    return dispatch_reward(h, [&](auto r) {
        constexpr bool RW = decltype(r)::value;
        if (h->time_limit > 0) hipLaunchKernelGGL((k_rollout_ds<K, MODE, true, RW>), grid, block, 0, h->stream, a, kp.p, kp.pc, tl, dr, fs, rw, ds);
        else hipLaunchKernelGGL((k_rollout_ds<K, MODE, false, RW>), grid, block, 0, h->stream, a, kp.p, kp.pc, tl, dr, fs, rw, ds);
        return (int)RMAV_OK;
    });
}

template <int K> int launch_step(rmav_handle h, const RolloutArgs &a, int bs, const FinalArgs &fa) {
    const KindParams<K> kp = kind_params<K>(h);
    const dim3 grid((unsigned)((h->n + bs - 1) / bs));
    const TimeLimitArgs tl = tl_args(h);
    const RangeArgs dr = range_args(h);
    const FrameSkipArgs fs = skip_args(h);
    const RewardArgs rw = reward_args(h);
    const DisturbArgs ds = disturb_args(h, a.t0);
    // k_step's preloaded leading arguments (StepHot in rmav_kernels.hpp), then the argument block
    return dispatch_reward(h, [&](auto r) {
        constexpr bool RW = decltype(r)::value;
        if (h->time_limit > 0)
            hipLaunchKernelGGL((k_step_ds<K, true, RW>), grid, dim3(bs), 0, h->stream, a.state, a.n, a.act_in, a.pitch, (uint32_t)bs, a.flags, a.ep_ret, a.rec, a,
                               kp.p, kp.pc, tl, fa, dr, fs, rw, ds);
        else
            hipLaunchKernelGGL((k_step_ds<K, false, RW>), grid, dim3(bs), 0, h->stream, a.state, a.n, a.act_in, a.pitch, (uint32_t)bs, a.flags, a.ep_ret, a.rec, a,
                               kp.p, kp.pc, tl, fa, dr, fs, rw, ds);
        return (int)RMAV_OK;
    });
}

}  // namespace

int rmav_launch_disturb_rollout(rmav_handle h, int mode, const RolloutArgs &a) {
    return dispatch_kind<QUAD_KINDS>(h->kind, [&](auto k) {
        constexpr int K = decltype(k)::value;
        switch (mode) {
        case ACT_BUFFER: return launch_km<K, ACT_BUFFER>(h, a);
        case ACT_RANDOM: return launch_km<K, ACT_RANDOM>(h, a);
        case ACT_CONTROLLER: return launch_km<K, ACT_CONTROLLER>(h, a);
        }
        return rmav_fail(RMAV_ERR_INVALID, "no disturbed kernel for action mode %d", mode);
    });
}

int rmav_launch_disturb_step(rmav_handle h, const RolloutArgs &a, int bs, const FinalArgs &fa) {
    return dispatch_kind<QUAD_KINDS>(h->kind, [&](auto k) { return launch_step<decltype(k)::value>(h, a, bs, fa); });
}

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

// rmav_sensor_abi.hip - the launches of a handle with sensor noise (rmav_set_sensor_noise; include/rmav.h): the single-step kernels
// k_step_sn, the one-wavefront fused rollouts k_rollout_sn and k_observe.  A translation unit of its own, as rmav_disturb_abi.hip and for
// its reason; rmav_abi.hip decides what a call launches and comes here only for the launch itself.
#include "rmav_handle.hpp"

using namespace rmav;

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
    const DisturbArgs ds = disturb_or_calm(h, a.t0);
    const SensorArgs sn = sensor_args(h);
    return dispatch_reward(h, [&](auto r) {
        constexpr bool RW = decltype(r)::value;
        if (h->time_limit > 0) hipLaunchKernelGGL((k_rollout_sn<K, MODE, true, RW>), grid, block, 0, h->stream, a, kp.p, kp.pc, tl, dr, fs, rw, ds, sn);
        else hipLaunchKernelGGL((k_rollout_sn<K, MODE, false, RW>), grid, block, 0, h->stream, a, kp.p, kp.pc, tl, dr, fs, rw, ds, sn);
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
    const DisturbArgs ds = disturb_or_calm(h, a.t0);
    const SensorArgs sn = sensor_args(h);
    // k_step's preloaded leading arguments (StepHot in rmav_kernels.hpp), then the argument block
    return dispatch_reward(h, [&](auto r) {
        constexpr bool RW = decltype(r)::value;
        if (h->time_limit > 0)
            hipLaunchKernelGGL((k_step_sn<K, true, RW>), grid, dim3(bs), 0, h->stream, a.state, a.n, a.act_in, a.pitch, (uint32_t)bs, a.flags, a.ep_ret, a.rec, a,
                               kp.p, kp.pc, tl, fa, dr, fs, rw, ds, sn);
        else
            hipLaunchKernelGGL((k_step_sn<K, false, RW>), grid, dim3(bs), 0, h->stream, a.state, a.n, a.act_in, a.pitch, (uint32_t)bs, a.flags, a.ep_ret, a.rec, a,
                               kp.p, kp.pc, tl, fa, dr, fs, rw, ds, sn);
        return (int)RMAV_OK;
    });
}

}  // namespace

int rmav_launch_sensor_rollout(rmav_handle h, int mode, const RolloutArgs &a) {
    return dispatch_kind<QUAD_KINDS>(h->kind, [&](auto k) {
        constexpr int K = decltype(k)::value;
        switch (mode) {
        case ACT_BUFFER: return launch_km<K, ACT_BUFFER>(h, a);
        case ACT_RANDOM: return launch_km<K, ACT_RANDOM>(h, a);
        case ACT_CONTROLLER: return launch_km<K, ACT_CONTROLLER>(h, a);
        }
        return rmav_fail(RMAV_ERR_INVALID, "no sensor-noise kernel for action mode %d", mode);
    });
}

int rmav_launch_sensor_step(rmav_handle h, const RolloutArgs &a, int bs, const FinalArgs &fa) {
    return dispatch_kind<QUAD_KINDS>(h->kind, [&](auto k) { return launch_step<decltype(k)::value>(h, a, bs, fa); });
}

int rmav_launch_observe(rmav_handle h, float *out_dev, int layout) {
    const SensorArgs sn = sensor_args(h);
    const int rc = dispatch_kind<QUAD_KINDS>(h->kind, [&](auto k) {
        hipLaunchKernelGGL((k_observe<decltype(k)::value>), dim3((unsigned)((h->n + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, (const float *)h->state, out_dev,
                           h->n, h->seed, h->env_base, h->t, layout == RMAV_AOS ? 1u : 0u, sn);
        return (int)RMAV_OK;
    });
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

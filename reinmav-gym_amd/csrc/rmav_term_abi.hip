// rmav_term_abi.hip - the launches of a handle with a termination spec (rmav_set_termination; include/rmav.h): the single-step kernels
// k_step_tc, the one-wavefront fused rollouts k_rollout_tc, and the small kernel that keeps the handle's device copy of the thresholds,
// k_set_termination.  A translation unit of its own, as rmav_start_abi.hip and for its reason; rmav_abi.hip decides what a call launches
// and comes here only for the launch itself.
#include "rmav_handle.hpp"

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
    const ActuatorArgs al = start_actuator_args(h);
    const StartArgs ss = term_start_args(h);
    const TermArgs tc = term_args(h);
    return dispatch_reward(h, [&](auto r) {
        constexpr bool RW = decltype(r)::value;
        if (h->time_limit > 0) hipLaunchKernelGGL((k_rollout_tc<K, MODE, true, RW>), grid, block, 0, h->stream, a, kp.p, kp.pc, tl, dr, fs, rw, ds, sn, al, ss, tc);
        else hipLaunchKernelGGL((k_rollout_tc<K, MODE, false, RW>), grid, block, 0, h->stream, a, kp.p, kp.pc, tl, dr, fs, rw, ds, sn, al, ss, tc);
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
    const ActuatorArgs al = start_actuator_args(h);
    const StartArgs ss = term_start_args(h);
    const TermArgs tc = term_args(h);
    // k_step's preloaded leading arguments (StepHot in rmav_kernels.hpp), then the argument block
    return dispatch_reward(h, [&](auto r) {
        constexpr bool RW = decltype(r)::value;
        if (h->time_limit > 0)
            hipLaunchKernelGGL((k_step_tc<K, true, RW>), grid, dim3(bs), 0, h->stream, a.state, a.n, a.act_in, a.pitch, (uint32_t)bs, a.flags, a.ep_ret, a.rec, a,
                               kp.p, kp.pc, tl, fa, dr, fs, rw, ds, sn, al, ss, tc);
        else
            hipLaunchKernelGGL((k_step_tc<K, false, RW>), grid, dim3(bs), 0, h->stream, a.state, a.n, a.act_in, a.pitch, (uint32_t)bs, a.flags, a.ep_ret, a.rec, a,
                               kp.p, kp.pc, tl, fa, dr, fs, rw, ds, sn, al, ss, tc);
        return (int)RMAV_OK;
    });
}

}  // namespace

int rmav_launch_term_rollout(rmav_handle h, int mode, const RolloutArgs &a) {
    return dispatch_kind<QUAD_KINDS>(h->kind, [&](auto k) {
        constexpr int K = decltype(k)::value;
        switch (mode) {
        case ACT_BUFFER: return launch_km<K, ACT_BUFFER>(h, a);
        case ACT_RANDOM: return launch_km<K, ACT_RANDOM>(h, a);
        case ACT_CONTROLLER: return launch_km<K, ACT_CONTROLLER>(h, a);
        }
        return rmav_fail(RMAV_ERR_INVALID, "no termination kernel for action mode %d", mode);
    });
}

int rmav_launch_term_step(rmav_handle h, const RolloutArgs &a, int bs, const FinalArgs &fa) {
    return dispatch_kind<QUAD_KINDS>(h->kind, [&](auto k) { return launch_step<decltype(k)::value>(h, a, bs, fa); });
}

int rmav_sync_term_dev(rmav_handle h) {
    hipLaunchKernelGGL(k_set_termination, dim3(1), dim3(64), 0, h->stream, reinterpret_cast<uint32_t *>(h->term_dev), term_args(h), (uint32_t)kCalmHold);
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

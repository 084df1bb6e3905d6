// rmav_actuator_abi.hip - the launches of a handle with actuator lag (rmav_set_actuator; include/rmav.h): the single-step kernels k_step_al,
// the one-wavefront fused rollouts k_rollout_al, and the two small kernels that keep the handle's device data: k_actuator_fill (every env's
// m = init) and k_set_actuator (the policy kernels' copy of the coefficients).  A translation unit of its own, as rmav_sensor_abi.hip and
// for its reason; rmav_abi.hip decides what a call launches and comes here only for the launch itself.
#include "rmav_handle.hpp"

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
    const ActuatorArgs al = actuator_args(h);
    return dispatch_reward(h, [&](auto r) {
        constexpr bool RW = decltype(r)::value;
        if (h->time_limit > 0) hipLaunchKernelGGL((k_rollout_al<K, MODE, true, RW>), grid, block, 0, h->stream, a, kp.p, kp.pc, tl, dr, fs, rw, ds, sn, al);
        else hipLaunchKernelGGL((k_rollout_al<K, MODE, false, RW>), grid, block, 0, h->stream, a, kp.p, kp.pc, tl, dr, fs, rw, ds, sn, al);
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
    const ActuatorArgs al = actuator_args(h);
    // k_step's preloaded leading arguments (StepHot in rmav_kernels.hpp), then the argument block
    return dispatch_reward(h, [&](auto r) {
        constexpr bool RW = decltype(r)::value;
        if (h->time_limit > 0)
            hipLaunchKernelGGL((k_step_al<K, true, RW>), grid, dim3(bs), 0, h->stream, a.state, a.n, a.act_in, a.pitch, (uint32_t)bs, a.flags, a.ep_ret, a.rec, a,
                               kp.p, kp.pc, tl, fa, dr, fs, rw, ds, sn, al);
        else
            hipLaunchKernelGGL((k_step_al<K, false, RW>), grid, dim3(bs), 0, h->stream, a.state, a.n, a.act_in, a.pitch, (uint32_t)bs, a.flags, a.ep_ret, a.rec, a,
                               kp.p, kp.pc, tl, fa, dr, fs, rw, ds, sn, al);
        return (int)RMAV_OK;
    });
}

}  // namespace

int rmav_launch_actuator_rollout(rmav_handle h, int mode, const RolloutArgs &a) {
    return dispatch_kind<QUAD_KINDS>(h->kind, [&](auto k) {
        constexpr int K = decltype(k)::value;
        switch (mode) {
        case ACT_BUFFER: return launch_km<K, ACT_BUFFER>(h, a);
        case ACT_RANDOM: return launch_km<K, ACT_RANDOM>(h, a);
        case ACT_CONTROLLER: return launch_km<K, ACT_CONTROLLER>(h, a);
        }
        return rmav_fail(RMAV_ERR_INVALID, "no actuator-lag kernel for action mode %d", mode);
    });
}

int rmav_launch_actuator_step(rmav_handle h, const RolloutArgs &a, int bs, const FinalArgs &fa) {
    return dispatch_kind<QUAD_KINDS>(h->kind, [&](auto k) { return launch_step<decltype(k)::value>(h, a, bs, fa); });
}

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

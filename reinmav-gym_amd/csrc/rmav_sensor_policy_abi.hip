// rmav_sensor_policy_abi.hip - the policy-in-kernel rollouts of a handle with sensor noise (rmav_set_sensor_noise; include/rmav.h): the three
// actors k_rollout_nrm_sn, k_rollout_pair_sn, k_rollout_pair_shared_sn and k_set_sensor_noise, which keeps the handle's device copy of the spec.  A translation unit of its own
// (the matrix-core kernels compile beside rmav_policy_abi.hip, with its flags); rmav_ppo_abi.hip makes the checks and comes here for the launch.
#include "rmav_policy_rung.hpp"

using namespace rmav;

namespace rmav {

// the handle's device copy (SensorDev): the sixteen sigmas, then the calm disturbance spec - nine zeros and the hold - by vector stores
__global__ __launch_bounds__(64) void k_set_sensor_noise(uint32_t *dst, const SensorArgs v, uint32_t calm_hold) {
    static_assert(sizeof(SensorDev) == 26 * sizeof(uint32_t) && offsetof(SensorDev, calm) == 64 && offsetof(DisturbSpec, hold) == 36, "16 + 9 + 1 words");
    uint32_t x = 0u;
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i) x = (threadIdx.x == i) ? __builtin_bit_cast(uint32_t, v.sigma[i]) : x;
    x = (threadIdx.x == 25u) ? calm_hold : x;
    if (threadIdx.x < 26u) dst[threadIdx.x] = x;
}

}  // namespace rmav

namespace {

struct Kernels {
    template <int K, bool BOOT, bool RW> static auto nrm() { return k_rollout_nrm_sn<K, BOOT, RW>; }
    template <int K, bool BOOT, bool RW> static auto pair() { return k_rollout_pair_sn<K, BOOT, RW>; }
    template <int K, bool BOOT, bool RW> static auto shared() { return k_rollout_pair_shared_sn<K, BOOT, RW>; }
    static auto args(const rmav_env_s *h, uint64_t t0) { return policy_sensor_args(h, t0); }
};

}  // namespace

int rmav_launch_sensor_policy_rollout(rmav_handle h, int kmode, const RolloutArgs &a, const BootArgs *bt, const NormArgs *nm) {
    return launch_policy_rung<RUNG_SENSOR, Kernels>(h, kmode, a, bt, nm);
}

int rmav_sync_sensor_dev(rmav_handle h) {
    hipLaunchKernelGGL(k_set_sensor_noise, dim3(1), dim3(64), 0, h->stream, reinterpret_cast<uint32_t *>(h->sensor_dev), sensor_args(h), (uint32_t)kCalmHold);
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

// rmav_sensor_abi.hip - the launches of a handle with sensor noise (rmav_set_sensor_noise; include/rmav.h): the single-step kernels
// k_step_sn, the one-wavefront fused rollouts k_rollout_sn and k_observe.  A translation unit of its own, as rmav_disturb_abi.hip and for
// its reason; rmav_abi.hip decides what a call launches and comes here only for the launch itself.
#include "rmav_rung_launch.hpp"

using namespace rmav;

namespace {

struct Kernels {
    template <int K, int MODE, int ST, bool TL, bool RW> static auto rollout() { return k_rollout_sn<K, MODE, TL, RW>; }
    template <int K, bool CTRL, bool TL, bool RW> static auto step() { return k_step_sn<K, TL, RW>; }
};

}  // namespace

int rmav_launch_sensor_rollout(rmav_handle h, int mode, int st, const RolloutArgs &a) { return launch_rung_rollout<RUNG_SENSOR, Kernels>(h, mode, st, a); }

int rmav_launch_sensor_step(rmav_handle h, const RolloutArgs &a, bool ctrl, int bs, const FinalArgs &fa) { return launch_rung_step<RUNG_SENSOR, Kernels>(h, a, ctrl, bs, fa); }

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

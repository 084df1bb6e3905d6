// rmav_range_abi.hip - the launches of a handle with a parameter range (rmav_set_env_param_range; include/rmav.h): the single-step
// kernels k_step_dr and the one-wavefront fused rollouts k_rollout_dr.  A translation unit of its own so that these kernels compile
// beside the others instead of lengthening the longest of them; rmav_abi.hip decides what a call launches (action mode, store
// policy, slices) and comes here only for the launch itself.  The ranged policy rollouts are in rmav_policy_abi.hip.
#include "rmav_rung_launch.hpp"

using namespace rmav;

namespace {

struct Kernels {
    template <int K, int MODE, int ST, bool TL, bool RW> static auto rollout() { return k_rollout_dr<K, MODE, ST, TL>; }
    template <int K, bool CTRL, bool TL, bool RW> static auto step() { return k_step_dr<K, CTRL, TL>; }
};

}  // namespace

int rmav_launch_ranged_rollout(rmav_handle h, int mode, int st, const RolloutArgs &a) { return launch_rung_rollout<RUNG_RANGE, Kernels>(h, mode, st, a); }

int rmav_launch_ranged_step(rmav_handle h, const RolloutArgs &a, bool ctrl, int bs, const FinalArgs &fa) { return launch_rung_step<RUNG_RANGE, Kernels>(h, a, ctrl, bs, fa); }

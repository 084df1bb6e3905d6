// rmav_skip_abi.hip - the launches of a handle with a frame skip (rmav_set_frame_skip; include/rmav.h): the single-step kernels k_step_fs
// and the one-wavefront fused rollouts k_rollout_fs.  A translation unit of its own, as rmav_range_abi.hip and for its reason;
// rmav_abi.hip decides what a call launches and comes here only for the launch itself.  The frame-skip policy rollouts are in
// rmav_policy_abi.hip.
#include "rmav_rung_launch.hpp"

using namespace rmav;

namespace {

struct Kernels {
    template <int K, int MODE, int ST, bool TL, bool RW> static auto rollout() { return k_rollout_fs<K, MODE, ST, TL>; }
    template <int K, bool CTRL, bool TL, bool RW> static auto step() { return k_step_fs<K, TL>; }
};

}  // namespace

int rmav_launch_skip_rollout(rmav_handle h, int mode, int st, const RolloutArgs &a) { return launch_rung_rollout<RUNG_SKIP, Kernels>(h, mode, st, a); }

int rmav_launch_skip_step(rmav_handle h, const RolloutArgs &a, bool ctrl, int bs, const FinalArgs &fa) { return launch_rung_step<RUNG_SKIP, Kernels>(h, a, ctrl, bs, fa); }

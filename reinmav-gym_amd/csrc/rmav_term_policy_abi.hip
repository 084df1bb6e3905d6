// rmav_term_policy_abi.hip - the policy-in-kernel rollouts of a handle with a termination spec (rmav_set_termination; include/rmav.h): the
// three actors k_rollout_nrm_tc, k_rollout_pair_tc, k_rollout_pair_shared_tc.  A translation unit of its own (the matrix-core kernels
// compile beside rmav_start_policy_abi.hip, with its flags); rmav_ppo_abi.hip makes the checks and comes here for the launch.
#include "rmav_policy_rung.hpp"

using namespace rmav;

namespace {

struct Kernels {
    template <int K, bool BOOT, bool RW> static auto nrm() { return k_rollout_nrm_tc<K, BOOT, RW>; }
    template <int K, bool BOOT, bool RW> static auto pair() { return k_rollout_pair_tc<K, BOOT, RW>; }
    template <int K, bool BOOT, bool RW> static auto shared() { return k_rollout_pair_shared_tc<K, BOOT, RW>; }
    static auto args(const rmav_env_s *h, uint64_t t0) { return policy_term_args(h, t0); }
};

}  // namespace

int rmav_launch_term_policy_rollout(rmav_handle h, int kmode, const RolloutArgs &a, const BootArgs *bt, const NormArgs *nm) {
    return launch_policy_rung<RUNG_TERM, Kernels>(h, kmode, a, bt, nm);
}

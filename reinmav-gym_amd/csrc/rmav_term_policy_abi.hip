// rmav_term_policy_abi.hip - the policy-in-kernel rollouts of a handle with a termination spec (rmav_set_termination; include/rmav.h): the
// three actors k_rollout_nrm_tc, k_rollout_pair_tc, k_rollout_pair_shared_tc.  A translation unit of its own (the matrix-core kernels
// compile beside rmav_start_policy_abi.hip, with its flags); rmav_ppo_abi.hip makes the checks and comes here for the launch.
#include "rmav_handle.hpp"
#include "rmav_policy_pair.hpp"

using namespace rmav;

namespace {

// what the three actors' launches differ in (rmav_policy_abi.hip's families, for the one slot a handle with a termination spec runs)
struct Shape {
    int envs_per_word;
    int64_t envs;       // per workgroup
    unsigned threads;
    size_t lds;
};
// pairs of one workgroup: RMAV_TUNE_PAIR_GROUP = 1 .. 4 overrides what was measured (rmav_policy_abi.hip: pairs_per_workgroup)
inline int pair_group(rmav_handle h, int measured) {
    const int forced = h->tune[RMAV_TUNE_PAIR_GROUP];
    return (forced >= 1 && forced <= kPairGroupMax) ? forced : measured;
}
constexpr size_t kNormBytes = sizeof(float) * kNormWords;   // the normaliser's tables, in LDS behind the weights

template <int K> int launch_k(rmav_handle h, int kmode, const RolloutArgs &a_in, const BootArgs *bt, const NormArgs *nm) {
    const bool limited = h->time_limit > 0;   // (the BOOT kernels: their tiles carry the terminal area)
    Shape sh{};
    if (kmode == ACT_POLICY_F32M) {   // both half-waves of the fp32 matrix-core actor work on the same 32 envs
        sh = {32, block_size(h) / 2, (unsigned)block_size(h), sizeof(float) * (size_t)Mfma32Layout::TOTAL + kNormBytes};
    } else if (kmode == ACT_POLICY_F16) {
        const int g = pair_group(h, h->n <= 98304 ? 4 : 2);
        sh = {64, 64 * g, 128u * g, (limited ? pair_boot_lds_bytes<K>(g) : pair_lds_bytes<K>(g)) + kNormBytes};
    } else {
        const int g = pair_group(h, 2);
        sh = {64, 64 * g, 128u * g, (limited ? shared_boot_lds_bytes<K>(g) : shared_lds_bytes<K>(g)) + kNormBytes};
    }
    RolloutArgs a = a_in;
    take_armed_exchange(h, a, sh.envs_per_word);
    const KindParams<K> kp = kind_params<K>(h);
    const dim3 grid((unsigned)((h->n + sh.envs - 1) / sh.envs)), block(sh.threads);
    const TimeLimitArgs tl = limited ? tl_args(h) : TimeLimitArgs{};
    const BootArgs b = (limited && bt) ? *bt : BootArgs{};
    const PolicyTermArgs ps = policy_term_args(h, a.t0);
    // the handle's time limit and reward choice as template parameters of the kernels
    auto with = [&](auto f) {
        if (limited) h->reward_on ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
        else h->reward_on ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
    };
    if (kmode == ACT_POLICY_F32M) {
        a.act_in = nm->tab;   // the tables travel in RolloutArgs::act_in and the range by device pointer, as for k_rollout_nrm_ss
        with([&](auto bo, auto rw) {
            hipLaunchKernelGGL((k_rollout_nrm_tc<K, decltype(bo)::value, decltype(rw)::value>), grid, block, sh.lds, h->stream, a, kp.p, kp.pc, tl, b,
                               (const RangeArgs *)h->range_dev, ps);
        });
    } else if (kmode == ACT_POLICY_F16) {
        with([&](auto bo, auto rw) {
            hipLaunchKernelGGL((k_rollout_pair_tc<K, decltype(bo)::value, decltype(rw)::value>), grid, block, sh.lds, h->stream, a, kp.p, kp.pc, tl, b, *nm,
                               range_args(h), ps);
        });
    } else {
        with([&](auto bo, auto rw) {
            hipLaunchKernelGGL((k_rollout_pair_shared_tc<K, decltype(bo)::value, decltype(rw)::value>), grid, block, sh.lds, h->stream, a, kp.p, kp.pc, tl, b,
                               *nm, range_args(h), ps);
        });
    }
    return check_rollout_launch(h, a);
}

}  // namespace

int rmav_launch_term_policy_rollout(rmav_handle h, int kmode, const RolloutArgs &a, const BootArgs *bt, const NormArgs *nm) {
    if (kmode != ACT_POLICY_F32M && kmode != ACT_POLICY_F16 && kmode != ACT_POLICY_F16_SHARED)
        return rmav_fail(RMAV_ERR_INVALID, "no termination kernel for policy mode %d", kmode);
    if (!nm || (h->time_limit > 0 && !bt)) return rmav_fail(RMAV_ERR_INVALID, "a handle with a termination spec runs the normalised kernels");
    return dispatch_kind<QUAD_KINDS>(h->kind, [&](auto k) { return launch_k<decltype(k)::value>(h, kmode, a, bt, nm); });
}

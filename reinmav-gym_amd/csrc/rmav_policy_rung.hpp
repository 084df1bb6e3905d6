// rmav_policy_rung.hpp - what the four policy units above the disturbance rung (rmav_sensor_policy_abi.hip ... rmav_term_policy_abi.hip)
// share: the launch of the one slot such a handle runs, for the three actors.  A unit names its kernels and its argument provider in a struct
//     struct Kernels {
//         template <int K, bool BOOT, bool RW> static auto nrm() { return k_rollout_nrm_xx<K, BOOT, RW>; }           // the fp32 matrix-core actor
//         template <int K, bool BOOT, bool RW> static auto pair() { return k_rollout_pair_xx<K, BOOT, RW>; }         // the f16 pair
//         template <int K, bool BOOT, bool RW> static auto shared() { return k_rollout_pair_shared_xx<K, BOOT, RW>; } // the shared-trunk pair
//         static auto args(const rmav_env_s *h, uint64_t t0) { return policy_xx_args(h, t0); }
//     };
// and forwards its rmav_launch_*_policy_rollout to launch_policy_rung.
#pragma once

#include "rmav_ladder.hpp"
#include "rmav_policy_pair.hpp"

// what the three actors' launches differ in (rmav_policy_abi.hip's families)
struct PolicyRungShape {
    int envs_per_word;
    int64_t envs;       // per workgroup
    unsigned threads;
    size_t lds;
};
// pairs of one workgroup: RMAV_TUNE_PAIR_GROUP = 1 .. 4 overrides what was measured (rmav_policy_abi.hip: pairs_per_workgroup)
inline int policy_rung_pair_group(rmav_handle h, int measured) {
    const int forced = h->tune[RMAV_TUNE_PAIR_GROUP];
    return (forced >= 1 && forced <= rmav::kPairGroupMax) ? forced : measured;
}

template <typename KN, int K>
RMAV_INTERNAL inline int launch_policy_rung_k(rmav_handle h, int kmode, const rmav::RolloutArgs &a_in, const rmav::BootArgs *bt, const rmav::NormArgs *nm) {
    using namespace rmav;
    constexpr size_t kNormBytes = sizeof(float) * kNormWords;   // the normaliser's tables, in LDS behind the weights
    const bool limited = h->time_limit > 0;   // (the BOOT kernels: their tiles carry the terminal area)
    PolicyRungShape sh{};
    if (kmode == ACT_POLICY_F32M) {   // both half-waves of the fp32 matrix-core actor work on the same 32 envs
        sh = {32, block_size(h) / 2, (unsigned)block_size(h), sizeof(float) * (size_t)Mfma32Layout::TOTAL + kNormBytes};
    } else if (kmode == ACT_POLICY_F16) {
        const int g = policy_rung_pair_group(h, h->n <= 98304 ? 4 : 2);
        sh = {64, 64 * g, 128u * g, (limited ? pair_boot_lds_bytes<K>(g) : pair_lds_bytes<K>(g)) + kNormBytes};
    } else {
        const int g = policy_rung_pair_group(h, 2);
        sh = {64, 64 * g, 128u * g, (limited ? shared_boot_lds_bytes<K>(g) : shared_lds_bytes<K>(g)) + kNormBytes};
    }
    RolloutArgs a = a_in;
    take_armed_exchange(h, a, sh.envs_per_word);
    const KindParams<K> kp = kind_params<K>(h);
    const dim3 grid((unsigned)((h->n + sh.envs - 1) / sh.envs)), block(sh.threads);
    const TimeLimitArgs tl = limited ? tl_args(h) : TimeLimitArgs{};
    const BootArgs b = (limited && bt) ? *bt : BootArgs{};
    const auto ps = KN::args(h, a.t0);
    // the handle's time limit and reward choice as template parameters of the kernels
    auto with = [&](auto f) {
        if (limited) h->reward_on ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
        else h->reward_on ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
    };
    if (kmode == ACT_POLICY_F32M) {
        a.act_in = nm->tab;   // the tables travel in RolloutArgs::act_in and the range by device pointer, as for k_rollout_nrm_ds
        with([&](auto bo, auto rw) {
            hipLaunchKernelGGL((KN::template nrm<K, decltype(bo)::value, decltype(rw)::value>()), grid, block, sh.lds, h->stream, a, kp.p, kp.pc, tl, b,
                               (const RangeArgs *)h->range_dev, ps);
        });
    } else if (kmode == ACT_POLICY_F16) {
        with([&](auto bo, auto rw) {
            hipLaunchKernelGGL((KN::template pair<K, decltype(bo)::value, decltype(rw)::value>()), grid, block, sh.lds, h->stream, a, kp.p, kp.pc, tl, b, *nm,
                               range_args(h), ps);
        });
    } else {
        with([&](auto bo, auto rw) {
            hipLaunchKernelGGL((KN::template shared<K, decltype(bo)::value, decltype(rw)::value>()), grid, block, sh.lds, h->stream, a, kp.p, kp.pc, tl, b, *nm,
                               range_args(h), ps);
        });
    }
    return check_rollout_launch(h, a);
}

// rmav_launch_policy_rollout's arguments; nm is required, bt on a time-limited handle (rmav_ppo_abi.hip passes the handle's own where the
// caller gave none)
template <Rung R, typename KN>
RMAV_INTERNAL inline int launch_policy_rung(rmav_handle h, int kmode, const rmav::RolloutArgs &a, const rmav::BootArgs *bt, const rmav::NormArgs *nm) {
    if (kmode != rmav::ACT_POLICY_F32M && kmode != rmav::ACT_POLICY_F16 && kmode != rmav::ACT_POLICY_F16_SHARED)
        return rmav_fail(RMAV_ERR_INVALID, "no %s kernel for policy mode %d", kLadder[R].noun, kmode);
    if (!nm || (h->time_limit > 0 && !bt)) return rmav_fail(RMAV_ERR_INVALID, "%s runs the normalised kernels", kLadder[R].handle);
    return dispatch_kind<QUAD_KINDS>(h->kind, [&](auto k) { return launch_policy_rung_k<KN, decltype(k)::value>(h, kmode, a, bt, nm); });
}

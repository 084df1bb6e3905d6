// rmav_policy_abi.hip - launches of the policy-in-kernel rollouts (rmav_rollout_policy / _boot / _norm, whose entry points and checks are
// in rmav_ppo_abi.hip): the unit that holds the matrix-core kernels.
//
// Compiled with -fno-slp-vectorize, as every unit of librmav.so since round 5.  hipcc's SLP vectoriser packs adjacent scalar fp32 operations of the dynamics into
// v_pk_mul / v_pk_fma / v_pk_add_f32 with cross-register op_sel selects, among them `v_pk_fma_f32 D, P, Q, D op_sel:[0,1,0]`
// (quat_body_z).  On gfx950 the operand that op_sel[1] = 1 selects - the HIGH dword of src1 for the LOW result - reads as ZERO in
// lanes 48..63 while a v_mfma_f32_32x32x16_{f16,bf16} of any wavefront executes on the same SIMD: the x-axis thrust term of
// quadrotor3d's step was lost in 1 - 25 % of the wavefronts of a rollout, never with one wavefront per SIMD (three rounds of parity
// tests at BASELINE sizes were green).  Root cause, wait-state sweep (they do not help), flag A/B (the stock build fails as
// well) and the 148-line stand-alone reproducer: profiles/r05/packed_f32_hazard.md, tools/micro/pk_hazard.hip.  The Makefile
// disassembles every object and refuses to build one that contains the form (`check_isa`);
// tests/test_gpu_ppo.py::test_matrix_core_actors_are_deterministic and tests/test_resource_usage.py guard it as well.
#include "rmav_handle.hpp"
#include "rmav_policy_pair.hpp"

using namespace rmav;

namespace {

// Which of an actor's kernels a launch runs.  A handle with a time limit takes the time-limited kernel, the *_boot one when the call
// wants the bootstrap term (bt); rmav_rollout_policy_norm (nm) takes the *_nrm kernels, whose BOOT variant is the one of a handle with
// a time limit (bt is required there).  Only the three actors a time-limited handle accepts - fp32-MFMA, f16 pair, shared-trunk pair,
// on a quadrotor kind - have other kernels than the plain one.
enum PolicyVariant { V_PLAIN, V_TL, V_BOOT, V_NRM, V_NRM_BOOT };
inline PolicyVariant policy_variant(rmav_handle h, const BootArgs *bt, const NormArgs *nm) {
    const bool limited = h->time_limit > 0;
    return nm ? (limited ? V_NRM_BOOT : V_NRM) : limited ? (bt ? V_BOOT : V_TL) : V_PLAIN;
}
// the trailing arguments of those kernels: zero where the variant does not read them
inline TimeLimitArgs variant_tl(rmav_handle h) { return h->time_limit > 0 ? tl_args(h) : TimeLimitArgs{}; }
inline BootArgs variant_boot(rmav_handle h, const BootArgs *bt) { return (h->time_limit > 0 && bt) ? *bt : BootArgs{}; }
constexpr size_t kNormBytes = sizeof(float) * kNormWords;   // the *_nrm kernels' tables, in LDS behind the weights

// ---- the three actor families -------------------------------------------------------------------------------------------------------
// A family names its kernels once - plain(), tl(), boot(), nrm<BOOT>, dr<BOOT>, fs<BOOT>, rw<BOOT>, ds<BOOT, RW>: the fifteen slots (the last twelve take the handle's
// action rule, act_rule_args: the identity unless rmav_set_policy_action_rule said otherwise) - and says what differs between the
// families around them: envs behind one arrival word, the workgroup (pairs sharing one LDS copy of the weights, envs, threads), the LDS
// bytes, and how the *_nrm / *_dr kernels take the tables and the range.  kVariants = false: the plain kernel is the only one.
struct Workgroup {
    int pairs;
    int64_t envs;
    unsigned threads;
};
struct VariantArgs {   // what the kernels take behind (a, p, pc); nm is set in the nrm / dr slots
    rmav_handle h;
    RolloutArgs &a;
    TimeLimitArgs tl;
    BootArgs b;
    const NormArgs *nm;
};

// one wavefront per 64 envs (32 for the fp32-MFMA actor: both half-waves work on the same 32 envs)
// (time-limited handles: k_rollout_tl, ACT_POLICY_F32M only - rmav_rollout_policy refuses the other one-wavefront actors)
template <int KIND, int MODE> struct OneWave {
    static constexpr int K = KIND, kEnvsPerWord = MODE == ACT_POLICY_F32M ? 32 : 64;
    static constexpr bool kVariants = K != REINMAV && MODE == ACT_POLICY_F32M;
    static Workgroup workgroup(rmav_handle h) { return {1, MODE == ACT_POLICY_F32M ? block_size(h) / 2 : block_size(h), (unsigned)block_size(h)}; }
    static size_t lds_bytes(int, bool, bool tables) {
        return sizeof(float) * (MODE == ACT_POLICY ? (size_t)PolicyLayout<Dims<K>::NS>::TOTAL
                                : MODE == ACT_POLICY_BF16 ? (size_t)MfmaLayout::TOTAL : (size_t)Mfma32Layout::TOTAL) + (tables ? kNormBytes : 0);
    }
    static auto plain() { return k_rollout<K, MODE, ST_DEFAULT>; }
    static auto tl() { return k_rollout_tl<K, MODE, ST_DEFAULT>; }
    static auto boot() { return k_rollout_boot<K, MODE, ST_DEFAULT>; }
    // the tables travel in RolloutArgs::act_in and the range by device pointer (see the kernels)
    template <bool BOOT, typename Go> static void nrm(Go go, const VariantArgs &v) { v.a.act_in = v.nm->tab, go(k_rollout_nrm<K, BOOT>, v.tl, v.b, act_rule_args(v.h)); }
    template <bool BOOT, typename Go> static void dr(Go go, const VariantArgs &v) {
        v.a.act_in = v.nm->tab, go(k_rollout_nrm_dr<K, BOOT>, v.tl, v.b, (const RangeArgs *)v.h->range_dev, act_rule_args(v.h));
    }
    template <bool BOOT, typename Go> static void fs(Go go, const VariantArgs &v) {
        v.a.act_in = v.nm->tab, go(k_rollout_nrm_fs<K, BOOT>, v.tl, v.b, (const RangeArgs *)v.h->range_dev, policy_skip_args(v.h));
    }
    template <bool BOOT, typename Go> static void rw(Go go, const VariantArgs &v) {
        v.a.act_in = v.nm->tab, go(k_rollout_nrm_rw<K, BOOT>, v.tl, v.b, (const RangeArgs *)v.h->range_dev, policy_reward_args(v.h));
    }
    template <bool BOOT, bool RW, typename Go> static void ds(Go go, const VariantArgs &v) {
        v.a.act_in = v.nm->tab, go(k_rollout_nrm_ds<K, BOOT, RW>, v.tl, v.b, (const RangeArgs *)v.h->range_dev, policy_disturb_args(v.h, v.a.t0));
    }
};

// The matrix-core actors as (actor, critic) wavefront pairs (rmav_policy_pair.hpp).  Pairs per workgroup: the pairs of a
// workgroup share one LDS copy of the weights (30 KB) but also one s_barrier; RMAV_TUNE_PAIR_GROUP = 1 .. 4 overrides.
// (The *_boot kernels' larger tiles - pair_boot_lds_bytes / shared_boot_lds_bytes - fit the 160 KiB of a workgroup at every group
// count: 4 pairs of the 16-state kind take 113 KiB / 101 KiB.)
static_assert(pair_boot_lds_bytes<QUAD3D_SL>(kPairGroupMax) + kNormBytes <= (160u << 10) &&
                  shared_boot_lds_bytes<QUAD3D_SL>(kPairGroupMax) + kNormBytes <= (160u << 10),
              "the hand-over tiles with their terminal-state areas must fit one workgroup's LDS");
inline Workgroup pairs_per_workgroup(rmav_handle h, int measured) {
    const int forced = h->tune[RMAV_TUNE_PAIR_GROUP];
    const int g = (forced >= 1 && forced <= kPairGroupMax) ? forced : measured;
    return {g, 64 * g, 128u * g};
}
template <int KIND, int FMT> struct Pair {   // (time-limited handles: RMAV_POLICY_F16_MFMA only)
    static constexpr int K = KIND, kEnvsPerWord = 64;
    static constexpr bool kVariants = K != REINMAV && FMT == FMT_F16;
    // measured (profiles/r04/actor_bench.txt, quadrotor3d x 32 steps): 65 536 envs 4 pairs 15.0 G env-steps/s, 2 pairs 14.1, 1 pair 13.7
    // (one workgroup per CU, weights staged once per CU); 131 072 envs 2 pairs 15.8 - 16.7, 4 pairs 15.5 - 16.3, 1 pair 11.1
    static Workgroup workgroup(rmav_handle h) { return pairs_per_workgroup(h, h->n <= 98304 ? 4 : 2); }
    static size_t lds_bytes(int g, bool boot_tiles, bool tables) { return (boot_tiles ? pair_boot_lds_bytes<K>(g) : pair_lds_bytes<K>(g)) + (tables ? kNormBytes : 0); }
    static auto plain() { return k_rollout_pair<K, FMT>; }
    static auto tl() { return k_rollout_pair_tl<K, FMT>; }
    static auto boot() { return k_rollout_pair_boot<K, FMT>; }
    template <bool BOOT, typename Go> static void nrm(Go go, const VariantArgs &v) { go(k_rollout_pair_nrm<K, BOOT>, v.tl, v.b, *v.nm, act_rule_args(v.h)); }
    template <bool BOOT, typename Go> static void dr(Go go, const VariantArgs &v) { go(k_rollout_pair_dr<K, BOOT>, v.tl, v.b, *v.nm, range_args(v.h), act_rule_args(v.h)); }
    template <bool BOOT, typename Go> static void fs(Go go, const VariantArgs &v) { go(k_rollout_pair_fs<K, BOOT>, v.tl, v.b, *v.nm, range_args(v.h), policy_skip_args(v.h)); }
    template <bool BOOT, typename Go> static void rw(Go go, const VariantArgs &v) { go(k_rollout_pair_rw<K, BOOT>, v.tl, v.b, *v.nm, range_args(v.h), policy_reward_args(v.h)); }
    template <bool BOOT, bool RW, typename Go> static void ds(Go go, const VariantArgs &v) {
        go(k_rollout_pair_ds<K, BOOT, RW>, v.tl, v.b, *v.nm, range_args(v.h), policy_disturb_args(v.h, v.a.t0));
    }
};

// RMAV_POLICY_F16_SHARED: one trunk, both wavefronts of a pair evaluate it for one 32-env column tile each (k_rollout_pair_shared)
template <int KIND> struct SharedPair {
    static constexpr int K = KIND, kEnvsPerWord = 64;
    static constexpr bool kVariants = K != REINMAV;
    // measured (profiles/r04/actor_bench.txt): 65 536 envs 1 / 2 / 4 pairs per workgroup 20.8 / 21.5 / 20.4 G env-steps/s, 131 072: 19.9 / 25.9 / 26.1
    static Workgroup workgroup(rmav_handle h) { return pairs_per_workgroup(h, 2); }
    static size_t lds_bytes(int g, bool boot_tiles, bool tables) { return (boot_tiles ? shared_boot_lds_bytes<K>(g) : shared_lds_bytes<K>(g)) + (tables ? kNormBytes : 0); }
    static auto plain() { return k_rollout_pair_shared<K>; }
    static auto tl() { return k_rollout_pair_shared_tl<K>; }
    static auto boot() { return k_rollout_pair_shared_boot<K>; }
    template <bool BOOT, typename Go> static void nrm(Go go, const VariantArgs &v) { go(k_rollout_pair_shared_nrm<K, BOOT>, v.tl, v.b, *v.nm, act_rule_args(v.h)); }
    template <bool BOOT, typename Go> static void dr(Go go, const VariantArgs &v) { go(k_rollout_pair_shared_dr<K, BOOT>, v.tl, v.b, *v.nm, range_args(v.h), act_rule_args(v.h)); }
    template <bool BOOT, typename Go> static void fs(Go go, const VariantArgs &v) { go(k_rollout_pair_shared_fs<K, BOOT>, v.tl, v.b, *v.nm, range_args(v.h), policy_skip_args(v.h)); }
    template <bool BOOT, typename Go> static void rw(Go go, const VariantArgs &v) { go(k_rollout_pair_shared_rw<K, BOOT>, v.tl, v.b, *v.nm, range_args(v.h), policy_reward_args(v.h)); }
    template <bool BOOT, bool RW, typename Go> static void ds(Go go, const VariantArgs &v) {
        go(k_rollout_pair_shared_ds<K, BOOT, RW>, v.tl, v.b, *v.nm, range_args(v.h), policy_disturb_args(v.h, v.a.t0));
    }
};

// ---- the one ladder: which of family F's kernels this launch runs, with which LDS size and trailing arguments ---------------------------
template <typename F> int launch_family(rmav_handle h, const RolloutArgs &a_in, const BootArgs *bt, const NormArgs *nm) {
    RolloutArgs a = a_in;
    take_armed_exchange(h, a, F::kEnvsPerWord);
    const KindParams<F::K> kp = kind_params<F::K>(h);
    const Workgroup wg = F::workgroup(h);
    const dim3 grid((unsigned)((h->n + wg.envs - 1) / wg.envs)), block(wg.threads);
    // go(boot tiles?)(kernel, trailing arguments...): a is read at the launch (OneWave::nrm / dr set its act_in first)
    const auto go = [&](bool boot_tiles) {
        return [&, lds = F::lds_bytes(wg.pairs, boot_tiles, nm != nullptr)](auto kernel, const auto &...tail) {
            hipLaunchKernelGGL(kernel, grid, block, lds, h->stream, a, kp.p, kp.pc, tail...);
        };
    };
    PolicyVariant v = V_PLAIN;
    if constexpr (F::kVariants) {
        v = policy_variant(h, bt, nm);
        const VariantArgs va{h, a, variant_tl(h), variant_boot(h, bt), nm};
        // a handle with a parameter range: the ranged *_nrm kernels (rmav_ppo_abi.hip hands every such call statistics and, with a limit, a boot_out)
        // a handle with a frame skip first: the *_fs kernels take the range (mask = 0 without one) and the rule as well
        // ... and one with a tracking reward in front of that: the *_rw kernels take the skip (k = 1 without one) as well
        // ... and one with a disturbance in front of that: the *_ds kernels take the reward as a template parameter
        if (h->disturb_on && (v == V_NRM || v == V_NRM_BOOT)) {
            if (v == V_NRM_BOOT) h->reward_on ? F::template ds<true, true>(go(true), va) : F::template ds<true, false>(go(true), va);
            else h->reward_on ? F::template ds<false, true>(go(false), va) : F::template ds<false, false>(go(false), va);
        } else if (h->disturb_on) return rmav_fail(RMAV_ERR_INVALID, "a handle with a disturbance runs the normalised kernels");
        else if (h->reward_on && v == V_NRM) F::template rw<false>(go(false), va);
        else if (h->reward_on && v == V_NRM_BOOT) F::template rw<true>(go(true), va);
        else if (h->reward_on) return rmav_fail(RMAV_ERR_INVALID, "a handle with a tracking reward runs the normalised kernels");
        else if (h->frame_skip > 1 && v == V_NRM) F::template fs<false>(go(false), va);
        else if (h->frame_skip > 1 && v == V_NRM_BOOT) F::template fs<true>(go(true), va);
        else if (h->frame_skip > 1) return rmav_fail(RMAV_ERR_INVALID, "a handle with a frame skip runs the normalised kernels");
        else if (h->range_mask && v == V_NRM) F::template dr<false>(go(false), va);
        else if (h->range_mask && v == V_NRM_BOOT) F::template dr<true>(go(true), va);
        else if (h->range_mask) return rmav_fail(RMAV_ERR_INVALID, "a ranged handle runs the normalised kernels");
        else if (has_act_rule(h) && v != V_NRM && v != V_NRM_BOOT) return rmav_fail(RMAV_ERR_INVALID, "a handle with a policy action rule runs the normalised kernels");
        else if (v == V_TL) go(false)(F::tl(), va.tl);
        else if (v == V_BOOT) go(true)(F::boot(), va.tl, va.b);
        else if (v == V_NRM) F::template nrm<false>(go(false), va);
        else if (v == V_NRM_BOOT) F::template nrm<true>(go(true), va);
    }
    if (v == V_PLAIN) go(false)(F::plain());
    return check_rollout_launch(h, a);
}

template <int K> int launch_policy_k(rmav_handle h, int kmode, const RolloutArgs &a, const BootArgs *bt, const NormArgs *nm) {
    // (rmav_rollout_policy_boot has checked that the handle has a time limit and that kmode is one of the three actors with a *_boot kernel)
    if ((nm || h->range_mask || has_act_rule(h) || h->frame_skip > 1 || h->reward_on || h->disturb_on) && (K == REINMAV || !policy_has_variants(kmode)))
        return rmav_fail(RMAV_ERR_INVALID, "no %s kernel for policy mode %d",
                         nm ? "normalised" : h->range_mask ? "ranged" : h->disturb_on ? "disturbed" : h->reward_on ? "tracking-reward" : h->frame_skip > 1 ? "frame-skip" : "action-rule", kmode);
    switch (kmode) {
    case RMAV_ACT_POLICY: return launch_family<OneWave<K, ACT_POLICY>>(h, a, nullptr, nullptr);
    case RMAV_ACT_POLICY_BF16:
        return h->tune[RMAV_TUNE_POLICY_PAIR] == 0 ? launch_family<OneWave<K, ACT_POLICY_BF16>>(h, a, nullptr, nullptr)
                                                   : launch_family<Pair<K, FMT_BF16>>(h, a, nullptr, nullptr);
    case ACT_POLICY_F32M: return launch_family<OneWave<K, ACT_POLICY_F32M>>(h, a, bt, nm);
    case ACT_POLICY_F16: return launch_family<Pair<K, FMT_F16>>(h, a, bt, nm);
    case ACT_POLICY_F16_SHARED: return launch_family<SharedPair<K>>(h, a, bt, nm);
    }
    return rmav_fail(RMAV_ERR_INVALID, "unknown policy mode %d", kmode);
}

}  // namespace

int rmav_launch_policy_rollout(rmav_handle h, int kmode, const RolloutArgs &a, const BootArgs *bt, const NormArgs *nm) {
    return dispatch_kind<ALL_KINDS>(h->kind, [&](auto k) { return launch_policy_k<decltype(k)::value>(h, kmode, a, bt, nm); });
}

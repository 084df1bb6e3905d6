// rmav_policy_pair.hpp - the matrix-core actors of the fused PPO rollout as an (actor, critic) wavefront PAIR per 64 envs.
//
// Why.  tools/micro/issue_rate.hip (profiles/r04/issue_rate.md) measured what one instruction costs on a gfx950 SIMD:
//   * a LONE wavefront issues a vector instruction every ~5.0-5.6 cycles, whatever it is (plain, packed, conversion, AGPR move),
//     and a transcendental (v_exp_f32, v_rcp_f32) every 8.8;
//   * the pipe behind it is only half busy then: with TWO wavefronts on the SIMD plain vector instructions retire every 2.5-3.0
//     cycles, packed f32 / conversions every 4.5-5.1, transcendentals every 8.4 (unchanged: they are the pipe's quarter rate);
//   * a v_mfma_f32_32x32x16 takes its 32 cycles on the matrix pipe and hides ~5 independent vector instructions.
// The one-wavefront-per-64-envs actor of round 3 (k_rollout<K, ACT_POLICY_BF16>: ~1 730 instructions per env-step, 512 of them
// transcendental) therefore ran at the lone-wavefront ISSUE rate - 12.5 k cycles per env-step where its pipe time is ~8.5 k -
// at BASELINE's C5 shape (65 536 envs per GPU = one wavefront per SIMD).
//
// What.  Each 64 envs get two wavefronts, so every SIMD hosts two instruction streams at that batch:
//   actor  (wave 0): policy net -> action = mean + std * z -> dynamics / reward / termination / auto-reset / episode bookkeeping;
//                    hands (obs, reward, done, action) over in an LDS tile.  The state never leaves its registers.
//   critic (wave 1): value net of the state the actor hands over, the Gaussian noise z (Philox + Box-Muller: state-independent,
//                    drawn one step AHEAD into an LDS tile) and its log-probability, and EVERY trajectory store.
// One s_barrier per env-step swaps the halves of both double-buffered tiles:
//   actor :            B | read Z(0), pi, step 0 -> O(0) | B0 | read Z(1), pi, step 1 -> O(1) | B1 | ...            | B(T-1)
//   critic: draw Z(0)  B | V(s0), draw Z(1)              | B0 | drain O(0), V(s1), draw Z(2)  | B1 | ... drain O(T-2), V(s(T-1)) | B(T-1) | drain O(T-1), V(sT)
// Same Philox counters, same per-net arithmetic: FMT_BF16 produces the bits of the one-wavefront bf16 actor.
//
// FMT_F16 (RMAV_POLICY_F16_MFMA) is the faster AND more accurate variant: f16 operands (11-bit mantissa against bf16's 8) on
// v_mfma_f32_32x32x16_f16, and the activation handed to the next layer is the logistic term r = 1 / (1 + e^(2z)) itself,
// with tanh(z) = 1 - 2 r folded into the next layer's weights and bias (W' = -2 W, b' = b + rowsum(W): rmav_pack_policy_f16
// scales the weights, the kernel derives b' from the ROUNDED weights when it stages them, so the identity holds exactly for
// the weights the matrix cores see).  That removes the final multiply-add of every tanh (2 v_exp + 2 v_rcp + v_pk_add + cvt
// per value pair: 21.5 pipe cycles per value against 24).  Worst activation error 2^-12 absolute (bf16 tanh: 2^-9 relative).
#pragma once

#include "rmav_kernels.hpp"

// RMAV_PAIR_DR: the pair bodies compile the redraw of a ranged handle's constants (rmav_set_env_param_range; the flag's uses are in the
// fragments both include, rmav_pair_env_load.inc and rmav_pair_episode.inc) only where a *_dr wrapper sets it around its #include.  Not a
// constexpr flag like TL / BOOT / NORM: even a dead local declaration in the bodies changed the register allocation of the bf16 pair kernels.
#define RMAV_PAIR_DR 0
// RMAV_PAIR_DS: likewise the wind / gust disturbance of the *_ds wrappers (rmav_set_disturbance): the per-lane wind and gust, the lane's gravity
// g_vec + d in front of every agent step, the new wind at a reset, the wave-uniform place in the gust sequence.
#define RMAV_PAIR_DS 0
// RMAV_PAIR_SN: likewise the sensor noise of the *_sn wrappers (rmav_set_sensor_noise; rmav_sensor.hpp): the rows of the output tile hold the
// noisy observation - computed once per step by the lane that owns the env -, both nets read it from there, the terminal area likewise.
#define RMAV_PAIR_SN 0
// RMAV_PAIR_AL: likewise the actuator lag of the *_al wrappers (rmav_set_actuator; rmav_actuator.hpp), which are cut from the *_sn bodies: the
// filter state m of the wavefront that integrates, the filter in front of every dynamics sub-step, m = init at a reset, and the noisy rows
// behind one wave-uniform branch per site (al_sn: a handle with lag and no sensor noise stores the state itself).
#define RMAV_PAIR_AL 0
// RMAV_PAIR_SS: likewise the start-state ranges of the *_ss wrappers (rmav_set_start_state; rmav_start.hpp), which are cut from the *_al
// bodies: the spare state of rmav_pair_env_load.inc and the on-demand draw of rmav_pair_episode.inc go through start_apply, and the filter
// with the loads and stores of its state sits behind one wave-uniform flag (ss_al: a handle with a start spec and no actuator lag).
#define RMAV_PAIR_SS 0
// RMAV_PAIR_TC: likewise the termination rules of the *_tc wrappers (rmav_set_termination; rmav_term.hpp), which are cut from the *_ss bodies:
// the termination flag of every dynamics sub-step of rmav_pair_dynamics.inc is term || term_rule<K>(s, tc).
#define RMAV_PAIR_TC 0

namespace rmav {

enum : int { FMT_BF16 = 0, FMT_F16 = 1 };
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;

constexpr int kPairGroupMax = 4;   // (actor, critic) pairs per workgroup: 1 .. 4 (512 threads), a launch parameter

template <int FMT> struct PairOps;
template <> struct PairOps<FMT_BF16> {
    using frag = bf16x8_t;
    static __device__ __forceinline__ f32x16_t mfma(frag a, frag b, f32x16_t c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct PairOps<FMT_F16> {
    using frag = f16x8_t;
    static __device__ __forceinline__ f32x16_t mfma(frag a, frag b, f32x16_t c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};

// LDS words of one pair's hand-over tiles (after the weights, which the pairs of a workgroup share)
template <int NS, int NA> struct PairTile {
    static constexpr int Z_HALF = 4 * 64, Z_WORDS = 2 * Z_HALF;            // noise [4][lane], double-buffered (critic -> actor)
    static constexpr int REW = NS * 64, DONE = REW + 64, ACT = DONE + 64;  // obs [c][lane], reward, done, action [c][lane]
    static constexpr int O_HALF = ACT + NA * 64, O_WORDS = 2 * O_HALF;     // (actor -> critic)
    static constexpr int WORDS = Z_WORDS + O_WORDS;
};
// ... of the kernels that also leave the bootstrap term of truncated steps (k_rollout_pair_boot): behind the words above - their
// offsets do not move - every half of the output tile gets a terminal-state area [c][lane], written by the actor only on a step
// with a truncated lane: the state its reset replaced, for the critic's value net.  A truncated step carries 2.0f in its DONE word.
template <int NS, int NA> struct PairBootTile {
    using PT = PairTile<NS, NA>;
    static constexpr int FIN = PT::WORDS, FIN_HALF = NS * 64;
    static constexpr int WORDS = PT::WORDS + 2 * FIN_HALF;
};
template <int K> constexpr size_t pair_boot_lds_bytes(int g) {
    return sizeof(float) * ((size_t)MfmaLayout::TOTAL + (size_t)g * PairBootTile<Dims<K>::NS, Dims<K>::NA>::WORDS);
}
// (the *_nrm kernels: + kNormWords words of tables between the weights and the tiles)
template <int K> constexpr size_t pair_lds_bytes(int g) {
    return sizeof(float) * ((size_t)MfmaLayout::TOTAL + (size_t)g * PairTile<Dims<K>::NS, Dims<K>::NA>::WORDS);
}

// registers [8 half, 8 half + 8) of an accumulator holding k z (k = 2 log2 e)  ->  r = 1 / (1 + 2^(k z)) = (1 - tanh z) / 2 as an
// f16 B fragment.  2^(kz) = inf -> r = 0, 0 -> r = 1: saturates cleanly.
__device__ __forceinline__ f16x8_t act_frag_f16(const f32x16_t &acc, int half) {
    typedef __attribute__((ext_vector_type(2))) float f32x2_t;
    typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
    u32x4_t packed;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f32x2_t e;
        e[0] = __builtin_amdgcn_exp2f(acc[8 * half + 2 * j]);
        e[1] = __builtin_amdgcn_exp2f(acc[8 * half + 2 * j + 1]);
        e = e + 1.0f;
        f32x2_t r;
        r[0] = __builtin_amdgcn_rcpf(e[0]);
        r[1] = __builtin_amdgcn_rcpf(e[1]);
        packed[j] = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, f16x2_t));   // round to nearest even
    }
    return __builtin_bit_cast(f16x8_t, packed);
}

template <int FMT> __device__ __forceinline__ typename PairOps<FMT>::frag ld_frag_t(const float *base, uint32_t lane) {
    return *reinterpret_cast<const typename PairOps<FMT>::frag *>(base + lane * 4u);   // 16 bytes per lane
}

// FMT_F16, once per launch, by the threads of the block between two barriers (the weights are in LDS): the bias tables
// become those of the folded network (header comment):  b1 <- k b1,  b2 <- k b2 - sum_j A2'[i][j] / 2  (A2' = -2k W2 rounded
// to f16),  b3 <- b3 - sum_j A3'[i][j] / 2  (A3' = -2 W3).
__device__ __forceinline__ void fold_biases_f16() {
    using L = MfmaLayout;
    for (int q = threadIdx.x; q < 2 * (64 + 64 + 32); q += blockDim.x) {
        const int net = q / 160, o = q % 160;
        float *w = lds_w + net * L::NET;
        if (o < 64) {
            w[L::B1 + o] *= kTanhScale;
        } else {
            const bool l2 = o < 128;
            const int i = l2 ? o - 64 : o - 128;            // row of layer 2 (64 rows) / layer 3 (32 rows, padded)
            const int T = l2 ? (i >> 5) : 0, m = i & 31;
            const float *frag0 = w + (l2 ? L::A2 + T * 4 * L::FRAG : L::A3);
            float sum = 0.0f;
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const f16x8_t v = *reinterpret_cast<const f16x8_t *>(frag0 + s * L::FRAG + (m + 32 * h) * 4);
#pragma unroll
                    for (int j = 0; j < 8; ++j) sum += (float)v[j];
                }
            float *b = w + (l2 ? L::B2 : L::B3) + i;
            *b = (l2 ? kTanhScale * *b : *b) - 0.5f * sum;
        }
    }
}

// One net (weights at float offset `net` of lds_w) for the two 32-env column tiles of this wavefront: rows 0..3 of the output
// layer for column tile 0 / 1 (valid in the lanes with h == 0).  Same instruction sequence per net as mlp_mfma (rmav_policy_mfma.hpp).
template <int FMT>
__device__ __forceinline__ void mlp_pair(typename PairOps<FMT>::frag b_in0, typename PairOps<FMT>::frag b_in1, uint32_t net,
                                         float (&t0)[4], float (&t1)[4]) {
    using L = MfmaLayout;
    using O = PairOps<FMT>;
    using frag = typename O::frag;
    asm volatile("" : "+v"(net));   // keep LLVM from hoisting the weight reads out of the env-step loop (136 registers)
    const float *w = lds_w + net;
    const uint32_t lane = threadIdx.x & 63u, h = lane >> 5;
    f32x16_t acc[2][2];   // [row tile T][column tile Nt]
#pragma unroll
    for (int T = 0; T < 2; ++T) {
        const frag a = ld_frag_t<FMT>(w + L::A1 + T * L::FRAG, lane);
        const f32x16_t c = bias_frag(w + L::B1 + 32 * T, h);
        acc[T][0] = O::mfma(a, b_in0, c);
        acc[T][1] = O::mfma(a, b_in1, c);
    }
    frag hb[2][4];        // [Nt][s]
#pragma unroll
    for (int Nt = 0; Nt < 2; ++Nt)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if constexpr (FMT == FMT_F16) hb[Nt][s] = act_frag_f16(acc[s >> 1][Nt], s & 1);
            else hb[Nt][s] = act_frag<true>(acc[s >> 1][Nt], s & 1);
        }
    f32x16_t acc2[2][2];
#pragma unroll
    for (int T = 0; T < 2; ++T) {
        const f32x16_t c = bias_frag(w + L::B2 + 32 * T, h);
        acc2[T][0] = c;
        acc2[T][1] = c;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const frag a = ld_frag_t<FMT>(w + L::A2 + (T * 4 + s) * L::FRAG, lane);
            acc2[T][0] = O::mfma(a, hb[0][s], acc2[T][0]);
            acc2[T][1] = O::mfma(a, hb[1][s], acc2[T][1]);
        }
    }
#pragma unroll
    for (int Nt = 0; Nt < 2; ++Nt)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if constexpr (FMT == FMT_F16) hb[Nt][s] = act_frag_f16(acc2[s >> 1][Nt], s & 1);
            else hb[Nt][s] = act_frag<false>(acc2[s >> 1][Nt], s & 1);
        }
    f32x16_t o0 = bias_frag(w + L::B3, h), o1 = o0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const frag a = ld_frag_t<FMT>(w + L::A3 + s * L::FRAG, lane);
        o0 = O::mfma(a, hb[0][s], o0);
        o1 = O::mfma(a, hb[1][s], o1);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        t0[r] = o0[r];
        t1[r] = o1[r];
    }
}

// Layer-1 B fragments of the wavefront's two column tiles from the env state this lane holds (x: padded to 16).  Lane (n, h)
// of column tile Nt carries components [8h, 8h + 8) of env 32 Nt + n, pre-multiplied by k = 2 log2 e (act_frag): the lane's own
// for its own tile, the partner lane's (l ^ 32) for the other (see policy_forward_mfma).
template <int FMT>
__device__ __forceinline__ void state_frags(const float (&x)[16], typename PairOps<FMT>::frag &b0, typename PairOps<FMT>::frag &b1) {
    using frag = typename PairOps<FMT>::frag;
    const uint32_t h = (threadIdx.x & 63u) >> 5, hmask = 0u - h;
    float mine[8], recv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t lo = __builtin_bit_cast(uint32_t, x[j]), hi = __builtin_bit_cast(uint32_t, x[8 + j]);
        mine[j] = kTanhScale * __builtin_bit_cast(float, (hi & hmask) | (lo & ~hmask));              // x[8h + j]
        const float send = kTanhScale * __builtin_bit_cast(float, (lo & hmask) | (hi & ~hmask));     // x[8(1-h) + j]
        recv[j] = xor32(send);
    }
    frag own, other;
    if constexpr (FMT == FMT_F16) {
        // round-toward-zero pack: one instruction per pair, and a diverged env's huge state saturates at 65504 instead of
        // becoming inf (an inf operand would make the whole tile's outputs NaN)
        typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
        u32x4_t po, pr;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            po[j] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(mine[2 * j], mine[2 * j + 1]));
            pr[j] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(recv[2 * j], recv[2 * j + 1]));
        }
        own = __builtin_bit_cast(frag, po);
        other = __builtin_bit_cast(frag, pr);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            own[j] = (__bf16)mine[j];
            other[j] = (__bf16)recv[j];
        }
    }
    b0 = h ? other : own;   // column tile 0 = envs of lanes 0..31
    b1 = h ? own : other;   // column tile 1 = envs of lanes 32..63
}

// G pairs per workgroup: threads [0, 64 G) are the actors, [64 G, 128 G) their critics; pair g owns envs 64 (G blockIdx + g) ..
// Lanes past the end of the batch are clones of env N-1 (every lane of both wavefronts reaches every barrier and every MFMA).

template <int K, int FMT>
__global__ __launch_bounds__(128 * kPairGroupMax, 2) void k_rollout_pair(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                          const ParamsT<double> pc_shared) {
    constexpr bool TL = false, BOOT = false, NORM = false, FS = false, RW = false;
    [[maybe_unused]] const FrameSkipArgs fs{};
    [[maybe_unused]] const RewardArgs rw{};
    [[maybe_unused]] const TimeLimitArgs tl{};
    [[maybe_unused]] const BootArgs bt{};
    [[maybe_unused]] const NormArgs nm{};
    [[maybe_unused]] const ActRuleArgs ar{};
#include "rmav_pair_body.inc"
}
// ... under an episode time limit (separate symbols: see k_rollout_tl)
template <int K, int FMT>
__global__ __launch_bounds__(128 * kPairGroupMax, 2) void k_rollout_pair_tl(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                             const ParamsT<double> pc_shared, const TimeLimitArgs tl) {
    constexpr bool TL = true, BOOT = false, NORM = false, FS = false, RW = false;
    [[maybe_unused]] const FrameSkipArgs fs{};
    [[maybe_unused]] const RewardArgs rw{};
    [[maybe_unused]] const BootArgs bt{};
    [[maybe_unused]] const NormArgs nm{};
    [[maybe_unused]] const ActRuleArgs ar{};
    static_assert(K != REINMAV, "ReinmavEnv ends an episode every step");
#include "rmav_pair_body.inc"
}
// ... that also leaves the bootstrap term of its truncated steps (rmav_rollout_policy_boot; PairBootTile)
template <int K, int FMT>
__global__ __launch_bounds__(128 * kPairGroupMax, 2) void k_rollout_pair_boot(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                               const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                               const BootArgs bt) {
    constexpr bool TL = true, BOOT = true, NORM = false, FS = false, RW = false;
    [[maybe_unused]] const FrameSkipArgs fs{};
    [[maybe_unused]] const RewardArgs rw{};
    [[maybe_unused]] const NormArgs nm{};
    [[maybe_unused]] const ActRuleArgs ar{};
    static_assert(K != REINMAV && FMT == FMT_F16, "the (actor, critic) pair of time-limited handles");
#include "rmav_pair_body.inc"
}
// The f16 pair on NORMALISED observations (rmav_rollout_policy_norm; see k_rollout_nrm): both wavefronts normalise what they feed
// their net - the actor its registers, the critic the raw state from the hand-over tile, which it also stores.  BOOT = the handle has
// a time limit (k_rollout_pair_boot's body and tiles), otherwise k_rollout_pair's.  kNormWords more LDS words in front of the tiles.
template <int K, bool BOOT>
__global__ __launch_bounds__(128 * kPairGroupMax, 2) void k_rollout_pair_nrm(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                              const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                              const BootArgs bt, const NormArgs nm, const ActRuleArgs ar) {
    constexpr int FMT = FMT_F16;
    constexpr bool TL = BOOT, NORM = true, FS = false, RW = false;
    [[maybe_unused]] const FrameSkipArgs fs{};
    [[maybe_unused]] const RewardArgs rw{};
    static_assert(K != REINMAV, "the four quadrotor kinds");
#include "rmav_pair_body.inc"
}
// The f16 pair of a handle with a parameter range (rmav_set_env_param_range; see k_rollout_nrm_dr): k_rollout_pair_nrm whose actor
// wavefront - the one that integrates - redraws the constants of a lane that resets.  Serves rmav_rollout_policy, _boot and _norm.
template <int K, bool BOOT>
__global__ __launch_bounds__(128 * kPairGroupMax, 2) void k_rollout_pair_dr(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                             const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                             const BootArgs bt, const NormArgs nm, const RangeArgs dr, const ActRuleArgs ar) {
    constexpr int FMT = FMT_F16;
    constexpr bool TL = BOOT, NORM = true, FS = false, RW = false;
    [[maybe_unused]] const FrameSkipArgs fs{};
    [[maybe_unused]] const RewardArgs rw{};
    static_assert(K != REINMAV, "the four quadrotor kinds");
#define RMAV_RUNG 1
#define RMAV_PAIR_BODY "rmav_pair_body.inc"
#include "rmav_pair_rung.inc"
}
// ... and of a handle with a frame skip (rmav_set_frame_skip; FrameSkipArgs in rmav_kernels.hpp): k_rollout_pair_dr - the most general body: a
// handle without a range passes mask = 0, a call without statistics the identity tables - whose actor wavefront holds each action for
// up to fs.k sub-steps between the same two barriers.
template <int K, bool BOOT>
__global__ __launch_bounds__(128 * kPairGroupMax, 2) void k_rollout_pair_fs(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                             const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                             const BootArgs bt, const NormArgs nm, const RangeArgs dr, const PolicySkipArgs ps) {
    const ActRuleArgs ar{ps.noise, ps.lo, ps.hi};
    const FrameSkipArgs fs{ps.k};
    constexpr int FMT = FMT_F16;
    constexpr bool TL = BOOT, NORM = true, FS = true, RW = false;
    [[maybe_unused]] const RewardArgs rw{};
    static_assert(K != REINMAV, "the four quadrotor kinds");
#define RMAV_RUNG 2
#define RMAV_PAIR_BODY "rmav_pair_body.inc"
#include "rmav_pair_rung.inc"
}
// ... and of a handle with a tracking reward (rmav_set_reward; RewardArgs in rmav_kernels.hpp): k_rollout_pair_fs (k = 1 without a skip) whose
// sub-steps are rewarded by reward_rw; the spec is read through the handle's device copy (PolicyRewardArgs).
template <int K, bool BOOT>
__global__ __launch_bounds__(128 * kPairGroupMax, 2) void k_rollout_pair_rw(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                             const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                             const BootArgs bt, const NormArgs nm, const RangeArgs dr, const PolicyRewardArgs ps) {
    const ActRuleArgs ar{ps.noise, ps.lo, ps.hi};
    const FrameSkipArgs fs{ps.k};
    const RewardArgs &rw = *ps.rw;
    constexpr int FMT = FMT_F16;
    constexpr bool TL = BOOT, NORM = true, FS = true, RW = true;
    static_assert(K != REINMAV, "the four quadrotor kinds");
#define RMAV_RUNG 3
#define RMAV_PAIR_BODY "rmav_pair_body.inc"
#include "rmav_pair_rung.inc"
}
// ... and of a handle with a disturbance (rmav_set_disturbance; rmav_disturb.hpp): k_rollout_pair_rw - whose reward becomes the template
// parameter RW, as in k_rollout_ds - whose actor wavefront steps under g_vec + d; both specs are read through the handle's device copies.
template <int K, bool BOOT, bool RW>
__global__ __launch_bounds__(128 * kPairGroupMax, 2) void k_rollout_pair_ds(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                             const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                             const BootArgs bt, const NormArgs nm, const RangeArgs dr, const PolicyDisturbArgs ps) {
    const ActRuleArgs ar{ps.noise, ps.lo, ps.hi};
    const FrameSkipArgs fs{ps.k};
    [[maybe_unused]] const RewardArgs &rw = *ps.rw;
    const DisturbRef ds{ps.ds, ps.b0, ps.phase0};
    constexpr int FMT = FMT_F16;
    constexpr bool TL = BOOT, NORM = true, FS = true;
    static_assert(K != REINMAV, "the four quadrotor kinds");
#define RMAV_RUNG 4
#define RMAV_PAIR_BODY "rmav_pair_body.inc"
#include "rmav_pair_rung.inc"
}
// ... and of a handle with sensor noise (rmav_set_sensor_noise; rmav_sensor.hpp): k_rollout_pair_ds - a handle without a disturbance passes
// the calm spec - whose output rows hold the noisy observation: the actor wavefront computes it once per step, both nets read it.
template <int K, bool BOOT, bool RW>
__global__ __launch_bounds__(128 * kPairGroupMax, 2) void k_rollout_pair_sn(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                             const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                             const BootArgs bt, const NormArgs nm, const RangeArgs dr, const PolicySensorArgs ps) {
    const ActRuleArgs ar{ps.noise, ps.lo, ps.hi};
    const FrameSkipArgs fs{ps.k};
    [[maybe_unused]] const RewardArgs &rw = *ps.rw;
    const DisturbRef ds{ps.ds, ps.b0, ps.phase0};
    const SensorArgs &sn = *ps.sn;
    constexpr int FMT = FMT_F16;
    constexpr bool TL = BOOT, NORM = true, FS = true;
    static_assert(K != REINMAV, "the four quadrotor kinds");
#define RMAV_RUNG 5
#define RMAV_PAIR_BODY "rmav_pair_body.inc"
#include "rmav_pair_rung.inc"
}
// ... and of a handle with actuator lag (rmav_set_actuator; rmav_actuator.hpp): k_rollout_pair_sn whose actor wavefront - the one that
// integrates - carries the filter state m and feeds the dynamics with it; the action it hands to the critic for storing stays the command.
template <int K, bool BOOT, bool RW>
__global__ __launch_bounds__(128 * kPairGroupMax, 2) void k_rollout_pair_al(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                             const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                             const BootArgs bt, const NormArgs nm, const RangeArgs dr, const PolicyActuatorArgs ps) {
    const ActRuleArgs ar{ps.noise, ps.lo, ps.hi};
    const FrameSkipArgs fs{ps.k};
    [[maybe_unused]] const RewardArgs &rw = *ps.rw;
    const DisturbRef ds{ps.ds, ps.b0, ps.phase0};
    const SensorArgs &sn = *ps.sn;
    ActuatorCoef alc;   // alpha and beta once per launch, into registers (every sub-step reads them); init is read where an env is reset
#pragma unroll
    for (int c = 0; c < Dims<K>::NA; ++c) alc.alpha[c] = ps.al->alpha[c], alc.beta[c] = ps.al->beta[c];
    const float *const al_init = ps.al->init;
    float *const al_m = ps.m;
    const uint32_t al_sn = ps.sn_on;
    constexpr int FMT = FMT_F16;
    constexpr bool TL = BOOT, NORM = true, FS = true;
    static_assert(K != REINMAV, "the four quadrotor kinds");
#define RMAV_RUNG 6
#define RMAV_PAIR_BODY "rmav_pair_body.inc"
#include "rmav_pair_rung.inc"
}
// ... and of a handle with a start-state spec (rmav_set_start_state; rmav_start.hpp): k_rollout_pair_al whose actor wavefront maps every fresh
// state it draws; the coefficients are read through the handle's device copy where a state is drawn.
template <int K, bool BOOT, bool RW>
__global__ __launch_bounds__(128 * kPairGroupMax, 2) void k_rollout_pair_ss(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                             const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                             const BootArgs bt, const NormArgs nm, const RangeArgs dr, const PolicyStartArgs pss) {
    const PolicyActuatorArgs &ps = pss.pa;
    const ActRuleArgs ar{ps.noise, ps.lo, ps.hi};
    const FrameSkipArgs fs{ps.k};
    [[maybe_unused]] const RewardArgs &rw = *ps.rw;
    const DisturbRef ds{ps.ds, ps.b0, ps.phase0};
    const SensorArgs &sn = *ps.sn;
    ActuatorCoef alc;   // (as k_rollout_pair_al; unread without actuator lag)
#pragma unroll
    for (int c = 0; c < Dims<K>::NA; ++c) alc.alpha[c] = ps.al->alpha[c], alc.beta[c] = ps.al->beta[c];
    const float *const al_init = ps.al->init;
    float *const al_m = ps.m;
    const uint32_t al_sn = ps.sn_on;
    const StartCoef &ssc = *pss.ss;
    const uint32_t ss_al = pss.al_on;
    constexpr int FMT = FMT_F16;
    constexpr bool TL = BOOT, NORM = true, FS = true;
    static_assert(K != REINMAV, "the four quadrotor kinds");
#define RMAV_RUNG 7
#define RMAV_PAIR_BODY "rmav_pair_body.inc"
#include "rmav_pair_rung.inc"
}
// ... and of a handle with a termination spec (rmav_set_termination; rmav_term.hpp): k_rollout_pair_ss with the rule behind every dynamics
// sub-step; the thresholds are read through the handle's device copy.
template <int K, bool BOOT, bool RW>
__global__ __launch_bounds__(128 * kPairGroupMax, 2) void k_rollout_pair_tc(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                             const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                             const BootArgs bt, const NormArgs nm, const RangeArgs dr, const PolicyTermArgs pts) {
    const PolicyStartArgs &pss = pts.ps;
    const PolicyActuatorArgs &ps = pss.pa;
    const TermArgs &tc = *pts.tc;
    const ActRuleArgs ar{ps.noise, ps.lo, ps.hi};
    const FrameSkipArgs fs{ps.k};
    [[maybe_unused]] const RewardArgs &rw = *ps.rw;
    const DisturbRef ds{ps.ds, ps.b0, ps.phase0};
    const SensorArgs &sn = *ps.sn;
    ActuatorCoef alc;   // (as k_rollout_pair_al; unread without actuator lag)
#pragma unroll
    for (int c = 0; c < Dims<K>::NA; ++c) alc.alpha[c] = ps.al->alpha[c], alc.beta[c] = ps.al->beta[c];
    const float *const al_init = ps.al->init;
    float *const al_m = ps.m;
    const uint32_t al_sn = ps.sn_on;
    const StartCoef &ssc = *pss.ss;
    const uint32_t ss_al = pss.al_on;
    constexpr int FMT = FMT_F16;
    constexpr bool TL = BOOT, NORM = true, FS = true;
    static_assert(K != REINMAV, "the four quadrotor kinds");
#define RMAV_RUNG 8
#define RMAV_PAIR_BODY "rmav_pair_body.inc"
#include "rmav_pair_rung.inc"
}

// ---- one shared 2 x 64 trunk with a mean head and a value head (RMAV_POLICY_F16_SHARED) -------------------------------------------
//
// baselines' build_policy(value_network=None) - what `python -m gym_reinmav.run --alg=ppo2 --network=mlp` builds for the NATIVE envs:
// their env_type is 'native' (entry point gym_reinmav.envs.native:...), for which baselines' ppo2 has no defaults entry, so
// value_network stays None = 'shared': the value function is a linear head on the policy's latent (run.py:63-68; third-party
// behaviour restated from memory).  The MuJoCo defaults (value_network='copy': two separate nets) are what
// k_rollout_pair above evaluates.  One net = half the activations (128 tanh per env and step instead of 256), and the pair splits
// differently: both wavefronts evaluate the net, each for ONE 32-env column tile -
//   A (wave 0): tile 0 = envs 0..31 from its registers;  then action = mean + std z, dynamics, bookkeeping for all 64 envs
//   B (wave 1): tile 1 = envs 32..63 from the hand-over tile; hands the 32 means to A; noise one step ahead, log-prob, all stores
// with two barriers per env-step (X: the means are there; Y: the step's outputs are there).  Output rows 0..3 of the padded
// 32-row output tile are the action mean, row 4 the value: after the last MFMA the mean of env column n sits in lane n
// (h = 0) and its value in lane 32 + n (h = 1), register 0 - for tile 0 that is already the lane that owns the env.
template <int NS, int NA> struct SharedTile {
    using PT = PairTile<NS, NA>;
    static constexpr int MEAN = PT::WORDS;            // means of tile 1's envs [4][32], B -> A
    static constexpr int WORDS = PT::WORDS + 4 * 32;
};
constexpr int kSharedWeights = MfmaLayout::NET + 4;   // one net + logstd[4]
template <int K> constexpr size_t shared_lds_bytes(int g) {
    return sizeof(float) * ((size_t)kSharedWeights + (size_t)g * SharedTile<Dims<K>::NS, Dims<K>::NA>::WORDS);
}

// the net for ONE column tile: o4 = registers 0..3 of the output accumulator (lanes h = 0: rows 0..3 = mean; h = 1: row 4 = value)
__device__ __forceinline__ void mlp_half_f16(f16x8_t b_in, float (&o4)[4]) {
    using L = MfmaLayout;
    using O = PairOps<FMT_F16>;
    uint32_t net = 0u;
    asm volatile("" : "+v"(net));   // keep the weight reads inside the env-step loop
    const float *w = lds_w + net;
    const uint32_t lane = threadIdx.x & 63u, h = lane >> 5;
    f32x16_t acc[2];
#pragma unroll
    for (int T = 0; T < 2; ++T)
        acc[T] = O::mfma(ld_frag_t<FMT_F16>(w + L::A1 + T * L::FRAG, lane), b_in, bias_frag(w + L::B1 + 32 * T, h));
    f16x8_t hb[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) hb[s] = act_frag_f16(acc[s >> 1], s & 1);
#pragma unroll
    for (int T = 0; T < 2; ++T) {
        acc[T] = bias_frag(w + L::B2 + 32 * T, h);
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[T] = O::mfma(ld_frag_t<FMT_F16>(w + L::A2 + (T * 4 + s) * L::FRAG, lane), hb[s], acc[T]);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) hb[s] = act_frag_f16(acc[s >> 1], s & 1);
    f32x16_t o = bias_frag(w + L::B3, h);
#pragma unroll
    for (int s = 0; s < 4; ++s) o = O::mfma(ld_frag_t<FMT_F16>(w + L::A3 + s * L::FRAG, lane), hb[s], o);
#pragma unroll
    for (int r = 0; r < 4; ++r) o4[r] = o[r];
}

__device__ __forceinline__ f16x8_t pack_frag_f16(const float (&v)[8]) {
    typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
    u32x4_t pk;
#pragma unroll
    for (int j = 0; j < 4; ++j) pk[j] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(kTanhScale * v[2 * j], kTanhScale * v[2 * j + 1]));
    return __builtin_bit_cast(f16x8_t, pk);
}


// k_rollout_pair_shared_boot: the terminal-state areas behind SharedTile's words (see PairBootTile), and B's share of a truncated step:
// the net on the terminal states of envs 32..63 from tile half `half` (lane (n, h): components [8h, 8h + 8) of env 32 + n, as
// eval_tile1); the value of env 32 + n arrives in lane 32 + n, the lane that stores for it.  Every lane stores its truncated flag.
template <int NS, int NA> struct SharedBootTile {
    using ST_ = SharedTile<NS, NA>;
    static constexpr int FIN = ST_::WORDS, FIN_HALF = NS * 64;
    static constexpr int WORDS = ST_::WORDS + 2 * FIN_HALF;
};
template <int K> constexpr size_t shared_boot_lds_bytes(int g) {
    return sizeof(float) * ((size_t)kSharedWeights + (size_t)g * SharedBootTile<Dims<K>::NS, Dims<K>::NA>::WORDS);
}
template <int NS, int NA, bool NORM>
__device__ __forceinline__ void shared_boot_tile1(const float *tile, int half, const BootArgs &bt, int64_t step_off, rsrc_t r_none,
                                                  uint32_t off, uint32_t li, [[maybe_unused]] const float *ntab) {
    using PT = PairTile<NS, NA>;
    using SB = SharedBootTile<NS, NA>;
    const uint32_t lane = threadIdx.x & 63u, h = lane >> 5;
    const bool tr = tile[PT::Z_WORDS + half * PT::O_HALF + PT::DONE + lane] == 2.0f;
    float bv = 0.0f;
    if (__ballot(tr) != 0) {   // wave-uniform
        const float *fin = tile + SB::FIN + half * SB::FIN_HALF + 32u + (lane & 31u);
        float x[8], u4[4];
        [[maybe_unused]] const float *nt = nullptr;
        [[maybe_unused]] float nclip = 0.0f;
        if constexpr (NORM) {
            nt = norm_tab(ntab);
            nclip = nt[32];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float lo = (j < NS) ? fin[j * 64] : 0.0f, hi = (8 + j < NS) ? fin[(8 + j) * 64] : 0.0f;
            if constexpr (NORM) {
                if (j < NS) lo = norm1(nt, j, lo, nclip);
                if (8 + j < NS) hi = norm1(nt, 8 + j, hi, nclip);
            }
            x[j] = h ? hi : lo;
        }
        mlp_half_f16(pack_frag_f16(x), u4);
        if (h && tr) bv = u4[0];
    }
    if (h) buf_st(make_rsrc(bt.boot_out + step_off), off, 0, bv);
    const rsrc_t rT = bt.trunc_out ? make_rsrc(bt.trunc_out + step_off) : r_none;
    __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(tr ? 1 : 0), rT, li, 0, 0);
}

template <int K>
__global__ __launch_bounds__(128 * kPairGroupMax, 2) void k_rollout_pair_shared(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                                 const ParamsT<double> pc_shared) {
    constexpr bool TL = false, BOOT = false, NORM = false, FS = false, RW = false;
    [[maybe_unused]] const FrameSkipArgs fs{};
    [[maybe_unused]] const RewardArgs rw{};
    [[maybe_unused]] const TimeLimitArgs tl{};
    [[maybe_unused]] const BootArgs bt{};
    [[maybe_unused]] const NormArgs nm{};
    [[maybe_unused]] const ActRuleArgs ar{};
#include "rmav_pair_shared_body.inc"
}
template <int K>
__global__ __launch_bounds__(128 * kPairGroupMax, 2) void k_rollout_pair_shared_tl(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                                    const ParamsT<double> pc_shared, const TimeLimitArgs tl) {
    constexpr bool TL = true, BOOT = false, NORM = false, FS = false, RW = false;
    [[maybe_unused]] const FrameSkipArgs fs{};
    [[maybe_unused]] const RewardArgs rw{};
    [[maybe_unused]] const BootArgs bt{};
    [[maybe_unused]] const NormArgs nm{};
    [[maybe_unused]] const ActRuleArgs ar{};
    static_assert(K != REINMAV, "ReinmavEnv ends an episode every step");
#include "rmav_pair_shared_body.inc"
}
template <int K>
__global__ __launch_bounds__(128 * kPairGroupMax, 2) void k_rollout_pair_shared_boot(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                                      const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                                      const BootArgs bt) {
    constexpr bool TL = true, BOOT = true, NORM = false, FS = false, RW = false;
    [[maybe_unused]] const FrameSkipArgs fs{};
    [[maybe_unused]] const RewardArgs rw{};
    [[maybe_unused]] const NormArgs nm{};
    [[maybe_unused]] const ActRuleArgs ar{};
    static_assert(K != REINMAV, "ReinmavEnv ends an episode every step");
#include "rmav_pair_shared_body.inc"
}
// ... on NORMALISED observations (rmav_rollout_policy_norm; see k_rollout_pair_nrm)
template <int K, bool BOOT>
__global__ __launch_bounds__(128 * kPairGroupMax, 2) void k_rollout_pair_shared_nrm(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                                     const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                                     const BootArgs bt, const NormArgs nm, const ActRuleArgs ar) {
    constexpr bool TL = BOOT, NORM = true, FS = false, RW = false;
    [[maybe_unused]] const FrameSkipArgs fs{};
    [[maybe_unused]] const RewardArgs rw{};
    static_assert(K != REINMAV, "the four quadrotor kinds");
#include "rmav_pair_shared_body.inc"
}
// ... and the shared-trunk pair of such a handle: k_rollout_pair_shared_nrm with the redraw.
template <int K, bool BOOT>
__global__ __launch_bounds__(128 * kPairGroupMax, 2) void k_rollout_pair_shared_dr(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                                    const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                                    const BootArgs bt, const NormArgs nm, const RangeArgs dr, const ActRuleArgs ar) {
    constexpr bool TL = BOOT, NORM = true, FS = false, RW = false;
    [[maybe_unused]] const FrameSkipArgs fs{};
    [[maybe_unused]] const RewardArgs rw{};
    static_assert(K != REINMAV, "the four quadrotor kinds");
#define RMAV_RUNG 1
#define RMAV_PAIR_BODY "rmav_pair_shared_body.inc"
#include "rmav_pair_rung.inc"
}
// ... and of a handle with a frame skip: k_rollout_pair_shared_dr with the sub-step loop (see k_rollout_pair_fs).
template <int K, bool BOOT>
__global__ __launch_bounds__(128 * kPairGroupMax, 2) void k_rollout_pair_shared_fs(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                                    const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                                    const BootArgs bt, const NormArgs nm, const RangeArgs dr, const PolicySkipArgs ps) {
    const ActRuleArgs ar{ps.noise, ps.lo, ps.hi};
    const FrameSkipArgs fs{ps.k};
    constexpr bool TL = BOOT, NORM = true, FS = true, RW = false;
    [[maybe_unused]] const RewardArgs rw{};
    static_assert(K != REINMAV, "the four quadrotor kinds");
#define RMAV_RUNG 2
#define RMAV_PAIR_BODY "rmav_pair_shared_body.inc"
#include "rmav_pair_rung.inc"
}
// ... and of a handle with a tracking reward: k_rollout_pair_shared_fs with reward_rw (see k_rollout_pair_rw).
template <int K, bool BOOT>
__global__ __launch_bounds__(128 * kPairGroupMax, 2) void k_rollout_pair_shared_rw(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                                    const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                                    const BootArgs bt, const NormArgs nm, const RangeArgs dr, const PolicyRewardArgs ps) {
    const ActRuleArgs ar{ps.noise, ps.lo, ps.hi};
    const FrameSkipArgs fs{ps.k};
    const RewardArgs &rw = *ps.rw;
    constexpr bool TL = BOOT, NORM = true, FS = true, RW = true;
    static_assert(K != REINMAV, "the four quadrotor kinds");
#define RMAV_RUNG 3
#define RMAV_PAIR_BODY "rmav_pair_shared_body.inc"
#include "rmav_pair_rung.inc"
}
// ... and of a handle with a disturbance: k_rollout_pair_shared_rw with the reward as a template parameter and wavefront A stepping under
// g_vec + d (see k_rollout_pair_ds).
template <int K, bool BOOT, bool RW>
__global__ __launch_bounds__(128 * kPairGroupMax, 2) void k_rollout_pair_shared_ds(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                                    const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                                    const BootArgs bt, const NormArgs nm, const RangeArgs dr, const PolicyDisturbArgs ps) {
    const ActRuleArgs ar{ps.noise, ps.lo, ps.hi};
    const FrameSkipArgs fs{ps.k};
    [[maybe_unused]] const RewardArgs &rw = *ps.rw;
    const DisturbRef ds{ps.ds, ps.b0, ps.phase0};
    constexpr bool TL = BOOT, NORM = true, FS = true;
    static_assert(K != REINMAV, "the four quadrotor kinds");
#define RMAV_RUNG 4
#define RMAV_PAIR_BODY "rmav_pair_shared_body.inc"
#include "rmav_pair_rung.inc"
}
// ... and of a handle with sensor noise: k_rollout_pair_shared_ds whose output rows hold the noisy observation (see k_rollout_pair_sn).
template <int K, bool BOOT, bool RW>
__global__ __launch_bounds__(128 * kPairGroupMax, 2) void k_rollout_pair_shared_sn(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                             const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                             const BootArgs bt, const NormArgs nm, const RangeArgs dr, const PolicySensorArgs ps) {
    const ActRuleArgs ar{ps.noise, ps.lo, ps.hi};
    const FrameSkipArgs fs{ps.k};
    [[maybe_unused]] const RewardArgs &rw = *ps.rw;
    const DisturbRef ds{ps.ds, ps.b0, ps.phase0};
    const SensorArgs &sn = *ps.sn;
    constexpr bool TL = BOOT, NORM = true, FS = true;
    static_assert(K != REINMAV, "the four quadrotor kinds");
#define RMAV_RUNG 5
#define RMAV_PAIR_BODY "rmav_pair_shared_body.inc"
#include "rmav_pair_rung.inc"
}

// ... and of a handle with actuator lag: k_rollout_pair_shared_sn whose wavefront A carries the filter state (see k_rollout_pair_al).
template <int K, bool BOOT, bool RW>
__global__ __launch_bounds__(128 * kPairGroupMax, 2) void k_rollout_pair_shared_al(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                             const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                             const BootArgs bt, const NormArgs nm, const RangeArgs dr, const PolicyActuatorArgs ps) {
    const ActRuleArgs ar{ps.noise, ps.lo, ps.hi};
    const FrameSkipArgs fs{ps.k};
    [[maybe_unused]] const RewardArgs &rw = *ps.rw;
    const DisturbRef ds{ps.ds, ps.b0, ps.phase0};
    const SensorArgs &sn = *ps.sn;
    ActuatorCoef alc;   // alpha and beta once per launch, into registers (every sub-step reads them); init is read where an env is reset
#pragma unroll
    for (int c = 0; c < Dims<K>::NA; ++c) alc.alpha[c] = ps.al->alpha[c], alc.beta[c] = ps.al->beta[c];
    const float *const al_init = ps.al->init;
    float *const al_m = ps.m;
    const uint32_t al_sn = ps.sn_on;
    constexpr bool TL = BOOT, NORM = true, FS = true;
    static_assert(K != REINMAV, "the four quadrotor kinds");
#define RMAV_RUNG 6
#define RMAV_PAIR_BODY "rmav_pair_shared_body.inc"
#include "rmav_pair_rung.inc"
}

// ... and of a handle with a start-state spec: k_rollout_pair_shared_al whose wavefront A maps every fresh state it draws (see k_rollout_pair_ss).
template <int K, bool BOOT, bool RW>
__global__ __launch_bounds__(128 * kPairGroupMax, 2) void k_rollout_pair_shared_ss(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                             const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                             const BootArgs bt, const NormArgs nm, const RangeArgs dr, const PolicyStartArgs pss) {
    const PolicyActuatorArgs &ps = pss.pa;
    const ActRuleArgs ar{ps.noise, ps.lo, ps.hi};
    const FrameSkipArgs fs{ps.k};
    [[maybe_unused]] const RewardArgs &rw = *ps.rw;
    const DisturbRef ds{ps.ds, ps.b0, ps.phase0};
    const SensorArgs &sn = *ps.sn;
    ActuatorCoef alc;   // (as k_rollout_pair_shared_al; unread without actuator lag)
#pragma unroll
    for (int c = 0; c < Dims<K>::NA; ++c) alc.alpha[c] = ps.al->alpha[c], alc.beta[c] = ps.al->beta[c];
    const float *const al_init = ps.al->init;
    float *const al_m = ps.m;
    const uint32_t al_sn = ps.sn_on;
    const StartCoef &ssc = *pss.ss;
    const uint32_t ss_al = pss.al_on;
    constexpr bool TL = BOOT, NORM = true, FS = true;
    static_assert(K != REINMAV, "the four quadrotor kinds");
#define RMAV_RUNG 7
#define RMAV_PAIR_BODY "rmav_pair_shared_body.inc"
#include "rmav_pair_rung.inc"
}
// ... and of a handle with a termination spec (rmav_set_termination; rmav_term.hpp): k_rollout_pair_shared_ss with the rule behind every dynamics
// sub-step; the thresholds are read through the handle's device copy.
template <int K, bool BOOT, bool RW>
__global__ __launch_bounds__(128 * kPairGroupMax, 2) void k_rollout_pair_shared_tc(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                             const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                             const BootArgs bt, const NormArgs nm, const RangeArgs dr, const PolicyTermArgs pts) {
    const PolicyStartArgs &pss = pts.ps;
    const PolicyActuatorArgs &ps = pss.pa;
    const TermArgs &tc = *pts.tc;
    const ActRuleArgs ar{ps.noise, ps.lo, ps.hi};
    const FrameSkipArgs fs{ps.k};
    [[maybe_unused]] const RewardArgs &rw = *ps.rw;
    const DisturbRef ds{ps.ds, ps.b0, ps.phase0};
    const SensorArgs &sn = *ps.sn;
    ActuatorCoef alc;   // (as k_rollout_pair_shared_al; unread without actuator lag)
#pragma unroll
    for (int c = 0; c < Dims<K>::NA; ++c) alc.alpha[c] = ps.al->alpha[c], alc.beta[c] = ps.al->beta[c];
    const float *const al_init = ps.al->init;
    float *const al_m = ps.m;
    const uint32_t al_sn = ps.sn_on;
    const StartCoef &ssc = *pss.ss;
    const uint32_t ss_al = pss.al_on;
    constexpr bool TL = BOOT, NORM = true, FS = true;
    static_assert(K != REINMAV, "the four quadrotor kinds");
#define RMAV_RUNG 8
#define RMAV_PAIR_BODY "rmav_pair_shared_body.inc"
#include "rmav_pair_rung.inc"
}

}  // namespace rmav

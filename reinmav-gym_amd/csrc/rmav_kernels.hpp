// rmav_kernels.hpp - HIP kernels of the batched quadrotor path (gfx950 / CDNA4, wave64).
//
// Data layout in HBM (per handle, N envs):
//   state      f32 [nS][N]   struct-of-arrays, updated in place; lane i of a wavefront owns env i,
//                            so every load/store of a component is one fully coalesced 256-byte
//                            wave transaction
//   rec        EnvRec [N]    ONE 16-byte record per env of what a lane needs only when its episode ENDS: steps_beyond_done
//                            (-1 = None), resets drawn so far (the RNG counter), the episode clock at the running episode's
//                            start, the last finished episode's length - one sector in, one out per termination (round 6;
//                            four separate arrays before: three scattered sectors in, four out)
//   ep_ret, last_ret   f32 [N]  running return (in / out every step when tracking), last finished episode's return
//   totals     {u64,f64,u64} [ceil(N/64)]  per-wavefront partial sums of finished episodes
//   env_time   f64 [N]       RMAV_REINMAV only: each env's clock
//   pe[3]      f32 [N]       optional per-env mass / load mass / tether length (domain randomisation)
// Caller buffers: actions [T][nA][N] | [T][N][nA], obs [T][nS][N] | [T][N][nS], rew f32 [T][N],
// done u8 [T][N].  INVARIANT: every kernel stores exactly 0 or 1 into `done` (all done stores below are `cond ? 1 : 0`):
// the Python layer views the bytes as bool without a conversion pass (vec_env.py).
//
// One kernel template covers step (n_steps = 1) and the fused rollout (n_steps = T, state held in
// registers between steps, so per-step HBM traffic shrinks to actions-in + trajectory-out).  The action
// source is a template parameter: caller buffer, counter RNG, the reference's geometric controller, or a
// Gaussian MLP policy evaluated in-kernel (fp32 VALU / bf16 MFMA).
// Per-step physics constants arrive as kernel arguments (scalar registers via s_load), not LDS: they are
// wave-uniform, ~200 bytes, and an LDS copy would cost a barrier per launch for nothing.  LDS is used where
// the constants are too big for SGPRs (the policy weights, 30-42 KB, staged once per launch), for the hand-over
// tiles between the integrator and the memory wavefront of small-batch fused rollouts, and for transposing
// batch-major obs tiles of big launches.
#pragma once

#include "rmav_math.hpp"
#include "rmav_disturb.hpp"
#include "rmav_sensor.hpp"
#include "rmav_actuator.hpp"
#include "rmav_start.hpp"
#include "rmav_term.hpp"
#include "rmav_policy.hpp"
#include "rmav_policy_mfma.hpp"
#include "rmav_policy_mfma32.hpp"

// RMAV_ROLLOUT_SN: the sensor noise of the *_sn wrappers (rmav_set_sensor_noise; rmav_sensor.hpp) is compiled into rmav_rollout_body.inc only
// where a wrapper sets it around its #include, as RMAV_PAIR_DS in the pair bodies: every other kernel's text is what it was.
#define RMAV_ROLLOUT_SN 0
// RMAV_ROLLOUT_AL: likewise the actuator lag of the *_al wrappers (rmav_set_actuator; rmav_actuator.hpp), which are cut from the *_sn bodies:
// the filter state m beside the state, the filter in front of every dynamics sub-step, m = init at a reset, and the noise draw behind ONE
// wave-uniform branch per site (al.sn_on: a handle with lag and no sensor noise does not pay it).
#define RMAV_ROLLOUT_AL 0
// RMAV_ROLLOUT_SS: likewise the start-state ranges of the *_ss wrappers (rmav_set_start_state; rmav_start.hpp), which are cut from the *_al
// bodies: every fresh state - the launch-head spare and the on-demand draw of rmav_rollout_reset.inc - goes through start_apply, and the
// filter, the loads and the stores of its state sit behind ONE wave-uniform flag (ss_al: a handle with a start spec and no actuator lag
// hands the command itself to the dynamics).  In every other kernel that flag is the constant true.
#define RMAV_ROLLOUT_SS 0
// RMAV_ROLLOUT_TC: likewise the termination rules of the *_tc wrappers (rmav_set_termination; rmav_term.hpp), which are cut from the *_ss
// bodies: the termination flag of every dynamics sub-step is term || term_rule<K>(s, tc), directly behind Env<K>::step (tc: TermArgs).
#define RMAV_ROLLOUT_TC 0

namespace rmav {

enum : int { ACT_BUFFER = 0, ACT_RANDOM = 1, ACT_CONTROLLER = 2, ACT_POLICY = 3, ACT_POLICY_BF16 = 4,
              // internal: ACT_RANDOM / ACT_CONTROLLER with a second, "memory" wavefront per 64 envs (see k_rollout)
              ACT_RANDOM_SPLIT = 5, ACT_CONTROLLER_SPLIT = 6,
              // internal: ACT_BUFFER, and the launch ends by evaluating control() on the state it leaves behind
              // (rmav_step_control: the gym-shaped single env gets step()'s outputs and the NEXT control() in one launch)
              ACT_BUFFER_CTRL = 7,
              // the fp32 policy on the fp32-input matrix instructions (rmav_policy_mfma32.hpp)
              ACT_POLICY_F32M = 8,
              // internal: ACT_BUFFER with the memory wavefront prefetching the caller's actions into the hand-over tile
              ACT_BUFFER_SPLIT = 9,
              // the f16 matrix-core actor (RMAV_POLICY_F16_MFMA): only as an (actor, critic) wavefront pair, rmav_policy_pair.hpp
              ACT_POLICY_F16 = 10,
              // ... and the shared-trunk form (one net with a mean head and a value head: RMAV_POLICY_F16_SHARED)
              ACT_POLICY_F16_SHARED = 11 };
constexpr bool is_mfma_policy(int mode) { return mode == ACT_POLICY_BF16 || mode == ACT_POLICY_F32M; }
constexpr bool is_policy(int mode) { return mode == ACT_POLICY || is_mfma_policy(mode); }
constexpr bool is_split(int mode) { return mode == ACT_RANDOM_SPLIT || mode == ACT_CONTROLLER_SPLIT || mode == ACT_BUFFER_SPLIT; }
// split mode whose memory wavefront hands actions TO the integrator (it draws them).  The caller's actions (ACT_BUFFER_SPLIT) were
// fetched by the memory wavefront as well until round 6: on gfx950 loads and stores share ONE counter (vmcnt) and return out of order
// with respect to each other, so a wavefront that both prefetches and stores can only wait for a load with vmcnt(0) - i.e. for every
// outstanding trajectory store (profiles/r06/kernel_sweep.md: 59 % of the wavefronts' cycles in waits).  Now the INTEGRATOR fetches
// them - it has no store in its step loop any more: its rare termination stores moved to the memory wavefront - in bursts of
// buf_prefetch<NA>() steps through a private LDS ring (split_self_fetch).
constexpr bool split_feeds_actions(int mode) { return mode == ACT_RANDOM_SPLIT; }
constexpr bool split_self_fetch(int mode) { return mode == ACT_BUFFER_SPLIT; }
constexpr bool is_buffer(int mode) { return mode == ACT_BUFFER || mode == ACT_BUFFER_CTRL; }
// kernels whose first workgroup publishes "begun" for an armed statistics exchange (see the top of k_rollout)
constexpr bool publishes_start(int mode) { return mode != ACT_CONTROLLER_SPLIT; }
// Split modes: env-steps per hand-over, and the LDS words of the double-buffered tiles
// (actions: helper -> integrator, only when the helper draws them; obs + reward + done [+ actions]: integrator -> helper)
// 1: the tiles of 8 pairs take 70 KB (quad3d) instead of 136 KB of the CU's 160 KB, so a communication kernel's
// workgroups (the overlapped statistics exchange) can share the CU with a rollout workgroup - with 2, a rollout next to a
// 60-80 us co-resident kernel measured +22..29 us at 131 072 envs, with 1 +10..11 us - and alone it is as fast or faster
// (profiles/r02/handover_chunk.md).
#ifndef RMAV_SPLIT_CHUNK
#define RMAV_SPLIT_CHUNK 1
#endif
constexpr int kSplitChunk = RMAV_SPLIT_CHUNK;
// Split modes: (integrator, memory wavefront) pairs per workgroup - a launch parameter (blockDim.x / 128, 1 .. 8).
// The pairs of one workgroup own ADJACENT 64-env groups and run on one CU, so its memory wavefronts store adjacent
// 256-byte segments of every trajectory column (the store-only microbenchmark tools/micro/store_patterns.hip absorbs
// 1 KiB-per-CU segments 6 % faster than 256-byte ones at 65 536 envs on cold buffers, and is at its fastest with
// 128-256 large workgroups).  Measured on cold trajectory buffers, 64-step launches (profiles/r02/split_group_ab.md,
// wg_scan.md): 1 -> 4 pairs at 65 536 envs: quadrotor3d 46.2 -> 45.5 us, slung load 74.3 -> 73.4, 2-D 45.5 -> 43.6,
// 2-D slung load 67.8 -> 65.1; 4 -> 8 pairs at 131 072 envs: quadrotor3d 102 -> 90 us (the one-wavefront kernel: 101),
// but 45 -> 64 us at 65 536 envs, where 8 pairs leave half of the CUs empty and put two integrators on every SIMD.
// The sweet spot is ONE workgroup per CU: the host launches ceil(N / 16 384) pairs per workgroup (256 workgroups).
constexpr int kSplitGroupMax = 8;   // 1024 threads
// ... which caps the kernel at 128 VGPRs.  Round 2's controller-driven slung-load integrators (fp64 controller on top of
// the fp64 step) needed 145-147 and stayed at 4 pairs; with the spare reset state in LDS (SplitTile::SPARE), dirty flags
// instead of copies of the loaded counters and the 8-coefficient atan2 of the 2-D controller they take 109 / 124, so
// every kind runs up to 8 pairs (tests/test_resource_usage.py pins the budgets).
template <int K, bool DRAWS> constexpr int split_group_cap() { return kSplitGroupMax; }
#ifndef RMAV_KBLOCK
#define RMAV_KBLOCK 256
#endif
constexpr int kBlock = RMAV_KBLOCK;  // upper bound (launch bounds); the launch may use 64/128/256 (.. RMAV_KBLOCK)
template <int K, int MODE> constexpr int rollout_threads_max() {   // launch bounds of k_rollout<K, MODE, *>
    return is_split(MODE) ? 128 * split_group_cap<K, split_feeds_actions(MODE)>() : kBlock;
}
template <int NS, int NA, bool DRAWS = true> struct SplitTile {
    static constexpr int CH = kSplitChunk;   // env-steps per hand-over
    static constexpr int A_HALF = DRAWS ? CH * NA * 64 : 0, A_WORDS = 2 * A_HALF;
    // one env-step of outputs: obs (feature-major [c][lane], or env-major [lane][c] with an odd row stride when the
    // trajectory is batch-major - both conflict-free to write), then reward[64], done[64]
    static constexpr int OBS_STRIDE = NS | 1, REW = OBS_STRIDE * 64, DONE = REW + 64;
    static constexpr int ACT = DONE + 64;   // actions [c][lane], only when the integrator computes them
    static constexpr int O_ROW = ACT + (DRAWS ? 0 : NA * 64), O_HALF = CH * O_ROW, O_WORDS = 2 * O_HALF;
    static constexpr int WORDS = A_WORDS + O_WORDS;
    // + (3-D slung load only, see spare_in_lds) the integrator's spare reset state [c][lane], drawn once per
    // launch and consumed by the first termination of a lane, laid out after the tiles of all pairs
    static constexpr int SPARE = NS * 64;
};
// Where the integrator of a two-wavefront kernel keeps its spare reset state.  In registers it is a predicated copy when a
// lane terminates; in LDS it frees NS = 16 registers of the step loop - what the controller-driven 3-D slung-load integrator
// (fp64 controller on top of the fp64 step: 140 VGPRs with it, 124 without) needs to fit the 128-register budget of 8 pairs per
// workgroup - but puts an LDS round trip into the reset path, which nearly every step of a 4-pair workgroup takes (one
// barrier for all pairs; 97 % of its steps have a terminating lane somewhere): 2-D kinds at 65 536 envs +5 %.  So only there.
// (The random- and caller-action 3-D slung-load integrators sit at 127-131 registers with it: LDS as well; measured equal.)
template <int K, int MODE> constexpr bool spare_in_lds() { return K == QUAD3D_SL && is_split(MODE); }
#ifndef RMAV_BUF_PREFETCH
#define RMAV_BUF_PREFETCH 4   // env-steps per burst of the integrator's action fetch (ACT_BUFFER_SPLIT); a power of two
#endif
// ... and twice that for the 2-action kinds, whose steps are half as long
template <int NA> constexpr int buf_prefetch() { return NA <= 2 ? 2 * RMAV_BUF_PREFETCH : RMAV_BUF_PREFETCH; }
// LDS words of the integrator's private action ring [buf_prefetch][NA][lane] (ACT_BUFFER_SPLIT), after the tiles and spares of all pairs
template <int NA> constexpr int buf_ring_words() { return buf_prefetch<NA>() * NA * 64; }
template <int K, int MODE> constexpr int split_words_per_pair() {
    using T = SplitTile<Dims<K>::NS, Dims<K>::NA, split_feeds_actions(MODE)>;
    return T::WORDS + (spare_in_lds<K, MODE>() ? T::SPARE : 0) + (split_self_fetch(MODE) ? buf_ring_words<Dims<K>::NA>() : 0);
}
// F_LEAN (set by the host for the two-wavefront kernels): feature-major trajectories whose every array spans < 4 GiB, so the
// memory wavefront can address them with ONE descriptor per array and a 32-bit scalar step offset (see the lean drain below)
enum : uint32_t { F_AUTO_RESET = 1u, F_TRACK = 2u, F_AOS = 4u, F_LEAN = 8u };


// What a lane needs only when its env's episode ends, as ONE 16-byte record per env (b128 / b96 accesses):
//   sbd        steps_beyond_done, -1 = None (quadrotor3d.py:68,112-122)
//   reset_cnt  resets drawn so far = the Philox counter of the next fresh state
//   ep_start   value of the handle's episode clock when the running episode began: length = clock - ep_start (ep_clock0 below)
//   last_len   length of the most recently finished episode (0: none yet); its return is last_ret[i]
// Round 6 (profiles/r06/step_shape_*.md: a kernel of k_step's memory shape, 1.3 % of the lanes ending an episode): as four
// arrays a termination costs three scattered 32-byte sectors in and four partial sectors out (+ the return); as one record
// one sector in, one 16-byte store out - 1 048 576 envs 24.0 -> 21.6 us, 262 144 envs 5.8 (eager dword loads) -> 5.4.
struct alignas(16) EnvRec {
    int32_t sbd;
    uint32_t reset_cnt;
    uint32_t ep_start;
    int32_t last_len;
};
static_assert(sizeof(EnvRec) == 16, "one b128 access per record");

struct Totals {
    unsigned long long episodes;
    double return_sum;
    unsigned long long length_sum;
};

struct RolloutArgs {
    float *state;
    int64_t n;
    int64_t pitch;          // elements between the feature columns of the trajectory arrays (act_in / act_out / obs_out [T][dim][pitch],
                            // rew_out / done_out [T][pitch]): N, or rmav_rollout_pitched's; batch-major arrays always N
    const float *act_in;
    float *act_out;
    float *obs_out;
    float *rew_out;
    uint8_t *done_out;
    EnvRec *rec;            // per-env termination record {sbd, reset_cnt, ep_start, last_len} (see EnvRec)
    float *ep_ret;
    float *last_ret;
    Totals *totals;
    uint64_t seed;
    uint64_t env_base;
    uint64_t t0;
    int32_t n_steps;
    uint32_t flags;
    float act_lo, act_hi;
    // ACT_POLICY only
    const float *pe[3];     // optional per-env constants (mass, load mass, tether length), nullptr = shared
    double *env_time;       // REINMAV only: the env's own clock t [N] (fp64: it decides 50 vs 51 sub-steps)
    const float *policy_w;  // packed weights (rmav_policy.hpp layout), device memory
    float *logp_out;        // [n_steps][N]
    float *val_out;         // [n_steps + 1][N]
    float *ctrl_out;        // ACT_BUFFER_CTRL only: control() of the state after the last step, [nA][N] | [N][nA]
    // this launch covers envs [slice_first, slice_first + slice_count) of the handle's N (slice_count = 0: all of them);
    // trajectory pitches stay what they are.  slice_first is a multiple of 64.
    uint32_t slice_first, slice_count;
    // statistics exchange armed for this launch (rmav_allgather_stats_arm), nullptr otherwise: every wavefront snapshots
    // its envs' last-episode statistics into the exchange's send buffer [2][xcmax] and then publishes xseq in its word of
    // xarrive - the communicator's stream polls those words (k_wait_arrivals), so the compute stream carries no pack or
    // signal kernel at all
    int32_t *xsend;
    int64_t xcmax;
    uint32_t *xarrive;
    uint32_t xseq;
    // ... and the launch's first workgroup publishes xseq here as soon as it runs: the bound of the communicator stream's wait
    // counts from THIS moment, not from when the waiter started (an armed launch may sit behind seconds of queued work)
    uint32_t *xstarted;
    // k_step of a batch that fits ONE wavefront, outputs in the handle's pinned host block: the wavefront ends by publishing
    // done_seq in this pinned word (system-scope release), and the host spins on it instead of going through
    // hipStreamSynchronize (the kernel's end-of-kernel release + the completion signal + the runtime's wait: ~4 us of a
    // ~15 us host round trip).  nullptr otherwise.
    uint32_t *done_flag;
    uint32_t done_seq;
};

// Episode time limit (rmav_set_time_limit) of the *_tl kernels: a trailing kernel argument of their own, so that RolloutArgs - and
// with it the kernel-argument layout and the instruction stream of every kernel without a limit - stays what it was.
//   max_steps   H > 0: a step after which the running episode length L reaches H (L >= H, for lengths that were already past H
//               when the limit was set) and that did not terminate ends the episode as truncated
//   last_trunc  u8 [N]: per env, 1 if its most recently finished episode was truncated, 0 if it terminated (one byte store per
//               finished episode)
struct TimeLimitArgs {
    uint8_t *last_trunc;
    int32_t max_steps;
};

// Episode lengths are not stored: every env keeps the value the episode clock had when its running episode began (ep_start).
// The clock is the low 32 bits of the handle's step counter t (rmav_seed / rmav_set_step_count, which move t, shift ep_start
// by the same amount) - a value every stepping kernel has in scalar registers anyway, so the scheme costs no register.  A fused kernel turns that into a
// running length once (clock0 - ep_start), counts in registers as before, and writes clock0 + n_steps - length back; the
// single-step kernel touches ep_start only in lanes whose episode ends - no per-step read-modify-write of a length array
// (8 B of 24 B of bookkeeping traffic per env-step; round 5).  32-bit wrap-around is harmless: only differences are used.
// What the auto-reset destroys (rmav_step_final; the k_step_final kernels): a trailing kernel argument of its own, as TimeLimitArgs.
//   final_obs   f32 nS*N in the launch's layout: the state after the dynamics and BEFORE the reset, stored only by the lanes whose
//               episode ended with this step (one masked store group per finished episode); nullptr = not wanted
//   trunc_out   u8 [N], every env: 1 if the time limit ended the episode with this step; nullptr = not wanted
struct FinalArgs {
    float *final_obs;
    uint8_t *trunc_out;
};
// The bootstrap term of a truncated step (rmav_rollout_policy_boot; the *_boot rollout kernels), trailing as well.
//   boot_out    f32 [n_steps][N]: V(s_final) of the launch's value net where the step was truncated, 0 elsewhere
//   trunc_out   u8 [n_steps][N] (nullable): 1 where the time limit ended the episode
struct BootArgs {
    float *boot_out;
    uint8_t *trunc_out;
};

// Observation normalisation (rmav_rollout_policy_norm; the *_nrm rollout kernels), trailing as well.
//   tab   the fp32 tables of a statistics buffer (rmav_obs_norm.hpp: ObsNormStats::mean_f): mean_f[16] | rstd_f[16] | clip | 3 pad words.
// Staged once per launch into LDS behind the weights (kNormWords floats); every evaluation of a net reads its operands from there.
struct NormArgs {
    const float *tab;
};
constexpr int kNormWords = 36;
// (every block of these kernels has at least 64 threads; a strided loop here instead of the one predicated copy cost the quadrotor2d
// k_rollout_nrm a stack frame)
__device__ __forceinline__ void stage_norm(float *dst, const float *tab) {
    if (threadIdx.x < (unsigned)kNormWords) dst[threadIdx.x] = tab[threadIdx.x];
}
// z = clamp((x - mean_f[c]) * rstd_f[c], -clip, clip): subtract, multiply, v_med3_f32, in fp32 (the build is uncontracted) - the
// order include/rmav_ppo.h fixes.  With the identity tables (mean 0, rstd 1, clip +inf) z has the bits of x.
__device__ __forceinline__ float norm1(const float *t, int c, float x, float clip) {
    return __builtin_amdgcn_fmed3f((x - t[c]) * t[16 + c], -clip, clip);
}
// the table pointer for one evaluation: opaque to the optimiser, so that the 33 reads stay inside the env-step loop as LDS
// broadcast reads instead of 33 registers hoisted out of it (the trick of mlp_pair's `net`)
__device__ __forceinline__ const float *norm_tab(const float *ntab) {
    uint32_t o = 0u;
    asm volatile("" : "+v"(o));
    return ntab + o;
}
// the layer-1 input of the actors that take all 16 (padded) components per lane
template <int NS> __device__ __forceinline__ void norm_state16(const float *ntab, const float (&s)[NS], float (&x)[16]) {
    const float *t = norm_tab(ntab);
    const float clip = t[32];
#pragma unroll
    for (int c = 0; c < 16; ++c) x[c] = (c < NS) ? norm1(t, c, s[c], clip) : 0.0f;
}

// Per-episode domain randomisation (rmav_set_env_param_range; the *_dr kernels), trailing as well.
//   pe     the handle's per-env arrays again, writable: a lane whose env resets stores its new constants there (RolloutArgs::pe is const)
//   lo, span   value = fma(span, u, lo), span = hi - lo in fp32, u = word `which` of the env's tag-4 Philox block (include/rmav.h)
//   mask   bit `which`: the parameter has a range; the others keep the value they have
struct RangeArgs {
    float *pe[3];
    float lo[3], span[3];
    uint32_t mask;
};
// the constants of the episode that starts with reset index rc: v[which] for the ranged parameters, v untouched for the others
RMAV_HD void range_draw(const RangeArgs &dr, uint64_t seed, uint64_t env_id, uint32_t rc, float (&v)[3]) {
    uint32_t r[4];
    philox4x32_10((uint32_t)env_id, (uint32_t)(env_id >> 32), rc, 4u << 24, (uint32_t)seed, (uint32_t)(seed >> 32), r);
#pragma unroll
    for (int w = 0; w < 3; ++w)
        if ((dr.mask >> w) & 1u) v[w] = rfma(dr.span[w], u01(r[w]), dr.lo[w]);
}
// ... stored, and re-derived for the lane in each of ps (the env's constants, the fp64 controller's).  A parameter without a range keeps
// its value in force: its per-env element (which no kernel writes) or the shared constant, read again here - on the rare reset path -
// rather than carried through the step loop.
template <typename... Ps>
__device__ __forceinline__ void range_apply(const RangeArgs &dr, const float *const (&pe)[3], const ParamsT<double> &pc_shared, uint32_t li, uint32_t off,
                                            const float (&v)[3], Ps &...ps) {
    const double m = (dr.mask & 1u) ? (double)v[0] : pe[0] ? (double)pe[0][li] : (double)pc_shared.mass;
    const double ml = (dr.mask & 2u) ? (double)v[1] : pe[1] ? (double)pe[1][li] : (double)pc_shared.load_mass;
    const double L = (dr.mask & 4u) ? (double)v[2] : pe[2] ? (double)pe[2][li] : (double)pc_shared.L;
    (override_params(ps, m, ml, L), ...);
#pragma unroll
    for (int w = 0; w < 3; ++w)
        if ((dr.mask >> w) & 1u)
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v[w]), __builtin_amdgcn_make_buffer_rsrc(dr.pe[w], 0, -1, 0x00020000), off, 0, 0);
}

// The action rule of the policy rollouts (rmav_set_policy_action_rule; the *_nrm and *_dr policy kernels), trailing as well: what the
// actors do between the mean head and Env<K>::step.  Three wave-uniform values, by value (scalar registers) - per handle, so not in the
// caller's statistics buffer, which collectors share.
//   noise   1.0f = sample, 0.0f = deterministic: std_eff[c] = std[c] * noise (once per launch), stored action a[c] = fma(std_eff[c], z[c],
//           mean[c]), logp = fma(-0.5, noise * sum z^2, logp0)
//   lo, hi  the action handed to Env<K>::step is min(max(a[c], lo), hi) (one v_med3_f32; lo <= hi); what is stored stays a[c]
// The identity {1, -inf, +inf} - what a handle without a rule passes - leaves the bits of every finite action: std * 1.0f, 1.0f * q and
// the clamp against -inf / +inf are exact.
struct ActRuleArgs {
    float noise, lo, hi;
};
__device__ __forceinline__ float act_clip(const ActRuleArgs &ar, float a) { return __builtin_amdgcn_fmed3f(a, ar.lo, ar.hi); }

// Frame skip (rmav_set_frame_skip; the *_fs kernels), trailing as well: the action of an agent step is evaluated once and held for up to
// k dynamics sub-steps - each an ordinary Env<K>::step with the reward / steps_beyond_done machine behind it - and the first termination
// ends the agent step.  The agent step's reward is R = r_0, then R + r_j in sub-step order (fp32, uncontracted; r_0 keeps its sign bit);
// everything behind the loop - time limit, episode bookkeeping, auto-reset, the stores - sees (state, R, terminated) once, as after one
// step.  The loop is rolled: ONE call site of Env<K>::step under the lane's `live` predicate, left when no lane is live or j reaches k.
//   k   sub-steps per agent step, 2 .. 1024 (a handle with k = 1 launches the kernels without the loop)
struct FrameSkipArgs {
    int32_t k;
};
// ... and what the frame-skip POLICY kernels take in its place: the bound with the handle's action rule (ActRuleArgs' three values), as ONE
// trailing argument - these kernels sit at their scalar-register limit, and the rule and the bound are read together, once per launch
struct PolicySkipArgs {
    float noise, lo, hi;
    int32_t k;
};

// The tracking reward (rmav_set_reward; the *_rw kernels), trailing as well: rmav_reward_spec of include/rmav.h, field for field
// (rmav_handle.hpp asserts the layout).  With it the reward of a dynamics step is no longer -dist / the steps_beyond_done literal but
//     r = terminated ? terminal : fma(-w_act, c, fma(-w_vel, v, fma(-w_pos, d, alive)))
// with d = |P - goal|, v = |V| of the tracked body (RewardBody<K>: the body whose distance the reference rewards) on the stored post-step
// state, and c = |u - act_ref|^2 of the action handed to Env<K>::step.  steps_beyond_done advances as ever; nothing but r depends on it.
struct RewardArgs {
    float goal[3];
    float alive, w_pos, w_vel, w_act;
    float act_ref[4];
    float terminal;
};
// ... and what the tracking-reward POLICY kernels take in PolicySkipArgs' place: its four values and the handle's device copy of the spec
// (rmav_env_s::reward_dev) by pointer - 2 scalar registers instead of 12 in kernels at their scalar-register limit; read at its use
struct PolicyRewardArgs {
    float noise, lo, hi;
    int32_t k;
    const RewardArgs *rw;
};
// ... and the disturbed POLICY kernels (the *_ds policy families): PolicyRewardArgs - rw is read only by the RW = true kernels - with the
// handle's device copy of the disturbance spec and the launch's place in the gust sequence (DisturbRef, rmav_disturb.hpp) behind it
struct PolicyDisturbArgs {
    float noise, lo, hi;
    int32_t k;
    const RewardArgs *rw;
    const DisturbSpec *ds;
    uint64_t b0;
    int32_t phase0;
    int32_t _pad;
};
// ... and the POLICY kernels of a handle with sensor noise (k_rollout_nrm_sn): PolicyDisturbArgs with the handle's device copy of the sensor
// spec behind it.  SensorDev is that copy (rmav_env_s::sensor_dev, rewritten in stream order by k_set_sensor_noise): the sigmas and, for
// a handle without a disturbance, the all-zero disturbance spec ds then points at - at the longest hold, so no launch redraws a gust.
struct SensorDev {
    SensorArgs sn;
    DisturbSpec calm;
};
struct PolicySensorArgs {
    float noise, lo, hi;
    int32_t k;
    const RewardArgs *rw;
    const DisturbSpec *ds;
    uint64_t b0;
    int32_t phase0;
    int32_t _pad;
    const SensorArgs *sn;
};
// ... and the POLICY kernels of a handle with actuator lag (the *_al policy families): PolicySensorArgs with the handle's device copy of the
// filter's coefficients behind it, the handle's array of m and whether the handle has sensor noise.  ActuatorDev is that copy
// (rmav_env_s::actuator_dev, rewritten in stream order by k_set_actuator): alpha, beta, init and - for a handle without a disturbance - the calm
// disturbance spec ds then points at.
struct ActuatorDev {
    ActuatorCoef c;
    DisturbSpec calm;
};
struct PolicyActuatorArgs {
    float noise, lo, hi;
    int32_t k;
    const RewardArgs *rw;
    const DisturbSpec *ds;
    uint64_t b0;
    int32_t phase0;
    uint32_t sn_on;
    const SensorArgs *sn;
    const ActuatorCoef *al;
    float *m;
};
// ... and the POLICY kernels of a handle with a start-state spec (the *_ss policy families): PolicyActuatorArgs with the handle's device copy
// of the map's coefficients behind it and whether the handle has actuator lag.  StartDev is that copy (rmav_env_s::start_dev, rewritten in
// stream order by k_set_start_state): h, m and - for a handle with neither a disturbance nor an actuator spec - the calm disturbance spec ds
// then points at.
struct StartDev {
    StartCoef c;
    DisturbSpec calm;
};
struct PolicyStartArgs {
    PolicyActuatorArgs pa;
    const StartCoef *ss;
    uint32_t al_on;
    uint32_t _pad;
};
// ... and the POLICY kernels of a handle with a termination spec (the *_tc policy families): PolicyStartArgs with the handle's device copy of
// the thresholds behind it.  TermDev is that copy (rmav_env_s::term_dev, rewritten in stream order by k_set_termination): the thresholds,
// the identity start coefficients ss then points at for a handle without a start-state spec (h = 1, m = 0: the plain bits), and the calm
// disturbance spec for a handle with neither a disturbance nor an actuator spec.
struct TermDev {
    TermArgs t;
    StartCoef ident;
    DisturbSpec calm;
};
struct PolicyTermArgs {
    PolicyStartArgs ps;
    const TermArgs *tc;
};
// the observation row of the *_al kernels: the noisy one, or - a handle without sensor noise, wave-uniform - the state itself
template <int NS>
__device__ __forceinline__ void actuator_obs(uint32_t sn_on, const SensorArgs &sn, uint64_t seed, uint64_t env_id, uint64_t b, const float (&s)[NS], float (&o)[NS]) {
    if (sn_on) {
        float z[NS];
        sensor_draw<NS>(seed, env_id, b, z);
        sensor_apply(sn, z, s, o);
    } else {
#pragma unroll
        for (int c = 0; c < NS; ++c) o[c] = s[c];
    }
}
// ... under a z already drawn (the single-step kernel: one z for the terminal and the post-reset observation)
template <int NS>
__device__ __forceinline__ void step_obs_al(uint32_t sn_on, const SensorArgs &sn, const float (&z)[NS], const float (&s)[NS], float (&o)[NS]) {
    if (sn_on) {
        sensor_apply(sn, z, s, o);
    } else {
#pragma unroll
        for (int c = 0; c < NS; ++c) o[c] = s[c];
    }
}
// ... into the words dst[c * 64] of a pair kernel's LDS row (sensor_store_row or the plain copy)
template <int NS>
__device__ __forceinline__ void actuator_obs_row(uint32_t sn_on, const SensorArgs &sn, uint64_t seed, uint64_t env_id, uint64_t b, const float (&s)[NS], float *dst) {
    if (sn_on) {
        sensor_store_row<NS>(sn, seed, env_id, b, s, dst);
    } else {
#pragma unroll
        for (int c = 0; c < NS; ++c) dst[c * 64] = s[c];
    }
}
// where the tracked body's position and velocity sit in the state, and their dimension
template <int K> struct RewardBody;
template <> struct RewardBody<QUAD2D>    { static constexpr int P = 0,  V = 3,  D = 2; };
template <> struct RewardBody<QUAD2D_SL> { static constexpr int P = 0,  V = 3,  D = 2; };   // the quadrotor
template <> struct RewardBody<QUAD3D>    { static constexpr int P = 0,  V = 7,  D = 3; };
template <> struct RewardBody<QUAD3D_SL> { static constexpr int P = 10, V = 13, D = 3; };   // the load
// the sums in the component order of the step norms (rmav_math.hpp): the last component is the plain product
template <int N> __device__ __forceinline__ float reward_sumsq(const float (&e)[N]) {
    float q = e[N - 1] * e[N - 1];
#pragma unroll
    for (int c = N - 2; c >= 0; --c) q = rfma(e[c], e[c], q);
    return q;
}
// c of an agent step: the action is held, so the *_rw bodies compute it once, in front of the sub-step loop
template <int K> __device__ __forceinline__ float reward_act_cost(const float (&u)[Dims<K>::NA], const RewardArgs &rw) {
    float e[Dims<K>::NA];
#pragma unroll
    for (int c = 0; c < Dims<K>::NA; ++c) e[c] = u[c] - rw.act_ref[c];
    return reward_sumsq(e);
}
// THE reward of one dynamics step of a handle with a spec: s = the state Env<K>::step left, c = reward_act_cost of its action
template <int K> __device__ __forceinline__ float reward_rw(const float (&s)[Dims<K>::NS], float c, const RewardArgs &rw, bool term) {
    using B = RewardBody<K>;
    float e[B::D], w[B::D];
#pragma unroll
    for (int i = 0; i < B::D; ++i) {
        e[i] = s[B::P + i] - rw.goal[i];
        w[i] = s[B::V + i];
    }
    const float d = root(reward_sumsq(e)), v = root(reward_sumsq(w));
    const float live = rfma(-rw.w_act, c, rfma(-rw.w_vel, v, rfma(-rw.w_pos, d, rw.alive)));
    return term ? rw.terminal : live;
}

__device__ __forceinline__ uint32_t ep_clock0(const RolloutArgs &a) { return (uint32_t)a.t0; }

template <typename T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// SoA accesses go through buffer instructions: a 128-bit resource descriptor (base address) and the
// per-component offset c*N*4 live in scalar registers (SALU arithmetic, issued beside the VALU stream),
// and the lane supplies only its 32-bit byte offset:   buffer_load_dword v, v_off, s[rsrc], s_coff offen.
// With plain pointers hipcc rebuilt a 64-bit per-lane address with VALU ops for every one of the
// 14 loads / 16-31 stores of a step (35 v_lshl_add_u64 per step, 88 -> 59 VGPRs for quad3d after the
// change).  Limits: lane offset 4*N and column offset 4*nS*N must fit 32 bits, hence N <= 2^25 envs
// per handle (rmav_create enforces it).
using rsrc_t = __amdgpu_buffer_rsrc_t;
__device__ __forceinline__ rsrc_t make_rsrc(const void *p) {
    // raw buffer (stride 0), bounds check disabled (num_records = 2^32-1; lanes are predicated by
    // li < N), word 3 = 0x00020000: the gfx9/CDNA raw-dword format
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, -1, 0x00020000);
}
// same, with the hardware range check armed: stores at byte offsets >= `bytes` are dropped (no per-lane predicate)
__device__ __forceinline__ rsrc_t make_rsrc_bounded(const void *p, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float buf_ld(rsrc_t r, uint32_t voff, uint32_t soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
// read-once data (a caller's action buffer): non-temporal
__device__ __forceinline__ float buf_ld_nt(rsrc_t r, uint32_t voff, uint32_t soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 2));
}
__device__ __forceinline__ int32_t buf_ld_i32(rsrc_t r, uint32_t voff, uint32_t soff) {
    return (int32_t)__builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0);
}
__device__ __forceinline__ void buf_st(rsrc_t r, uint32_t voff, uint32_t soff, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), r, voff, soff, 0);
}
__device__ __forceinline__ void buf_st_i32(rsrc_t r, uint32_t voff, uint32_t soff, int32_t v) {
    __builtin_amdgcn_raw_buffer_store_b32((uint32_t)v, r, voff, soff, 0);
}
// EnvRec accesses: the lane's record sits at byte offset 16 * env (N <= 2^25: fits 32 bits).  b96 = {sbd, reset_cnt, ep_start},
// b64 = {sbd, reset_cnt}; last_len (offset 12) is written on its own by the kernels that keep the rest in registers.
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x3_t __attribute__((ext_vector_type(3)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4_t rec_ld4(rsrc_t r, uint32_t env) { return __builtin_amdgcn_raw_buffer_load_b128(r, env * 16u, 0, 0); }
__device__ __forceinline__ u32x3_t rec_ld3(rsrc_t r, uint32_t env) { return __builtin_amdgcn_raw_buffer_load_b96(r, env * 16u, 0, 0); }
__device__ __forceinline__ u32x2_t rec_ld2(rsrc_t r, uint32_t env) { return __builtin_amdgcn_raw_buffer_load_b64(r, env * 16u, 0, 0); }
__device__ __forceinline__ void rec_st4(rsrc_t r, uint32_t env, u32x4_t v) { __builtin_amdgcn_raw_buffer_store_b128(v, r, env * 16u, 0, 0); }
__device__ __forceinline__ void rec_st3(rsrc_t r, uint32_t env, u32x3_t v) { __builtin_amdgcn_raw_buffer_store_b96(v, r, env * 16u, 0, 0); }
__device__ __forceinline__ void rec_st2(rsrc_t r, uint32_t env, u32x2_t v) { __builtin_amdgcn_raw_buffer_store_b64(v, r, env * 16u, 0, 0); }
// one field (word w of the record) on its own: for kernels at their register limit, where a 2- / 3-register tuple would spill
__device__ __forceinline__ uint32_t rec_ld_word(rsrc_t r, uint32_t env, int w) { return __builtin_amdgcn_raw_buffer_load_b32(r, env * 16u, 4 * w, 0); }
__device__ __forceinline__ void rec_st_word(rsrc_t r, uint32_t env, int w, uint32_t v) { __builtin_amdgcn_raw_buffer_store_b32(v, r, env * 16u, 4 * w, 0); }
__device__ __forceinline__ void rec_st_last_len(rsrc_t r, uint32_t env, int32_t v) { __builtin_amdgcn_raw_buffer_store_b32((uint32_t)v, r, env * 16u, 12, 0); }

// Cache policy of the SoA trajectory stores - a template parameter because the policy bits are instruction
// immediates (a wave-uniform runtime switch around three copies of the stores measured 9 % SLOWER than no
// choice at all: code size and SGPR pressure in the step loop).  Measured, 64-step quadrotor3d rollouts:
//   ST_WRITE_THROUGH (sc0 sc1): the line leaves the L2 at once.  Best when one launch's trajectory is small
//       (65 536 envs: 65.3 -> 62.5 us): nothing is left dirty for the end-of-kernel L2 write-back.
//   ST_STREAM (nt): best when one launch writes more than the 256 MB Infinity Cache absorbs
//       (262 144 envs: 232 -> 206 us, 1 M envs: 892 -> 772 us).
//   ST_DEFAULT in between and for single-step launches.
//   ST_AOS_LDS: big launches that want the obs trajectory as [T][N][nS] (gym / torch batch-major tensors).  A
//       lane storing its own nS floats touches every 128-byte line of the wavefront's 64 x nS x 4 byte span
//       once per component (40 / 64 byte lane stride: 1 M envs 21 % (quadrotor3d) / 32 % (slung load) slower
//       than SoA).  Here each full wavefront transposes its obs tile through LDS (row stride nS | 1 words:
//       conflict-free writes) and emits it as nS fully coalesced 256-byte `nt` stores.
enum : int { ST_DEFAULT = 0, ST_WRITE_THROUGH = 1, ST_STREAM = 2, ST_AOS_LDS = 3 };
template <int ST> struct StoreAux {
    static constexpr int value = (ST == ST_WRITE_THROUGH) ? 17 : ((ST == ST_STREAM || ST == ST_AOS_LDS) ? 2 : 0);
};
// LDS words per wavefront of the ST_AOS_LDS obs tile
template <int NS> struct AosTile { static constexpr int STRIDE = NS | 1, WORDS = 64 * STRIDE; };

template <int AUX>
__device__ __forceinline__ void buf_st_aux(rsrc_t r, uint32_t voff, uint32_t soff, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), r, voff, soff, AUX);
}

// Wide drain of the hand-over tiles, built and measured, NOT the default: the memory wavefront
// reads 4 consecutive envs of a column with one ds_read_b128 and stores them with one buffer_store_dwordx4 - lane
// (cg = lane >> 4, eq = lane & 15) handles envs 4 eq .. 4 eq + 3 of column 4 j + cg - so a 64-env step of quadrotor3d
// leaves in 10 memory instructions instead of 28.  Measured (profiles/r02/wide_drain_ab.md, cold buffers, three
// interleaved repetitions): random-action rollouts 0-8 % slower, controller-driven ones 0-4 % faster; and the memory
// system absorbs 16-byte and 4-byte stores at the same rate (tools/micro/store_patterns.hip).  -DRMAV_WIDE_DRAIN=1
// builds it; both drains pass the parity suite bit for bit.

#ifndef RMAV_WIDE_DRAIN
#define RMAV_WIDE_DRAIN 0
#endif
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
template <int AUX>
__device__ __forceinline__ void buf_st4_aux(rsrc_t r, uint32_t voff, uint32_t soff, float4 v) {
    u32x4_t d;
    d[0] = __builtin_bit_cast(uint32_t, v.x);
    d[1] = __builtin_bit_cast(uint32_t, v.y);
    d[2] = __builtin_bit_cast(uint32_t, v.z);
    d[3] = __builtin_bit_cast(uint32_t, v.w);
    __builtin_amdgcn_raw_buffer_store_b128(d, r, voff, soff, AUX);
}
// C feature-major columns of a tile (column c at words [64 c, 64 c + 64)) -> C SoA columns of `r` (pitch `col` bytes),
// full 64-env wavefront starting at byte offset `wave_off` of each column
template <int AUX, int C>
__device__ __forceinline__ void wide_cols(const float *tile, rsrc_t r, uint32_t wave_off, uint32_t col, uint32_t lane) {
    const uint32_t cg = lane >> 4, eq = lane & 15u;
#pragma unroll
    for (int j = 0; 4 * j < C; ++j) {
        if (4 * j + 3 < C || 4 * j + (int)cg < C) {
            const float4 v = *reinterpret_cast<const float4 *>(tile + (4 * j + cg) * 64u + 4u * eq);
            buf_st4_aux<AUX>(r, wave_off + 16u * eq + cg * col, (uint32_t)(4 * j) * col, v);
        }
    }
}

// FIXED: the launch's options are the usual ones - feature-major trajectories, episode statistics tracked, auto-reset - and known
// at compile time.  The step loop tests each of them with a scalar compare + branch per env-step otherwise (loop-invariant, but the
// compiler does not unswitch a loop of this size), and where a lone wavefront's issue rate IS the step time (one pair per SIMD:
// ~5 cycles per instruction of any kind, profiles/r04/issue_rate.md) those ~10 instructions are 4-9 % of the launch
// (65 536 envs: quadrotor3d 41.8 -> 40.2 us, quadrotor2d-slungload 42.3 -> 38.9, controller-driven quadrotor3d 52.4 -> 47.5).
// Instantiated for the two-wavefront kernels with their default store policy; every other combination takes the runtime flags.
template <int K, int MODE, int ST = ST_DEFAULT, bool FIXED = false>
__global__ __launch_bounds__((rollout_threads_max<K, MODE>())) void k_rollout(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                    const ParamsT<double> pc_shared) {
    constexpr bool TL = false, BOOT = false, NORM = false, DR = false, FS = false, RW = false, DS = false;
    [[maybe_unused]] const DisturbArgs ds{};
    [[maybe_unused]] const FrameSkipArgs fs{};
    [[maybe_unused]] const RewardArgs rw{};
    [[maybe_unused]] const RangeArgs dr{};
    [[maybe_unused]] const ActRuleArgs ar{};
    [[maybe_unused]] const TimeLimitArgs tl{};
    [[maybe_unused]] const BootArgs bt{};
    [[maybe_unused]] const NormArgs nm{};
#include "rmav_rollout_body.inc"
}
// The same kernel under an episode time limit (rmav_set_time_limit): separate symbols, so that the kernels of handles without a limit
// keep their exact instruction stream (and tests/test_resource_usage.py its one hit per k_rollout<K, MODE, ST, FIXED>).  One-wavefront
// modes only (ACT_BUFFER, ACT_RANDOM, ACT_CONTROLLER, ACT_POLICY_F32M); the host routes time-limited launches there.
template <int K, int MODE, int ST = ST_DEFAULT>
__global__ __launch_bounds__((rollout_threads_max<K, MODE>())) void k_rollout_tl(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                       const ParamsT<double> pc_shared, const TimeLimitArgs tl) {
    constexpr bool TL = true, FIXED = false, BOOT = false, NORM = false, DR = false, FS = false, RW = false, DS = false;
    [[maybe_unused]] const DisturbArgs ds{};
    [[maybe_unused]] const FrameSkipArgs fs{};
    [[maybe_unused]] const RewardArgs rw{};
    [[maybe_unused]] const RangeArgs dr{};
    [[maybe_unused]] const ActRuleArgs ar{};
    [[maybe_unused]] const BootArgs bt{};
    [[maybe_unused]] const NormArgs nm{};
    static_assert(!is_split(MODE) && K != REINMAV, "time-limited launches run the one-wavefront kernels");
#include "rmav_rollout_body.inc"
}
// k_rollout_tl of the fp32 matrix-core actor that also leaves the bootstrap term of its truncated steps (rmav_rollout_policy_boot):
// on a step with a truncated lane - about one in max_steps - the wavefront runs the value net once more, on the state the reset is
// about to replace.  A symbol of its own again: k_rollout_tl keeps its instruction stream.
template <int K, int MODE, int ST = ST_DEFAULT>
__global__ __launch_bounds__((rollout_threads_max<K, MODE>())) void k_rollout_boot(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                         const ParamsT<double> pc_shared, const TimeLimitArgs tl, const BootArgs bt) {
    constexpr bool TL = true, FIXED = false, BOOT = true, NORM = false, DR = false, FS = false, RW = false, DS = false;
    [[maybe_unused]] const DisturbArgs ds{};
    [[maybe_unused]] const FrameSkipArgs fs{};
    [[maybe_unused]] const RewardArgs rw{};
    [[maybe_unused]] const RangeArgs dr{};
    [[maybe_unused]] const ActRuleArgs ar{};
    [[maybe_unused]] const NormArgs nm{};
    static_assert(MODE == ACT_POLICY_F32M && K != REINMAV, "the one-wavefront actor of time-limited handles");
#include "rmav_rollout_body.inc"
}
// The fp32 matrix-core actor on NORMALISED observations (rmav_rollout_policy_norm): every evaluation of the policy and the value net -
// the bootstrap value of the last state and of truncated steps included - takes clamp((s - mean) * rstd, -clip, clip) from the tables
// in nm; what is stored as obs stays the raw state.  BOOT = the handle has a time limit (such a launch always leaves the bootstrap
// term: k_rollout_boot's body), otherwise k_rollout's.  Symbols of their own: the kernels above keep their instruction streams.
template <int K, bool BOOT>
__global__ __launch_bounds__((rollout_threads_max<K, ACT_POLICY_F32M>())) void k_rollout_nrm(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                            const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                            const BootArgs bt, const ActRuleArgs ar) {
    // The table pointer rides in RolloutArgs::act_in, which the policy modes do not read: the argument block is k_rollout_boot's.  As a
    // trailing NormArgs (the pair kernels take it that way) the 8 more bytes moved the scalar loads of the argument block, and the
    // quadrotor2d and quadrotor3d kernels came out with a stack frame (64 / 32 bytes per lane, no VGPR spill: these kernels run out of
    // scalar registers) wherever the argument was placed (profiles/r09/obs_norm.md).
    const NormArgs nm{a.act_in};
    constexpr int MODE = ACT_POLICY_F32M, ST = ST_DEFAULT;
    constexpr bool TL = BOOT, FIXED = false, NORM = true, DR = false, FS = false, RW = false, DS = false;
    [[maybe_unused]] const DisturbArgs ds{};
    [[maybe_unused]] const FrameSkipArgs fs{};
    [[maybe_unused]] const RewardArgs rw{};
    [[maybe_unused]] const RangeArgs dr{};
    static_assert(K != REINMAV, "the four quadrotor kinds");
#include "rmav_rollout_body.inc"
}
// The one-wavefront kernels of a handle with a parameter range (rmav_set_env_param_range): a lane whose env resets draws the new
// episode's constants (with the spare reset state where there is one), re-derives what override_params derives, and stores them.
// TL = the handle has a time limit too (tl is not read otherwise).  Symbols of their own: the kernels above keep their instruction streams.
template <int K, int MODE, int ST, bool TL>
__global__ __launch_bounds__((rollout_threads_max<K, MODE>())) void k_rollout_dr(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                       const ParamsT<double> pc_shared, const TimeLimitArgs tl, const RangeArgs dr) {
    constexpr bool FIXED = false, BOOT = false, NORM = false, DR = true, FS = false, RW = false, DS = false;
    [[maybe_unused]] const DisturbArgs ds{};
    [[maybe_unused]] const FrameSkipArgs fs{};
    [[maybe_unused]] const RewardArgs rw{};
    [[maybe_unused]] const ActRuleArgs ar{};
    [[maybe_unused]] const BootArgs bt{};
    [[maybe_unused]] const NormArgs nm{};
    static_assert((MODE == ACT_BUFFER || MODE == ACT_RANDOM || MODE == ACT_CONTROLLER) && K != REINMAV, "ranged launches run the one-wavefront kernels");
#include "rmav_rollout_body.inc"
}

// The fp32 matrix-core actor of a handle with a parameter range: k_rollout_nrm with the redraw, for rmav_rollout_policy, _boot and _norm
// alike - a call without statistics gets the handle's identity tables (z has the bits of x), a call on a time-limited handle that
// wants no bootstrap term gets a scratch boot_out.
template <int K, bool BOOT>
__global__ __launch_bounds__((rollout_threads_max<K, ACT_POLICY_F32M>())) void k_rollout_nrm_dr(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                               const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                               const BootArgs bt, const RangeArgs *drp, const ActRuleArgs ar) {
    // (the range by pointer - the handle's device copy, read with scalar loads on the reset path: as 60 more bytes of kernel arguments
    // it cost three of these kernels, which run out of scalar registers first, a stack frame)
    const RangeArgs &dr = *drp;
    const NormArgs nm{a.act_in};
    constexpr int MODE = ACT_POLICY_F32M, ST = ST_DEFAULT;
    constexpr bool TL = BOOT, FIXED = false, NORM = true, DR = true, FS = false, RW = false, DS = false;
    [[maybe_unused]] const DisturbArgs ds{};
    [[maybe_unused]] const FrameSkipArgs fs{};
    [[maybe_unused]] const RewardArgs rw{};
    static_assert(K != REINMAV, "the four quadrotor kinds");
#include "rmav_rollout_body.inc"
}

// The one-wavefront kernels of a handle with a frame skip (rmav_set_frame_skip): k_rollout_dr - the most general body: a handle without
// a range passes mask = 0 - whose step loop holds each action for up to fs.k sub-steps (FrameSkipArgs).  Symbols of their own: the kernels
// above keep their instruction streams.
template <int K, int MODE, int ST, bool TL>
__global__ __launch_bounds__((rollout_threads_max<K, MODE>())) void k_rollout_fs(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                       const ParamsT<double> pc_shared, const TimeLimitArgs tl, const RangeArgs dr,
                                                       const FrameSkipArgs fs) {
    constexpr bool FIXED = false, BOOT = false, NORM = false, DR = true, FS = true, RW = false, DS = false;
    [[maybe_unused]] const DisturbArgs ds{};
    [[maybe_unused]] const RewardArgs rw{};
    [[maybe_unused]] const ActRuleArgs ar{};
    [[maybe_unused]] const BootArgs bt{};
    [[maybe_unused]] const NormArgs nm{};
    static_assert((MODE == ACT_BUFFER || MODE == ACT_RANDOM || MODE == ACT_CONTROLLER) && K != REINMAV, "frame-skip launches run the one-wavefront kernels");
#include "rmav_rollout_body.inc"
}
// ... and the fp32 matrix-core actor of such a handle: k_rollout_nrm_dr with the sub-step loop, for rmav_rollout_policy, _boot and _norm
// alike (identity tables, a range with mask = 0 and a scratch boot_out where the call or the handle has none).  The actor runs once per
// agent step; the action rule's clip is applied once, in front of the loop.
template <int K, bool BOOT>
__global__ __launch_bounds__((rollout_threads_max<K, ACT_POLICY_F32M>())) void k_rollout_nrm_fs(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                               const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                               const BootArgs bt, const RangeArgs *drp, const PolicySkipArgs ps) {
    const ActRuleArgs ar{ps.noise, ps.lo, ps.hi};
    const FrameSkipArgs fs{ps.k};
    const RangeArgs &dr = *drp;
    const NormArgs nm{a.act_in};
    constexpr int MODE = ACT_POLICY_F32M, ST = ST_DEFAULT;
    constexpr bool TL = BOOT, FIXED = false, NORM = true, DR = true, FS = true, RW = false, DS = false;
    [[maybe_unused]] const DisturbArgs ds{};
    [[maybe_unused]] const RewardArgs rw{};
    static_assert(K != REINMAV, "the four quadrotor kinds");
#include "rmav_rollout_body.inc"
}

// The one-wavefront kernels of a handle with a tracking reward (rmav_set_reward): k_rollout_fs - a handle without a skip passes k = 1, and
// the rolled loop then leaves R = r_0, the bits of the loop-free body - whose sub-steps are rewarded by reward_rw (RewardArgs, by value).
// Symbols of their own: the kernels above keep their instruction streams.
template <int K, int MODE, int ST, bool TL>
__global__ __launch_bounds__((rollout_threads_max<K, MODE>())) void k_rollout_rw(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                       const ParamsT<double> pc_shared, const TimeLimitArgs tl, const RangeArgs dr,
                                                       const FrameSkipArgs fs, const RewardArgs rw) {
    constexpr bool FIXED = false, BOOT = false, NORM = false, DR = true, FS = true, RW = true, DS = false;
    [[maybe_unused]] const DisturbArgs ds{};
    [[maybe_unused]] const ActRuleArgs ar{};
    [[maybe_unused]] const BootArgs bt{};
    [[maybe_unused]] const NormArgs nm{};
    static_assert((MODE == ACT_BUFFER || MODE == ACT_RANDOM || MODE == ACT_CONTROLLER) && K != REINMAV, "tracking-reward launches run the one-wavefront kernels");
#include "rmav_rollout_body.inc"
}
// ... and the fp32 matrix-core actor of such a handle: k_rollout_nrm_fs with reward_rw; the spec is read through the handle's device copy
// (PolicyRewardArgs), the action cost from the clipped action.
template <int K, bool BOOT>
__global__ __launch_bounds__((rollout_threads_max<K, ACT_POLICY_F32M>())) void k_rollout_nrm_rw(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                               const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                               const BootArgs bt, const RangeArgs *drp, const PolicyRewardArgs ps) {
    const ActRuleArgs ar{ps.noise, ps.lo, ps.hi};
    const FrameSkipArgs fs{ps.k};
    const RewardArgs &rw = *ps.rw;
    const RangeArgs &dr = *drp;
    const NormArgs nm{a.act_in};
    constexpr int MODE = ACT_POLICY_F32M, ST = ST_DEFAULT;
    constexpr bool TL = BOOT, FIXED = false, NORM = true, DR = true, FS = true, RW = true, DS = false;
    [[maybe_unused]] const DisturbArgs ds{};
    static_assert(K != REINMAV, "the four quadrotor kinds");
#include "rmav_rollout_body.inc"
}

// The one-wavefront kernels of a handle with a disturbance (rmav_set_disturbance; DisturbArgs in rmav_disturb.hpp): k_rollout_rw's body - k = 1
// without a skip, mask = 0 without a range - whose lane constants carry gv + d.  The wind is drawn at the start of the launch and with
// every spare reset state, the gust whenever the wave-uniform phase counter leaves a block; the fp64 controller's constants keep g_vec.
// RW: the handle has a tracking reward as well (the reference's first-termination literal is no spec: a template parameter; rw is not
// read without it).  One store policy: results never depend on it.
template <int K, int MODE, bool TL, bool RW>
__global__ __launch_bounds__((rollout_threads_max<K, MODE>())) void k_rollout_ds(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                       const ParamsT<double> pc_shared, const TimeLimitArgs tl, const RangeArgs dr,
                                                       const FrameSkipArgs fs, const RewardArgs rw, const DisturbArgs ds) {
    constexpr int ST = ST_DEFAULT;
    constexpr bool FIXED = false, BOOT = false, NORM = false, DR = true, FS = true, DS = true;
    [[maybe_unused]] const ActRuleArgs ar{};
    [[maybe_unused]] const BootArgs bt{};
    [[maybe_unused]] const NormArgs nm{};
    static_assert((MODE == ACT_BUFFER || MODE == ACT_RANDOM || MODE == ACT_CONTROLLER) && K != REINMAV, "disturbed launches run the one-wavefront kernels");
#include "rmav_rollout_body.inc"
}

// ... and the fp32 matrix-core actor of such a handle: k_rollout_nrm_rw - whose reward becomes the template parameter RW - with the lane
// constants of k_rollout_ds; the specs are read through the handle's device copies (PolicyDisturbArgs).
template <int K, bool BOOT, bool RW>
__global__ __launch_bounds__((rollout_threads_max<K, ACT_POLICY_F32M>())) void k_rollout_nrm_ds(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                               const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                               const BootArgs bt, const RangeArgs *drp, const PolicyDisturbArgs ps) {
    const ActRuleArgs ar{ps.noise, ps.lo, ps.hi};
    const FrameSkipArgs fs{ps.k};
    [[maybe_unused]] const RewardArgs &rw = *ps.rw;
    const DisturbRef ds{ps.ds, ps.b0, ps.phase0};
    const RangeArgs &dr = *drp;
    const NormArgs nm{a.act_in};
    constexpr int MODE = ACT_POLICY_F32M, ST = ST_DEFAULT;
    constexpr bool TL = BOOT, FIXED = false, NORM = true, DR = true, FS = true, DS = true;
    static_assert(K != REINMAV, "the four quadrotor kinds");
#include "rmav_rollout_body.inc"
}

// The one-wavefront kernels of a handle with sensor noise (rmav_set_sensor_noise; SensorArgs in rmav_sensor.hpp): k_rollout_ds's body and
// argument list - a handle without a disturbance passes the all-zero spec, whose d = +0 leaves g_vec's bits - with the spec behind it.  Every
// stored observation row is fma(sigma, z, s) of the state after the step and its reset, z of the step counter after the step; nothing
// else reads the noise.  One store policy.
template <int K, int MODE, bool TL, bool RW>
__global__ __launch_bounds__((rollout_threads_max<K, MODE>())) void k_rollout_sn(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                       const ParamsT<double> pc_shared, const TimeLimitArgs tl, const RangeArgs dr,
                                                       const FrameSkipArgs fs, const RewardArgs rw, const DisturbArgs ds, const SensorArgs sn) {
    constexpr int ST = ST_DEFAULT;
    constexpr bool FIXED = false, BOOT = false, NORM = false, DR = true, FS = true, DS = true;
    [[maybe_unused]] const ActRuleArgs ar{};
    [[maybe_unused]] const BootArgs bt{};
    [[maybe_unused]] const NormArgs nm{};
    static_assert((MODE == ACT_BUFFER || MODE == ACT_RANDOM || MODE == ACT_CONTROLLER) && K != REINMAV, "noisy launches run the one-wavefront kernels");
#define RMAV_RUNG 5
#include "rmav_rollout_rung.inc"
}

// ... and the fp32 matrix-core actor of such a handle: k_rollout_nrm_ds whose nets - the actor and the value net of every step, of the
// bootstrap term and of value_out[n_steps] - read the noisy observation, in front of the normaliser, and whose stored obs rows hold it.
// The dynamics, the reward and the state stored in place stay true.  The specs are read through the handle's device copies.
template <int K, bool BOOT, bool RW>
__global__ __launch_bounds__((rollout_threads_max<K, ACT_POLICY_F32M>())) void k_rollout_nrm_sn(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                               const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                               const BootArgs bt, const RangeArgs *drp, const PolicySensorArgs ps) {
    const ActRuleArgs ar{ps.noise, ps.lo, ps.hi};
    const FrameSkipArgs fs{ps.k};
    [[maybe_unused]] const RewardArgs &rw = *ps.rw;
    const DisturbRef ds{ps.ds, ps.b0, ps.phase0};
    const SensorArgs &sn = *ps.sn;
    const RangeArgs &dr = *drp;
    const NormArgs nm{a.act_in};
    constexpr int MODE = ACT_POLICY_F32M, ST = ST_DEFAULT;
    constexpr bool TL = BOOT, FIXED = false, NORM = true, DR = true, FS = true, DS = true;
    static_assert(K != REINMAV, "the four quadrotor kinds");
#define RMAV_RUNG 5
#include "rmav_rollout_rung.inc"
}

// The one-wavefront kernels of a handle with actuator lag (rmav_set_actuator; ActuatorArgs in rmav_actuator.hpp): k_rollout_sn's body and
// argument list with the filter behind it.  m is loaded at the head of the launch, advanced in front of every dynamics sub-step (which reads
// it in the action's place), set to init where the state is reset and stored with the state.  A handle without sensor noise passes
// al.sn_on = 0, which skips the draw with one scalar branch per site; one without a disturbance the all-zero spec.  One store policy.
template <int K, int MODE, bool TL, bool RW>
__global__ __launch_bounds__((rollout_threads_max<K, MODE>())) void k_rollout_al(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                       const ParamsT<double> pc_shared, const TimeLimitArgs tl, const RangeArgs dr,
                                                       const FrameSkipArgs fs, const RewardArgs rw, const DisturbArgs ds, const SensorArgs sn,
                                                       const ActuatorArgs al) {
    constexpr int ST = ST_DEFAULT;
    constexpr bool FIXED = false, BOOT = false, NORM = false, DR = true, FS = true, DS = true;
    [[maybe_unused]] const ActRuleArgs ar{};
    [[maybe_unused]] const BootArgs bt{};
    [[maybe_unused]] const NormArgs nm{};
    const ActuatorCoef &alc = al.c;
    const float *const al_init = al.c.init;
    float *const al_m = al.m;
    const uint32_t al_sn = al.sn_on;
    static_assert((MODE == ACT_BUFFER || MODE == ACT_RANDOM || MODE == ACT_CONTROLLER) && K != REINMAV, "lagged launches run the one-wavefront kernels");
#define RMAV_RUNG 6
#include "rmav_rollout_rung.inc"
}

// ... and the fp32 matrix-core actor of such a handle: k_rollout_nrm_sn whose dynamics read the filtered action.  The filter takes the action
// after the rule's clip; the stored action and its log-probability stay what the policy drew.  The coefficients are read through the
// handle's device copy.
template <int K, bool BOOT, bool RW>
__global__ __launch_bounds__((rollout_threads_max<K, ACT_POLICY_F32M>())) void k_rollout_nrm_al(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                               const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                               const BootArgs bt, const RangeArgs *drp, const PolicyActuatorArgs ps) {
    const ActRuleArgs ar{ps.noise, ps.lo, ps.hi};
    const FrameSkipArgs fs{ps.k};
    [[maybe_unused]] const RewardArgs &rw = *ps.rw;
    const DisturbRef ds{ps.ds, ps.b0, ps.phase0};
    const SensorArgs &sn = *ps.sn;
    const ActuatorCoef &alc = *ps.al;   // (read at their uses, as the other specs of this kernel: held in registers they cost the kind-0 kernels a wave of occupancy)
    const float *const al_init = ps.al->init;
    float *const al_m = ps.m;
    const uint32_t al_sn = ps.sn_on;
    const RangeArgs &dr = *drp;
    const NormArgs nm{a.act_in};
    constexpr int MODE = ACT_POLICY_F32M, ST = ST_DEFAULT;
    constexpr bool TL = BOOT, FIXED = false, NORM = true, DR = true, FS = true, DS = true;
    static_assert(K != REINMAV, "the four quadrotor kinds");
#define RMAV_RUNG 6
#include "rmav_rollout_rung.inc"
}

// The one-wavefront kernels of a handle with a start-state spec (rmav_set_start_state; StartArgs in rmav_start.hpp): k_rollout_al's body and
// argument list with the map behind it.  Every fresh state the launch draws - the spare at its head, the on-demand draw of a second
// termination - is fma(h, v, m) of what reset_state<K> draws; the coefficients are read where a state is drawn.  A handle without actuator
// lag passes ss.al_on = 0 (no filter, no filter state), one without sensor noise al.sn_on = 0, one without a disturbance the all-zero spec.
template <int K, int MODE, bool TL, bool RW>
__global__ __launch_bounds__((rollout_threads_max<K, MODE>())) void k_rollout_ss(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                       const ParamsT<double> pc_shared, const TimeLimitArgs tl, const RangeArgs dr,
                                                       const FrameSkipArgs fs, const RewardArgs rw, const DisturbArgs ds, const SensorArgs sn,
                                                       const ActuatorArgs al, const StartArgs ss) {
    constexpr int ST = ST_DEFAULT;
    constexpr bool FIXED = false, BOOT = false, NORM = false, DR = true, FS = true, DS = true;
    [[maybe_unused]] const ActRuleArgs ar{};
    [[maybe_unused]] const BootArgs bt{};
    [[maybe_unused]] const NormArgs nm{};
    const ActuatorCoef &alc = al.c;
    const float *const al_init = al.c.init;
    float *const al_m = al.m;
    const uint32_t al_sn = al.sn_on;
    const StartCoef &ssc = ss.c;
    const uint32_t ss_al = ss.al_on;
    static_assert((MODE == ACT_BUFFER || MODE == ACT_RANDOM || MODE == ACT_CONTROLLER) && K != REINMAV, "launches with a start spec run the one-wavefront kernels");
#define RMAV_RUNG 7
#include "rmav_rollout_rung.inc"
}

// ... and the fp32 matrix-core actor of such a handle: k_rollout_nrm_al whose fresh states go through the map.  The coefficients are read
// through the handle's device copy, where a state is drawn.
template <int K, bool BOOT, bool RW>
__global__ __launch_bounds__((rollout_threads_max<K, ACT_POLICY_F32M>())) void k_rollout_nrm_ss(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                               const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                               const BootArgs bt, const RangeArgs *drp, const PolicyStartArgs pss) {
    const PolicyActuatorArgs &ps = pss.pa;
    const ActRuleArgs ar{ps.noise, ps.lo, ps.hi};
    const FrameSkipArgs fs{ps.k};
    [[maybe_unused]] const RewardArgs &rw = *ps.rw;
    const DisturbRef ds{ps.ds, ps.b0, ps.phase0};
    const SensorArgs &sn = *ps.sn;
    const ActuatorCoef &alc = *ps.al;
    const float *const al_init = ps.al->init;
    float *const al_m = ps.m;
    const uint32_t al_sn = ps.sn_on;
    const StartCoef &ssc = *pss.ss;
    const uint32_t ss_al = pss.al_on;
    const RangeArgs &dr = *drp;
    const NormArgs nm{a.act_in};
    constexpr int MODE = ACT_POLICY_F32M, ST = ST_DEFAULT;
    constexpr bool TL = BOOT, FIXED = false, NORM = true, DR = true, FS = true, DS = true;
    static_assert(K != REINMAV, "the four quadrotor kinds");
#define RMAV_RUNG 7
#include "rmav_rollout_rung.inc"
}

// The one-wavefront kernels of a handle with a termination spec (rmav_set_termination; TermArgs in rmav_term.hpp): k_rollout_ss's body and
// argument list with the thresholds behind it.  Every dynamics sub-step ends the episode where the reference's rule or term_rule fires;
// everything downstream sees one flag.  A handle without a start-state spec passes the identity coefficients (h = 1, m = 0), one without
// actuator lag ss.al_on = 0, one without sensor noise al.sn_on = 0, one without a disturbance the all-zero spec.
template <int K, int MODE, bool TL, bool RW>
__global__ __launch_bounds__((rollout_threads_max<K, MODE>())) void k_rollout_tc(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                       const ParamsT<double> pc_shared, const TimeLimitArgs tl, const RangeArgs dr,
                                                       const FrameSkipArgs fs, const RewardArgs rw, const DisturbArgs ds, const SensorArgs sn,
                                                       const ActuatorArgs al, const StartArgs ss, const TermArgs tc) {
    constexpr int ST = ST_DEFAULT;
    constexpr bool FIXED = false, BOOT = false, NORM = false, DR = true, FS = true, DS = true;
    [[maybe_unused]] const ActRuleArgs ar{};
    [[maybe_unused]] const BootArgs bt{};
    [[maybe_unused]] const NormArgs nm{};
    const ActuatorCoef &alc = al.c;
    const float *const al_init = al.c.init;
    float *const al_m = al.m;
    const uint32_t al_sn = al.sn_on;
    const StartCoef &ssc = ss.c;
    const uint32_t ss_al = ss.al_on;
    static_assert((MODE == ACT_BUFFER || MODE == ACT_RANDOM || MODE == ACT_CONTROLLER) && K != REINMAV, "launches with a termination spec run the one-wavefront kernels");
#define RMAV_RUNG 8
#include "rmav_rollout_rung.inc"
}

// ... and the fp32 matrix-core actor of such a handle: k_rollout_nrm_ss with the rule behind every dynamics sub-step.  The thresholds are read
// through the handle's device copy.
template <int K, bool BOOT, bool RW>
__global__ __launch_bounds__((rollout_threads_max<K, ACT_POLICY_F32M>())) void k_rollout_nrm_tc(const RolloutArgs a, const typename Env<K>::P p_shared,
                                                                               const ParamsT<double> pc_shared, const TimeLimitArgs tl,
                                                                               const BootArgs bt, const RangeArgs *drp, const PolicyTermArgs pts) {
    const PolicyStartArgs &pss = pts.ps;
    const PolicyActuatorArgs &ps = pss.pa;
    const TermArgs &tc = *pts.tc;
    const ActRuleArgs ar{ps.noise, ps.lo, ps.hi};
    const FrameSkipArgs fs{ps.k};
    [[maybe_unused]] const RewardArgs &rw = *ps.rw;
    const DisturbRef ds{ps.ds, ps.b0, ps.phase0};
    const SensorArgs &sn = *ps.sn;
    const ActuatorCoef &alc = *ps.al;
    const float *const al_init = ps.al->init;
    float *const al_m = ps.m;
    const uint32_t al_sn = ps.sn_on;
    const StartCoef &ssc = *pss.ss;
    const uint32_t ss_al = pss.al_on;
    const RangeArgs &dr = *drp;
    const NormArgs nm{a.act_in};
    constexpr int MODE = ACT_POLICY_F32M, ST = ST_DEFAULT;
    constexpr bool TL = BOOT, FIXED = false, NORM = true, DR = true, FS = true, DS = true;
    static_assert(K != REINMAV, "the four quadrotor kinds");
#define RMAV_RUNG 8
#include "rmav_rollout_rung.inc"
}

// reset_state<K> for the lanes of a wavefront that need it, computed cooperatively (all 64 lanes must be active).
// Philox4x32-10 is ~20 quarter-rate 32x32->64 multiplies per call and reset_state needs ceil(nS / 4) calls (the counter
// word c3 selects the block of four components); executed by a whole wavefront for the one or two lanes whose env has
// just terminated, that is ~1 us of a ~4.5 us single-step launch at one wavefront per SIMD.  Here every group of four
// lanes serves ONE terminating lane instead: lane 4g + b draws block b for the g-th terminating lane (env id and reset
// counter of that lane, so the same counters and the same bits), and the terminating lane picks its components up
// with ds_bpermute.  One Philox call per wavefront covers up to 16 terminations (more: the loop goes round again).
template <int K>
__device__ __forceinline__ void reset_state_wave(uint64_t seed, uint64_t env_id_lane0, uint32_t rc, bool need,
                                                 float (&s)[Dims<K>::NS]) {
    constexpr int NS = Dims<K>::NS;
    static_assert(NS <= 16, "four lanes x four components per terminating lane");
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t m = __ballot(need);                      // wave-uniform
    while (m) {
        // source lane of this lane's group: the (lane >> 2)-th set bit of m, if there is one
        uint64_t t = m;
        for (uint32_t q = lane >> 2; q != 0 && t != 0; --q) t &= t - 1;
        const uint32_t src = t ? (uint32_t)__builtin_ctzll(t) : 0u;
        const uint32_t rc_src = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)rc);
        const uint64_t env = env_id_lane0 + src;
        uint32_t r[4];
        philox4x32_10((uint32_t)env, (uint32_t)(env >> 32), rc_src, (1u << 24) | (lane & 3u), (uint32_t)seed,
                      (uint32_t)(seed >> 32), r);
        float u[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) u[i] = rfma(1.0f / 8388608.0f, (float)(r[i] >> 8), -1.0f);
        // a needing lane with k set bits of m below it (k < 16) takes component c from lane 4k + c / 4, register c % 4
        const uint32_t k = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        const bool mine = need && ((m >> lane) & 1ull) && k < 16u;
#pragma unroll
        for (int c = 0; c < NS; ++c) {
            const float v = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((int)((4u * (k & 15u) + (uint32_t)(c >> 2)) << 2),
                                                                                  __builtin_bit_cast(int, u[c & 3])));
            if (mine) s[c] = v;
        }
        for (int q = 0; q < 16 && m; ++q) m &= m - 1;   // the 16 lowest set bits are served
    }
}

// One env-step per launch (rmav_step, rmav_step_control, the fused = 0 loop of rmav_rollout with caller actions).
// At BASELINE's 65 536 envs such a launch is latency-bound (a few us against 0.8 us of HBM time), so this is
// k_rollout<K, ACT_BUFFER> at n_steps = 1 re-cut for latency, same arithmetic and same bits:
//   * a small straight-line body (no step loop, action prefetch, spare reset state, store-policy or tile variants):
//     less code to fetch into an instruction cache that is cold at every kernel boundary;
//   * outputs that do not depend on the reset state (reward, done, episode accumulators, last-episode stores,
//     steps_beyond_done) are issued BEFORE the Philox draws of reset_state(), whose ~130 instructions then run
//     under the stores' flight time; only the state / obs stores wait for them;
//   * no atomics: the wavefront's slot of the episode totals is read with scalar loads at the top of the kernel
//     (in flight beside the state loads) and rewritten by one lane with plain stores; the per-wave sums are
//     gathered with v_readlane over the set bits of the `done` ballot (usually one bit) instead of shuffle
//     reductions.  (k_rollout adds to the same slots with atomics; launches are stream-ordered, so they mix.)
//
// LAZY (the default from 786 432 envs; rmav_set_tuning(RMAV_TUNE_STEP_LAZY, 0 | 1) overrides): steps_beyond_done and the reset counter are
// needed only by lanes whose env terminates (~1.3 % per step), so they are loaded under that predicate AFTER `done` is known -
// 8 B per env-step less HBM-side traffic (the launch fetches 1.28 x its algorithmic bytes otherwise, of which these two
// arrays are 0.08), but a dependent memory round trip on the critical path of every wavefront that has a finishing lane
// (57 % of them), in a kernel whose whole duration is ~1.5 round trips above the launch floor.  profiles/r03/step_lazy_ab.md.
// What the first loads of k_step need, as LEADING scalar kernel arguments (16 dwords): with -mllvm -amdgpu-kernarg-preload-count=16
// (Makefile) the command processor puts them into scalar registers when it launches a wavefront, so the state / action loads issue
// without first waiting for an s_load of the argument block - one scalar-cache round trip off the critical path of a launch that
// lasts ~1.5 memory round trips (round 6; tools/micro/launch_floor.hip with and without the flag: 2.90 -> 2.72 us for a 14-load /
// 11-store kernel at 65 536 threads).  Aggregates (RolloutArgs, the constants) cannot be preloaded and follow as before; the fields
// duplicated here are read from these arguments only.
struct StepHot {   // (documentation of the argument order; passed as separate scalars)
    float *state; int64_t n; const float *act_in; int64_t pitch; uint32_t block, flags; float *ep_ret; EnvRec *rec;
};
// TL: the launch has an episode time limit (tl; k_step_tl) - with the eager record load only: every lane needs ep_start every step.
// FIN: the launch also reports what the auto-reset destroys (fa; k_step_final).
// DR: the handle has a parameter range (dr; k_step_dr): a finishing lane draws and stores the constants of its new episode.
// RW: the handle has a tracking reward (rw; k_step_rw, on FS's loop - k = 1 without a skip): reward_rw in the literal's place.
// DS: the handle has a disturbance (ds; k_step_ds): the lane's gravity is g_vec + d of this step; the controller's constants keep g_vec.
// SN: the handle has sensor noise (sn; k_step_sn): obs_out and final_obs are fma(sigma, z, s) with ONE z, that of the step counter after
// this step (a.t0 + 1); the state stored in place stays the true one.
// AL: the handle has actuator lag (al; k_step_al): the filter state m is loaded beside the state, advanced in front of every dynamics
// sub-step - which reads m, not the action -, set to init where the env is reset and stored in place; al.sn_on = 0 skips the noise draw.
// SS: the handle has a start-state spec (ss; k_step_ss): a finishing lane maps what it picked up from reset_state_wave (start_apply);
// ss.al_on = 0 skips the filter and the loads and stores of its state (al.m may be NULL).
// TC: the handle has a termination spec (tc; k_step_tc): the flag of every dynamics sub-step is term || term_rule<K>(s, tc).
template <int K, bool CTRL, bool LAZY, int ST, bool TL = false, bool FIN = false, bool DR = false, bool FS = false, bool RW = false, bool DS = false,
          bool SN = false, bool AL = false, bool SS = false, bool TC = false>
__device__ __forceinline__ void step_body(const RolloutArgs &a, const uint32_t block_pl, const typename Env<K>::P &p_shared, const ParamsT<double> &pc_shared,
                                          const TimeLimitArgs &tl = TimeLimitArgs{}, const FinalArgs &fa = FinalArgs{}, const RangeArgs &dr = RangeArgs{},
                                          [[maybe_unused]] const FrameSkipArgs &fs = FrameSkipArgs{}, [[maybe_unused]] const RewardArgs &rw = RewardArgs{},
                                          [[maybe_unused]] const DisturbArgs &ds = DisturbArgs{}, [[maybe_unused]] const SensorArgs &sn = SensorArgs{},
                                          [[maybe_unused]] const ActuatorArgs &al = ActuatorArgs{}, [[maybe_unused]] const StartArgs &ss = StartArgs{},
                                          [[maybe_unused]] const TermArgs &tc = TermArgs{}) {
    static_assert(!TC || SS, "the step of a handle with a termination spec is cut from the start-state body");
    static_assert(!RW || FS, "the tracking reward is evaluated in the sub-step loop");
    static_assert(!SS || AL, "the step of a handle with a start spec is cut from the lagged body");
    // (wave-uniform; the constant true in every kernel but k_step_ss)
    [[maybe_unused]] const bool al_live = !SS || ss.al_on != 0u;
    static_assert(!AL || SN, "the lagged step is cut from the noisy body");
    static_assert(!SN || (DS && FIN), "the noisy step is cut from the disturbed body");
    static_assert(!DS || (FS && DR && !CTRL), "the disturbed step is cut from the most general body: the running reset index, eagerly; k_control behind it");
    static_assert(K != REINMAV, "ReinmavEnv steps go through k_rollout");
    static_assert(!(FS && LAZY), "the frame-skip loop runs the reward machine per sub-step: every lane's record, eagerly");
    static_assert(!(TL && LAZY), "a time limit needs every lane's episode start");
    constexpr int NS = Dims<K>::NS, NA = Dims<K>::NA;
    constexpr int AUX = StoreAux<ST>::value;   // cache policy of the per-env stores (RMAV_TUNE_STEP_STORE; measured in profiles/r04/step_store_policy.md)
    const uint32_t gi = blockIdx.x * block_pl + threadIdx.x;
    const int64_t n = a.n;
    const bool valid = gi < (uint64_t)n;
    // lanes past the end of the batch are clones of env N-1 that store nothing: all 64 lanes of every wavefront
    // stay active, which the cooperative reset needs
    const uint32_t li = valid ? gi : (uint32_t)n - 1u;
    const uint32_t col = (uint32_t)n * 4u, off = li * 4u;
    const uint32_t tcol = (uint32_t)a.pitch * 4u;   // trajectory columns (actions in, obs out): rmav_rollout_pitched
    const bool aos = (a.flags & F_AOS) != 0;
    const bool track = (a.flags & F_TRACK) != 0;
    const bool auto_reset = (a.flags & F_AUTO_RESET) != 0;

    // This wavefront's slot of the episode totals is read at the top of the kernel and rewritten by one lane at the end (no atomics).
    // Through the scalar cache the read shares lgkmcnt with the late kernel-argument loads, so the `s_waitcnt lgkmcnt(0)` in front of
    // the bookkeeping loads also waits for that memory round trip; as a VECTOR load issued behind all other loads it does not.
    // Same-box A/B (profiles/r05/step_totals_ab.md): the vector form is 2.5 - 6 % faster for the 3-D kinds up to 262 144 envs (65 536:
    // 4.32 - 4.47 -> 4.18 - 4.24 us) and 1 - 3.5 % slower for the 2-D kinds and the lazy kernel of the big batches - so it is chosen by kind.
    constexpr bool kVectorTotals = !LAZY && (K == QUAD3D || K == QUAD3D_SL);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(gi >> 6);
    Totals tot = {0ull, 0.0, 0ull};
    if constexpr (!kVectorTotals) {
        if (track) tot = a.totals[wave];
    }

    const rsrc_t r_state = make_rsrc(a.state);
    float s[NS], act[NA];
#pragma unroll
    for (int c = 0; c < NS; ++c) s[c] = buf_ld(r_state, off, (uint32_t)c * col);
    if (aos) {
        // batch-major actions [N][nA] (what a policy network / the VecEnv hands over): ONE 8- / 16-byte load per lane when the
        // buffer is aligned for it (torch tensors are), instead of nA dword loads that each touch all of the wavefront's lines
        const float *src = a.act_in + (int64_t)li * NA;
        if ((reinterpret_cast<uintptr_t>(a.act_in) & (NA * 4 - 1)) == 0) {   // wave-uniform (NA is 2 or 4)
            if constexpr (NA == 4) {
                const float4 v = *reinterpret_cast<const float4 *>(src);
                act[0] = v.x; act[1] = v.y; act[2] = v.z; act[3] = v.w;
            } else {
                const float2 v = *reinterpret_cast<const float2 *>(src);
                act[0] = v.x; act[1] = v.y;
            }
        } else {
#pragma unroll
            for (int c = 0; c < NA; ++c) act[c] = src[c];
        }
    } else {
        const rsrc_t r = make_rsrc(a.act_in);
#pragma unroll
        for (int c = 0; c < NA; ++c) act[c] = LAZY ? buf_ld_nt(r, off, (uint32_t)c * tcol) : buf_ld(r, off, (uint32_t)c * tcol);   // big batches: read-once, non-temporal (1 048 576 envs -2 %)
    }
    [[maybe_unused]] float am[AL ? NA : 1];   // AL: the filter state of this env
    if constexpr (AL) {
        if constexpr (SS) {
#pragma unroll
            for (int c = 0; c < NA; ++c) am[c] = 0.0f;
        }
        if (al_live) {
            const rsrc_t r_m = make_rsrc(al.m);
#pragma unroll
            for (int c = 0; c < NA; ++c) am[c] = buf_ld(r_m, off, (uint32_t)c * col);
        }
    }
    float er = 0.0f;
    if (track) er = buf_ld(make_rsrc(a.ep_ret), off, 0);
    // needed only by lanes whose env terminates in this step: steps_beyond_done (the terminal reward), the reset counter
    // (the Philox counter of the fresh state) and the episode's start (its length)
    // - ONE 16-byte record per env (EnvRec): one b128 load, and one b128 store when the episode ends
    int32_t sb = -1;
    uint32_t rc = 0, es = 0;
    int32_t ll = 0;   // the record's last_len: rewritten with the record (kept when the handle does not track episodes)
    if constexpr (!LAZY) {
        const u32x4_t q = rec_ld4(make_rsrc(a.rec), li);
        sb = (int32_t)q.x;
        rc = q.y;
        es = q.z;
        ll = (int32_t)q.w;
    }
    if constexpr (kVectorTotals) if (track) {
        const Totals *tp = a.totals + (gi >> 6);
        asm volatile("" : "+v"(tp));          // keep it a vector address (vmcnt, in order), not an s_load
        tot = *tp;
    }
    typename Env<K>::P pl = p_shared;
    ParamsT<double> pcl = pc_shared;
    if (a.pe[0] || a.pe[1] || a.pe[2]) {
        const double m = a.pe[0] ? (double)a.pe[0][li] : (double)pc_shared.mass;
        const double ml = a.pe[1] ? (double)a.pe[1][li] : (double)pc_shared.load_mass;
        const double L = a.pe[2] ? (double)a.pe[2][li] : (double)pc_shared.L;
        override_params(pl, m, ml, L);
        override_params(pcl, m, ml, L);
    }
    // DS: the wind of the running episode (reset index rc - 1: rc names the NEXT fresh state), the gust of this step's block (ds.b0: the
    // host has divided), added to the lane's gravity; one d for all sub-steps.  Lanes past the end are clones of env N-1 here too.
    if constexpr (DS) {
        float w[disturb_dim<K>()], q[disturb_dim<K>()];
        wind_draw(ds.spec(), a.seed, a.env_base + (uint64_t)li, rc - 1u, w);
        gust_draw(ds.spec(), a.seed, a.env_base + (uint64_t)li, ds.b0, q);
        disturb_apply(pl, p_shared, w, q);
    }

    float dist = 0.0f;
    bool done;
    // FS (k_step_fs): the action is held for up to fs.k sub-steps; the reward machine runs behind each, r accumulates in sub-step order
    [[maybe_unused]] float r_fs = 0.0f;
    if constexpr (FS) {
        [[maybe_unused]] float c_rw = 0.0f;   // RW: the action cost of the agent step - the action is held, so once
        if constexpr (RW) c_rw = reward_act_cost<K>(act, rw);
        bool live = true;
        done = false;
        int32_t j = 0;
        do {
            if (live) {
                bool term;
                if constexpr (AL) {   // the filter advances in front of every dynamics sub-step, which reads m; c_rw keeps the command
                    actuator_step<NA>(al.c, am, act);
                    if constexpr (SS) {   // (without actuator lag: the command itself - a select, as in rmav_rollout_body.inc)
#pragma unroll
                        for (int c = 0; c < NA; ++c) am[c] = al_live ? am[c] : act[c];
                    }
                    Env<K>::step(s, am, pl, dist, term);
                } else {
                    Env<K>::step(s, act, pl, dist, term);
                }
                if constexpr (TC) term = term || term_rule<K>(s, tc);   // the termination rules (rmav_term.hpp)
                float rj = -dist;
                if constexpr (RW) {   // the tracking reward (RewardArgs) in the literal's place; steps_beyond_done advances as ever
                    rj = reward_rw<K>(s, c_rw, rw, term);
                    if (term) sb = (sb < 0) ? 0 : sb + 1;
                } else if (term) {
                    rj = (sb < 0) ? 1.0f : 0.0f;
                    sb = (sb < 0) ? 0 : sb + 1;
                }
                r_fs = (j == 0) ? rj : r_fs + rj;
                done = term;
                live = !term;
            }
            ++j;
        } while (j < fs.k && __ballot(live) != 0);
    } else {
        Env<K>::step(s, act, pl, dist, done);
    }
    // SN: the noise of every observation this step emits (wave-uniform: skipped when the caller asked for none)
    [[maybe_unused]] float sn_z[SN ? NS : 1];
    if constexpr (AL) {   // (a handle with lag and no sensor noise skips the draw and stores the state itself: al.sn_on is wave-uniform)
        if ((a.obs_out || fa.final_obs) && al.sn_on) sensor_draw<NS>(a.seed, a.env_base + (uint64_t)li, a.t0 + 1u, sn_z);
    } else if constexpr (SN) {
        if (a.obs_out || fa.final_obs) sensor_draw<NS>(a.seed, a.env_base + (uint64_t)li, a.t0 + 1u, sn_z);
    }
    // Where and how the step's outputs are stored (same values on both paths): reward, done, running return
    auto store_scalars = [&](float r_, bool done_, float er_) {
        if (a.rew_out) buf_st_aux<AUX>(make_rsrc(a.rew_out), off, 0, r_);
        if (a.done_out) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(done_ ? 1 : 0), make_rsrc(a.done_out), li, 0, AUX);
        if (track) buf_st_aux<AUX>(make_rsrc(a.ep_ret), off, 0, er_);
    };
    // ... the state in place, and the obs copy when the caller wants one
    // (Batch-major obs through an LDS transpose - as the fused kernels do for big launches - was built and measured here in
    // round 3: QuadrotorVecEnv.step at 65 536 envs 4.91-5.02 us with it, 4.99-5.01 without; not kept.)
    auto store_state = [&]() {
#pragma unroll
        for (int c = 0; c < NS; ++c) buf_st_aux<AUX>(r_state, off, (uint32_t)c * col, s[c]);
        if (a.obs_out) {
            if constexpr (SN) {   // the observation of the state just stored: the z the terminal observation took
                float o[NS];
                if constexpr (AL) step_obs_al(al.sn_on, sn, sn_z, s, o);
                    else sensor_apply(sn, sn_z, s, o);
                if (aos) {
                    float *dst = a.obs_out + (int64_t)li * NS;
#pragma unroll
                    for (int c = 0; c < NS; ++c) dst[c] = o[c];
                } else {
                    const rsrc_t ro = make_rsrc(a.obs_out);
#pragma unroll
                    for (int c = 0; c < NS; ++c) buf_st_aux<AUX>(ro, off, (uint32_t)c * tcol, o[c]);
                }
            } else if (aos) {
                float *dst = a.obs_out + (int64_t)li * NS;
#pragma unroll
                for (int c = 0; c < NS; ++c) dst[c] = s[c];
            } else {
                const rsrc_t ro = make_rsrc(a.obs_out);
#pragma unroll
                for (int c = 0; c < NS; ++c) buf_st_aux<AUX>(ro, off, (uint32_t)c * tcol, s[c]);
            }
        }
    };
    // (Round 6, measured and NOT kept - profiles/r06/step_early_stores_ab.md: storing the outputs of the lanes whose env goes on
    // right here, under the execution mask, ahead of the finishing lanes' record round trip and reset draw, and the finishing
    // lanes' afterwards.  Every store of the 57 % of wavefronts with a finishing lane then leaves as two partial-line pieces:
    // 1 048 576 envs 23.0 -> 25.9 us, 4 194 304 envs 85.1 -> 99.9.)
    if constexpr (LAZY) {
        if (done) {   // only the finishing lanes fetch: ONE 32-byte sector each
            const u32x4_t q = rec_ld4(make_rsrc(a.rec), li);
            sb = (int32_t)q.x;
            rc = q.y;
            es = q.z;
            ll = (int32_t)q.w;
        }
    }
    // reward / steps_beyond_done machine  (quadrotor3d.py:112-122 and siblings)
    float r = -dist;
    if constexpr (FS) {
        r = r_fs;   // (the machine ran inside the loop)
    } else if (done) {
        r = (sb < 0) ? 1.0f : 0.0f;
        sb = (sb < 0) ? 0 : sb + 1;
    }
    // time limit: the episode that has run L = clock + 1 - ep_start steps after this one ends here as truncated when L reaches the
    // limit and the dynamics did not terminate (r and sb stay the step's own)
    [[maybe_unused]] bool trunc = false;
    if constexpr (TL) {
        trunc = !done && (int32_t)(ep_clock0(a) + 1u - es) >= tl.max_steps;
        done = done || trunc;
    }
    bool fin = false;
    float fin_ret = 0.0f;
    int32_t fin_len = 0;
    // everything that does not need the reset state goes out first
    if (valid) {
        if (track) {
            er += r;
            if (done) {
                const uint32_t clk = ep_clock0(a) + 1u;       // the episode clock after this step
                const int32_t el = (int32_t)(clk - es);       // steps of the episode that ends here
                buf_st(make_rsrc(a.last_ret), off, 0, er);
                ll = el;
                es = clk;                                     // the next episode starts now
                fin = true;
                fin_ret = er;
                fin_len = el;
                er = 0.0f;
            }
        }
        if constexpr (TL) {
            if (done) es = ep_clock0(a) + 1u;                 // (also when the handle does not track episodes)
        }
        store_scalars(r, done, er);
        if (done) {   // the whole record in one 16-byte store
            rec_st4(make_rsrc(a.rec), li, u32x4_t{(uint32_t)sb, auto_reset ? rc + 1u : rc, es, (uint32_t)ll});
            if constexpr (TL) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(trunc ? 1 : 0), make_rsrc(tl.last_trunc), li, 0, 0);
        }
        // the terminal state of the finishing lanes, under the execution mask, before reset_state_wave() replaces it; the truncated
        // flag of every lane
        if constexpr (FIN) {
            if (fa.final_obs && done) {
                if constexpr (SN) {   // the terminal observation: the pre-reset state under the step's z
                    float o[NS];
                    if constexpr (AL) step_obs_al(al.sn_on, sn, sn_z, s, o);
                    else sensor_apply(sn, sn_z, s, o);
                    if (aos) {
                        float *dst = fa.final_obs + (int64_t)li * NS;
#pragma unroll
                        for (int c = 0; c < NS; ++c) dst[c] = o[c];
                    } else {
                        const rsrc_t rf = make_rsrc(fa.final_obs);
#pragma unroll
                        for (int c = 0; c < NS; ++c) buf_st_aux<AUX>(rf, off, (uint32_t)c * tcol, o[c]);
                    }
                } else if (aos) {
                    float *dst = fa.final_obs + (int64_t)li * NS;
#pragma unroll
                    for (int c = 0; c < NS; ++c) dst[c] = s[c];
                } else {
                    const rsrc_t rf = make_rsrc(fa.final_obs);
#pragma unroll
                    for (int c = 0; c < NS; ++c) buf_st_aux<AUX>(rf, off, (uint32_t)c * tcol, s[c]);
                }
            }
            if (fa.trunc_out) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(trunc ? 1 : 0), make_rsrc(fa.trunc_out), li, 0, AUX);
        }
    }
    if (auto_reset)   // wave-uniform; every lane takes part
        reset_state_wave<K>(a.seed, a.env_base + (uint64_t)(gi - (threadIdx.x & 63u)), rc, done && valid, s);
    if constexpr (SS) {   // the start-state spec: the finishing lane maps the v it picked up
        if (auto_reset && done && valid) start_apply<NS>(ss.c, s);
    }
    if constexpr (DR) {
        // the new episode's constants: the tag-4 block of the reset index its state was drawn with.  The step above used the old
        // ones; the control() below, on the fresh state, uses these.
        if (auto_reset && done && valid) {
            float v[3] = {0.0f, 0.0f, 0.0f};
            range_draw(dr, a.seed, a.env_base + (uint64_t)gi, rc, v);
            range_apply(dr, a.pe, pc_shared, li, off, v, pl, pcl);
        }
    }
    if (valid) store_state();
    if constexpr (AL) {   // the filter state in place: init where the env was reset (the step that ended the episode ran with the old m)
        if (valid && al_live) {
            const rsrc_t r_m = make_rsrc(al.m);
#pragma unroll
            for (int c = 0; c < NA; ++c) buf_st_aux<AUX>(r_m, off, (uint32_t)c * col, (auto_reset && done) ? al.c.init[c] : am[c]);
        }
    }
    if constexpr (CTRL) {   // control() of the state this launch leaves behind
        float a2[NA];
        env_control<K>(s, pcl, a2);
        if (valid) {
            if (aos) {
                float *dst = a.ctrl_out + (int64_t)li * NA;
#pragma unroll
                for (int c = 0; c < NA; ++c) dst[c] = a2[c];
            } else {
                const rsrc_t rc2 = make_rsrc(a.ctrl_out);
#pragma unroll
                for (int c = 0; c < NA; ++c) buf_st(rc2, off, (uint32_t)c * col, a2[c]);
            }
        }
    }
    if (track) {
        uint64_t m = __ballot(fin);
        if (m != 0) {   // wave-uniform
            uint32_t cnt = 0, len = 0;
            float ret = 0.0f;
            while (m) {
                const int l = __builtin_ctzll(m);
                m &= m - 1;
                cnt += 1u;
                len += (uint32_t)__builtin_amdgcn_readlane(fin_len, l);
                ret += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, fin_ret), l));
            }
            if ((threadIdx.x & 63u) == 0u) {
                Totals *slot = a.totals + wave;
                slot->episodes = tot.episodes + cnt;
                slot->return_sum = tot.return_sum + (double)ret;
                slot->length_sum = tot.length_sum + len;
            }
        }
    }
    if (a.done_flag) {   // wave-uniform; the launch is a single wavefront (the host guarantees it)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every lane's output stores have been acknowledged
        if (gi == 0) __hip_atomic_store(a.done_flag, a.done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// The two entry points of step_body.  k_step: the eager variant (below 786 432 envs, where a launch is latency-bound) with the
// preloaded leading arguments (StepHot).  k_step_big: the lazy variant of the big batches WITHOUT them - there the command processor's
// extra work per wavefront launch (16 384 wavefronts at 1 048 576 envs) costs more than the saved scalar load: same-box A/B
// 21.7 -> 22.6 us with preloading, against 4.25 -> 3.93 us at 65 536 envs and 6.32 -> 5.95 at 262 144 (profiles/r06/step_preload_ab.md).
template <int K, bool CTRL, bool LAZY = false, int ST = ST_DEFAULT>
__global__ __launch_bounds__(kBlock) void k_step(float *state_pl, int64_t n_pl, const float *act_pl, int64_t pitch_pl, uint32_t block_pl, uint32_t flags_pl,
                                                 float *ep_ret_pl, EnvRec *rec_pl, const RolloutArgs a_in, const typename Env<K>::P p_shared,
                                                 const ParamsT<double> pc_shared) {
    // the preloaded copies replace the struct's fields (same values: launch_step_k fills both); every other field is still
    // loaded from the argument block when it is first used
    RolloutArgs a = a_in;
    a.state = state_pl;
    a.n = n_pl;
    a.act_in = act_pl;
    a.pitch = pitch_pl;
    a.flags = flags_pl;
    a.ep_ret = ep_ret_pl;
    a.rec = rec_pl;
    step_body<K, CTRL, LAZY, ST>(a, block_pl, p_shared, pc_shared);
}
template <int K, bool LAZY, int ST>
__global__ __launch_bounds__(kBlock) void k_step_big(const RolloutArgs a, const typename Env<K>::P p_shared, const ParamsT<double> pc_shared) {
    step_body<K, false, LAZY, ST>(a, blockDim.x, p_shared, pc_shared);
}
// k_step under an episode time limit, for every batch size (eager record load; k_step's preloaded leading arguments, the limit as a
// trailing argument: k_step and k_step_big keep their instruction streams)
template <int K, bool CTRL, int ST = ST_DEFAULT>
__global__ __launch_bounds__(kBlock) void k_step_tl(float *state_pl, int64_t n_pl, const float *act_pl, int64_t pitch_pl, uint32_t block_pl, uint32_t flags_pl,
                                                    float *ep_ret_pl, EnvRec *rec_pl, const RolloutArgs a_in, const typename Env<K>::P p_shared,
                                                    const ParamsT<double> pc_shared, const TimeLimitArgs tl) {
    RolloutArgs a = a_in;
    a.state = state_pl;
    a.n = n_pl;
    a.act_in = act_pl;
    a.pitch = pitch_pl;
    a.flags = flags_pl;
    a.ep_ret = ep_ret_pl;
    a.rec = rec_pl;
    step_body<K, CTRL, false, ST, true>(a, block_pl, p_shared, pc_shared, tl);
}

// rmav_step_final: k_step / k_step_tl (TL) that also store the finishing lanes' terminal state and every lane's truncated flag (FinalArgs).
// Eager record load for every batch size, as k_step_tl; without a limit `tl` is not read.
template <int K, bool TL, int ST = ST_DEFAULT>
__global__ __launch_bounds__(kBlock) void k_step_final(float *state_pl, int64_t n_pl, const float *act_pl, int64_t pitch_pl, uint32_t block_pl, uint32_t flags_pl,
                                                       float *ep_ret_pl, EnvRec *rec_pl, const RolloutArgs a_in, const typename Env<K>::P p_shared,
                                                       const ParamsT<double> pc_shared, const TimeLimitArgs tl, const FinalArgs fa) {
    RolloutArgs a = a_in;
    a.state = state_pl;
    a.n = n_pl;
    a.act_in = act_pl;
    a.pitch = pitch_pl;
    a.flags = flags_pl;
    a.ep_ret = ep_ret_pl;
    a.rec = rec_pl;
    step_body<K, false, false, ST, TL, true>(a, block_pl, p_shared, pc_shared, tl, fa);
}

// The single-step kernel of a handle with a parameter range, for every batch size and all four single-step entry points: k_step_final's
// argument list (fa's pointers are NULL when the call wants neither output, tl is read only with TL) and the range behind it.
template <int K, bool CTRL, bool TL>
__global__ __launch_bounds__(kBlock) void k_step_dr(float *state_pl, int64_t n_pl, const float *act_pl, int64_t pitch_pl, uint32_t block_pl, uint32_t flags_pl,
                                                    float *ep_ret_pl, EnvRec *rec_pl, const RolloutArgs a_in, const typename Env<K>::P p_shared,
                                                    const ParamsT<double> pc_shared, const TimeLimitArgs tl, const FinalArgs fa, const RangeArgs dr) {
    RolloutArgs a = a_in;
    a.state = state_pl;
    a.n = n_pl;
    a.act_in = act_pl;
    a.pitch = pitch_pl;
    a.flags = flags_pl;
    a.ep_ret = ep_ret_pl;
    a.rec = rec_pl;
    step_body<K, CTRL, false, ST_DEFAULT, TL, true, true>(a, block_pl, p_shared, pc_shared, tl, fa, dr);
}

// The single-step kernel of a handle with a frame skip (rmav_set_frame_skip), for every batch size: k_step_dr's body and argument list -
// a handle without a range passes mask = 0, one without a limit TL = false, a call that wants neither of fa's outputs NULL pointers -
// with the sub-step loop, whose bound trails.  No CTRL form: control() is evaluated per agent step by rmav_control (rmav_step_control
// refuses such a handle).
template <int K, bool TL>
__global__ __launch_bounds__(kBlock) void k_step_fs(float *state_pl, int64_t n_pl, const float *act_pl, int64_t pitch_pl, uint32_t block_pl, uint32_t flags_pl,
                                                    float *ep_ret_pl, EnvRec *rec_pl, const RolloutArgs a_in, const typename Env<K>::P p_shared,
                                                    const ParamsT<double> pc_shared, const TimeLimitArgs tl, const FinalArgs fa, const RangeArgs dr,
                                                    const FrameSkipArgs fs) {
    RolloutArgs a = a_in;
    a.state = state_pl;
    a.n = n_pl;
    a.act_in = act_pl;
    a.pitch = pitch_pl;
    a.flags = flags_pl;
    a.ep_ret = ep_ret_pl;
    a.rec = rec_pl;
    step_body<K, false, false, ST_DEFAULT, TL, true, true, true>(a, block_pl, p_shared, pc_shared, tl, fa, dr, fs);
}

// The single-step kernel of a handle with a tracking reward (rmav_set_reward): k_step_fs (k = 1 without a skip) with reward_rw, the spec
// trailing by value.  No CTRL form either: rmav_step_control launches k_control behind it.
// (quadrotor3d: the twelve values of the spec take k_step_fs's 94 scalar registers past the 96 that eight wavefronts per SIMD leave each;
// asked for eight, the compiler parks a few of them in lanes of a vector register - it has twenty to spare - and reads them back with
// v_readlane: no scratch)
template <int K> constexpr unsigned step_rw_min_waves() { return K == QUAD3D ? 8u : 1u; }
template <int K, bool TL>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(step_rw_min_waves<K>()))) void k_step_rw(float *state_pl, int64_t n_pl, const float *act_pl, int64_t pitch_pl, uint32_t block_pl, uint32_t flags_pl,
                                                    float *ep_ret_pl, EnvRec *rec_pl, const RolloutArgs a_in, const typename Env<K>::P p_shared,
                                                    const ParamsT<double> pc_shared, const TimeLimitArgs tl, const FinalArgs fa, const RangeArgs dr,
                                                    const FrameSkipArgs fs, const RewardArgs rw) {
    RolloutArgs a = a_in;
    a.state = state_pl;
    a.n = n_pl;
    a.act_in = act_pl;
    a.pitch = pitch_pl;
    a.flags = flags_pl;
    a.ep_ret = ep_ret_pl;
    a.rec = rec_pl;
    step_body<K, false, false, ST_DEFAULT, TL, true, true, true, true>(a, block_pl, p_shared, pc_shared, tl, fa, dr, fs, rw);
}

// The single-step kernel of a handle with a disturbance (rmav_set_disturbance): k_step_rw's body and argument list with the spec behind it.
// RW: the handle has a tracking reward as well (rw is not read without it).  No CTRL form: rmav_step_control launches k_control behind
// it, with the undisturbed constants.
template <int K, bool TL, bool RW>
__global__ __launch_bounds__(kBlock) void k_step_ds(float *state_pl, int64_t n_pl, const float *act_pl, int64_t pitch_pl, uint32_t block_pl, uint32_t flags_pl,
                                                    float *ep_ret_pl, EnvRec *rec_pl, const RolloutArgs a_in, const typename Env<K>::P p_shared,
                                                    const ParamsT<double> pc_shared, const TimeLimitArgs tl, const FinalArgs fa, const RangeArgs dr,
                                                    const FrameSkipArgs fs, const RewardArgs rw, const DisturbArgs ds) {
    RolloutArgs a = a_in;
    a.state = state_pl;
    a.n = n_pl;
    a.act_in = act_pl;
    a.pitch = pitch_pl;
    a.flags = flags_pl;
    a.ep_ret = ep_ret_pl;
    a.rec = rec_pl;
    step_body<K, false, false, ST_DEFAULT, TL, true, true, true, RW, true>(a, block_pl, p_shared, pc_shared, tl, fa, dr, fs, rw, ds);
}

// rmav_disturbance_now: d of every env's NEXT step, out [3][n] (row 2 is 0 for the 2-D kinds).  ds.b0 is the block of the handle's step
// counter; the running episode's reset index is the record's reset_cnt - 1.
template <int K>
__global__ __launch_bounds__(kBlock) void k_disturbance_now(float *out, int64_t n, const EnvRec *rec, uint64_t seed, uint64_t env_base, const DisturbArgs ds) {
    constexpr int D = disturb_dim<K>();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float w[D], q[D];
    wind_draw(ds.spec(), seed, env_base + (uint64_t)i, rec[i].reset_cnt - 1u, w);
    gust_draw(ds.spec(), seed, env_base + (uint64_t)i, ds.b0, q);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[(int64_t)c * n + i] = (c < D) ? w[c < D ? c : 0] + q[c < D ? c : 0] : 0.0f;
}

// The single-step kernel of a handle with sensor noise (rmav_set_sensor_noise): k_step_ds's body and argument list with the spec behind
// it.  obs_out and final_obs are noisy (one z: that of the step counter after the step); the state stored in place is the true one.
template <int K, bool TL, bool RW>
__global__ __launch_bounds__(kBlock) void k_step_sn(float *state_pl, int64_t n_pl, const float *act_pl, int64_t pitch_pl, uint32_t block_pl, uint32_t flags_pl,
                                                    float *ep_ret_pl, EnvRec *rec_pl, const RolloutArgs a_in, const typename Env<K>::P p_shared,
                                                    const ParamsT<double> pc_shared, const TimeLimitArgs tl, const FinalArgs fa, const RangeArgs dr,
                                                    const FrameSkipArgs fs, const RewardArgs rw, const DisturbArgs ds, const SensorArgs sn) {
    RolloutArgs a = a_in;
    a.state = state_pl;
    a.n = n_pl;
    a.act_in = act_pl;
    a.pitch = pitch_pl;
    a.flags = flags_pl;
    a.ep_ret = ep_ret_pl;
    a.rec = rec_pl;
    step_body<K, false, false, ST_DEFAULT, TL, true, true, true, RW, true, true>(a, block_pl, p_shared, pc_shared, tl, fa, dr, fs, rw, ds, sn);
}

// The single-step kernel of a handle with actuator lag (rmav_set_actuator): k_step_sn's body and argument list with the filter behind it.
// m is updated in place: advanced once per dynamics sub-step, init where the env was reset.
template <int K, bool TL, bool RW>
__global__ __launch_bounds__(kBlock) void k_step_al(float *state_pl, int64_t n_pl, const float *act_pl, int64_t pitch_pl, uint32_t block_pl, uint32_t flags_pl,
                                                    float *ep_ret_pl, EnvRec *rec_pl, const RolloutArgs a_in, const typename Env<K>::P p_shared,
                                                    const ParamsT<double> pc_shared, const TimeLimitArgs tl, const FinalArgs fa, const RangeArgs dr,
                                                    const FrameSkipArgs fs, const RewardArgs rw, const DisturbArgs ds, const SensorArgs sn,
                                                    const ActuatorArgs al) {
    RolloutArgs a = a_in;
    a.state = state_pl;
    a.n = n_pl;
    a.act_in = act_pl;
    a.pitch = pitch_pl;
    a.flags = flags_pl;
    a.ep_ret = ep_ret_pl;
    a.rec = rec_pl;
    step_body<K, false, false, ST_DEFAULT, TL, true, true, true, RW, true, true, true>(a, block_pl, p_shared, pc_shared, tl, fa, dr, fs, rw, ds, sn, al);
}

// The single-step kernel of a handle with a start-state spec (rmav_set_start_state): k_step_al's body and argument list with the map behind
// the cooperative reset draw.
template <int K, bool TL, bool RW>
__global__ __launch_bounds__(kBlock) void k_step_ss(float *state_pl, int64_t n_pl, const float *act_pl, int64_t pitch_pl, uint32_t block_pl, uint32_t flags_pl,
                                                    float *ep_ret_pl, EnvRec *rec_pl, const RolloutArgs a_in, const typename Env<K>::P p_shared,
                                                    const ParamsT<double> pc_shared, const TimeLimitArgs tl, const FinalArgs fa, const RangeArgs dr,
                                                    const FrameSkipArgs fs, const RewardArgs rw, const DisturbArgs ds, const SensorArgs sn,
                                                    const ActuatorArgs al, const StartArgs ss) {
    RolloutArgs a = a_in;
    a.state = state_pl;
    a.n = n_pl;
    a.act_in = act_pl;
    a.pitch = pitch_pl;
    a.flags = flags_pl;
    a.ep_ret = ep_ret_pl;
    a.rec = rec_pl;
    step_body<K, false, false, ST_DEFAULT, TL, true, true, true, RW, true, true, true, true>(a, block_pl, p_shared, pc_shared, tl, fa, dr, fs, rw, ds, sn, al, ss);
}

// The single-step kernel of a handle with a termination spec (rmav_set_termination): k_step_ss's body and argument list with the rule behind
// every dynamics sub-step.
template <int K, bool TL, bool RW>
__global__ __launch_bounds__(kBlock) void k_step_tc(float *state_pl, int64_t n_pl, const float *act_pl, int64_t pitch_pl, uint32_t block_pl, uint32_t flags_pl,
                                                    float *ep_ret_pl, EnvRec *rec_pl, const RolloutArgs a_in, const typename Env<K>::P p_shared,
                                                    const ParamsT<double> pc_shared, const TimeLimitArgs tl, const FinalArgs fa, const RangeArgs dr,
                                                    const FrameSkipArgs fs, const RewardArgs rw, const DisturbArgs ds, const SensorArgs sn,
                                                    const ActuatorArgs al, const StartArgs ss, const TermArgs tc) {
    RolloutArgs a = a_in;
    a.state = state_pl;
    a.n = n_pl;
    a.act_in = act_pl;
    a.pitch = pitch_pl;
    a.flags = flags_pl;
    a.ep_ret = ep_ret_pl;
    a.rec = rec_pl;
    step_body<K, false, false, ST_DEFAULT, TL, true, true, true, RW, true, true, true, true, true>(a, block_pl, p_shared, pc_shared, tl, fa, dr, fs, rw, ds, sn, al, ss, tc);
}

// rmav_observe: the observation of every env's current state at the step counter b, out nS * n floats, feature-major or - aos - batch-major.
// Every route that emits an observation stores the bits this kernel gives right after it.
template <int K>
__global__ __launch_bounds__(kBlock) void k_observe(const float *state, float *out, int64_t n, uint64_t seed, uint64_t env_base, uint64_t b, uint32_t aos,
                                                    const SensorArgs sn) {
    constexpr int NS = Dims<K>::NS;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s[NS], z[NS], o[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) s[c] = state[(int64_t)c * n + i];
    sensor_draw<NS>(seed, env_base + (uint64_t)i, b, z);
    sensor_apply(sn, z, s, o);
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        if (aos) out[i * NS + c] = o[c];
        else out[(int64_t)c * n + i] = o[c];
    }
}

// reset() of every env
template <int K>
__global__ __launch_bounds__(kBlock) void k_reset(float *state, int64_t n, EnvRec *rec,
                                                  float *ep_ret, uint32_t ep_clock, float *obs_out,
                                                  uint64_t seed, uint64_t env_base, uint32_t flags) {
    constexpr int NS = Dims<K>::NS;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s[NS];
    EnvRec q = rec[i];
    const uint32_t rc = q.reset_cnt;
    if constexpr (K == REINMAV) {   // ReinmavEnv.reset() returns the current state unchanged (reinmav_env.py:348-351)
#pragma unroll
        for (int c = 0; c < NS; ++c) s[c] = state[(int64_t)c * n + i];
    } else {
        reset_state<K>(seed, env_base + (uint64_t)i, rc, s);
#pragma unroll
        for (int c = 0; c < NS; ++c) state[(int64_t)c * n + i] = s[c];
    }
    q.reset_cnt = rc + 1;
    if (flags & F_TRACK) {
        ep_ret[i] = 0.0f;
        q.ep_start = ep_clock;   // running length 0
    }
    rec[i] = q;                  // (steps_beyond_done is NOT cleared: quadrotor3d.py:182-185 does not)
    if (obs_out) {
        if (flags & F_AOS) {
#pragma unroll
            for (int c = 0; c < NS; ++c) obs_out[i * NS + c] = s[c];
        } else {
#pragma unroll
            for (int c = 0; c < NS; ++c) obs_out[(int64_t)c * n + i] = s[c];
        }
    }
}

// reset() of every env of a handle with a start-state spec (the four quadrotor kinds): k_reset whose fresh state goes through the map
template <int K>
__global__ __launch_bounds__(kBlock) void k_reset_ss(float *state, int64_t n, EnvRec *rec, float *ep_ret, uint32_t ep_clock, float *obs_out, uint64_t seed,
                                                     uint64_t env_base, uint32_t flags, const StartCoef ss) {
    static_assert(K != REINMAV, "ReinmavEnv takes no start spec");
    constexpr int NS = Dims<K>::NS;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s[NS];
    EnvRec q = rec[i];
    const uint32_t rc = q.reset_cnt;
    reset_state<K>(seed, env_base + (uint64_t)i, rc, s);
    start_apply<NS>(ss, s);
#pragma unroll
    for (int c = 0; c < NS; ++c) state[(int64_t)c * n + i] = s[c];
    q.reset_cnt = rc + 1;
    if (flags & F_TRACK) {
        ep_ret[i] = 0.0f;
        q.ep_start = ep_clock;   // running length 0
    }
    rec[i] = q;                  // (steps_beyond_done is NOT cleared, as in k_reset)
    if (obs_out) {
        if (flags & F_AOS) {
#pragma unroll
            for (int c = 0; c < NS; ++c) obs_out[i * NS + c] = s[c];
        } else {
#pragma unroll
            for (int c = 0; c < NS; ++c) obs_out[(int64_t)c * n + i] = s[c];
        }
    }
}

// control(): state -> action
template <int K>
__global__ __launch_bounds__(kBlock) void k_control(const float *state, int64_t n, float *act_out,
                                                    uint32_t flags, const ParamsT<double> pc_shared,
                                                    const float *pe_mass, const float *pe_lmass, const float *pe_L) {
    constexpr int NS = Dims<K>::NS, NA = Dims<K>::NA;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ParamsT<double> pc = pc_shared;
    if (pe_mass || pe_lmass || pe_L)
        override_params(pc, pe_mass ? (double)pe_mass[i] : pc_shared.mass, pe_lmass ? (double)pe_lmass[i] : pc_shared.load_mass,
                        pe_L ? (double)pe_L[i] : pc_shared.L);
    float s[NS], act[NA];
#pragma unroll
    for (int c = 0; c < NS; ++c) s[c] = state[(int64_t)c * n + i];
    env_control<K>(s, pc, act);
    if (flags & F_AOS) {
#pragma unroll
        for (int c = 0; c < NA; ++c) act_out[i * NA + c] = act[c];
    } else {
#pragma unroll
        for (int c = 0; c < NA; ++c) act_out[(int64_t)c * n + i] = act[c];
    }
}

}  // namespace rmav

// rmav_abi.hip - the C ABI of include/rmav.h: handle management, launches, host/device staging.
// There is deliberately no CPU implementation in this library: without a GPU rmav_create fails.
// The entry points of include/rmav_ppo.h are in rmav_ppo_abi.hip, those of include/rmav_comm.h in rmav_comm_abi.hip.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <new>

#include "rmav_ladder.hpp"
#include "rmav_core_kernels.hpp"

using namespace rmav;

namespace {

thread_local char g_err[768] = "";

}  // namespace

int rmav_fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// ---- what rmav_ppo_abi.hip shares with this unit (declared in rmav_handle.hpp) ------------------------------------------------
int ensure_scratch(rmav_handle h, size_t bytes) {
    if (bytes <= h->scratch_bytes) return RMAV_OK;
    if (h->scratch) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        HIP_TRY(hipFree(h->scratch));
        h->scratch = nullptr;
        h->scratch_bytes = 0;
    }
    size_t want = bytes + (bytes >> 2);
    if (hipMalloc(&h->scratch, want) != hipSuccess) {
        (void)hipGetLastError();
        return rmav_fail(RMAV_ERR_ALLOC, "hipMalloc(%zu) for scratch failed", want);
    }
    h->scratch_bytes = want;
    return RMAV_OK;
}

// What launch_policy_call feeds a ranged handle's kernels when the caller passed none: identity tables (allocated once) ...
int ensure_ident_norm(rmav_handle h) {
    if (h->ident_norm) return RMAV_OK;
    float tab[kNormWords] = {};
    for (int c = 0; c < 16; ++c) tab[16 + c] = 1.0f;
    tab[32] = INFINITY;
    if (hipMalloc((void **)&h->ident_norm, sizeof(tab)) != hipSuccess) {
        (void)hipGetLastError();
        h->ident_norm = nullptr;
        return rmav_fail(RMAV_ERR_ALLOC, "device allocation of the identity tables failed");
    }
    HIP_TRY(hipMemcpyAsync(h->ident_norm, tab, sizeof(tab), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));   // (tab is on this stack frame)
    return RMAV_OK;
}
// ... and, on a time-limited handle, a boot_out nobody reads (grown on demand, to exactly `bytes`)
int ensure_boot_scratch(rmav_handle h, size_t bytes) {
    if (bytes <= h->boot_scratch_bytes) return RMAV_OK;
    if (h->boot_scratch) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        HIP_TRY(hipFree(h->boot_scratch));
        h->boot_scratch = nullptr;
        h->boot_scratch_bytes = 0;
    }
    if (hipMalloc((void **)&h->boot_scratch, bytes) != hipSuccess) {
        (void)hipGetLastError();
        h->boot_scratch = nullptr;
        return rmav_fail(RMAV_ERR_ALLOC, "device allocation of %zu bytes for the unused bootstrap terms failed", bytes);
    }
    h->boot_scratch_bytes = bytes;
    return RMAV_OK;
}

RolloutArgs base_args(rmav_handle h) {
    RolloutArgs a;
    memset(&a, 0, sizeof(a));
    a.state = h->state;
    a.n = h->n;
    a.pitch = h->n;
    a.rec = h->rec;
    a.ep_ret = h->ep_ret;
    a.last_ret = h->last_ret;
    a.totals = h->totals;
    a.env_time = h->env_time;
    for (int i = 0; i < 3; ++i) a.pe[i] = h->pe[i];
    a.seed = h->seed;
    a.env_base = h->env_base;
    a.t0 = h->t;
    a.n_steps = 1;
    a.flags = h->flags & (F_AUTO_RESET | F_TRACK);
    a.act_lo = (float)h->params.act_lo;
    a.act_hi = (float)h->params.act_hi;
    return a;
}

namespace {

int check_params(const rmav_params &q) {
    if (q.integrator != RMAV_INT_EULER && q.integrator != RMAV_INT_RK4)
        return rmav_fail(RMAV_ERR_INVALID, "rmav_params.integrator must be RMAV_INT_EULER or RMAV_INT_RK4");
    if (!(q.mass > 0) || !(q.dt > 0) || !(q.tau != 0) || !(q.mass + q.load_mass > 0))
        return rmav_fail(RMAV_ERR_INVALID, "rmav_params: mass, dt must be > 0 and tau != 0");
    for (int i = 0; i < 3; ++i)
        if (!(q.g_vec[i] == q.g_vec[i]) || q.g_vec[i] - q.g_vec[i] != 0.0)
            return rmav_fail(RMAV_ERR_INVALID, "rmav_params.g_vec must be finite");
    return RMAV_OK;
}

// slots of the per-wavefront episode totals: one per 32 envs (the fp32-MFMA policy mode runs 32 envs per wavefront)
// + 4: k_step reads its wavefront's slot in EVERY wavefront of the launch grid, also in those of the last 256-thread workgroup that lie
// wholly past N (they add nothing and write nothing); the padding keeps those reads inside the array
inline size_t n_total_slots(int64_t n) { return (size_t)((n + 31) / 32) + 4; }

// Host-pointer calls that move at most this many bytes go through the pinned block (zero-copy); bigger ones
// stage through device scratch with hipMemcpyAsync, which is the faster route for bulk data.
constexpr size_t kPinnedMax = 256u << 10;

int ensure_pinned(rmav_handle h, size_t bytes) {
    if (bytes <= h->pinned_bytes) return RMAV_OK;
    if (h->pinned) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        HIP_TRY(hipHostFree(h->pinned));
        h->pinned = h->pinned_dev = nullptr;
        h->pinned_bytes = 0;
    }
    size_t want = bytes < 4096 ? 4096 : bytes;
    if (hipHostMalloc(&h->pinned, want, hipHostMallocMapped) != hipSuccess) {
        (void)hipGetLastError();
        h->pinned = nullptr;
        return rmav_fail(RMAV_ERR_ALLOC, "hipHostMalloc(%zu) for the pinned staging block failed", want);
    }
    if (hipHostGetDevicePointer(&h->pinned_dev, h->pinned, 0) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipHostFree(h->pinned);
        h->pinned = nullptr;
        return rmav_fail(RMAV_ERR_HIP, "hipHostGetDevicePointer failed");
    }
    h->pinned_bytes = want;
    return RMAV_OK;
}

// Cache policy of the trajectory stores for one launch.  Measured with COLD trajectory buffers (bench.py's ring of
// buffer sets; profiles/r02/policy_split_sweep.md), 64-step launches, every kind, 65 536 .. 1 048 576 envs:
//   two-wavefront kernel : write-through (sc0 sc1) is best or within 1 % of best everywhere
//   one-wavefront kernel : non-temporal (nt) is best from 131 072 envs up (+3..7 % over the default policy, which is
//                          never the best choice for a fused launch); small trajectories that stay in the Infinity
//                          Cache for their consumer keep write-through
// Single-step and very short launches use the default policy.  rmav_set_tuning(RMAV_TUNE_STORE_POLICY, 0|1|2|3) overrides.
int pick_store_policy(rmav_handle h, const RolloutArgs &a, bool split) {
    const int forced = h->tune[RMAV_TUNE_STORE_POLICY];
    if (forced >= 0 && forced <= 2 && !(a.flags & F_AOS)) return forced;
    if (a.n_steps < 8 && !split) return ST_DEFAULT;
    double per_step = 0.0;
    if (a.act_out) per_step += 4.0 * kActionDim[h->kind];
    if (a.obs_out) per_step += 4.0 * kStateDim[h->kind];
    if (a.rew_out) per_step += 4.0;
    if (a.done_out) per_step += 1.0;
    const double bytes = per_step * (double)h->n * (double)a.n_steps;
    if (a.flags & F_AOS) {   // batch-major trajectories: LDS-transposed obs stores once the launch is big (RMAV_TUNE_STORE_POLICY 3: always, 0: never)
        if (forced == 0) return ST_DEFAULT;
        if (split) return ST_WRITE_THROUGH;   // the memory wavefront drains batch-major tiles itself
        // measured (profiles/r01/layout_sweep.md): pays from 131 072 envs x 64 steps (512 MB), costs 10-15 % at 65 536 (256 MB)
        return (a.obs_out && (bytes >= 448.0e6 || forced == ST_AOS_LDS)) ? ST_AOS_LDS : ST_WRITE_THROUGH;
    }
    // Feature-major columns are 4 N bytes apart: unless N is a multiple of 16 they start off a 64-byte line, every wavefront's
    // 256-byte store ends in partial lines, and only the write-back L2 can merge them with the neighbouring wavefront's part -
    // write-through / non-temporal stores send the fragments on (same box: 65 599 envs 100.4 us per launch, write-back 67.7;
    // 131 071: 200.9 -> 116.5; 1 048 575: 1700 -> 1564; the aligned sizes next to them: 48.8, 90.8, 730).
    if ((a.pitch & 15) != 0) return ST_DEFAULT;   // (rmav_rollout_pitched: the caller padded the columns, the batch size is free)
    if (split) return ST_WRITE_THROUGH;
    return bytes <= 192.0e6 ? ST_WRITE_THROUGH : ST_STREAM;
}

// Two-wavefront (integrator + memory wavefront) kernel or one wavefront per 64 envs?  Measured on cold trajectory
// buffers (profiles/r02/split_autog.md: every kind, both in-kernel action sources, 16 384 .. 163 840 envs): the
// two-wavefront kernel wins or ties whenever the whole batch fits ONE workgroup per CU - ceil(N / 16 384) pairs per
// workgroup, 256 workgroups - and loses as soon as it does not (a second round of workgroups, or pairs capped by the
// 1024-thread / 160 KiB-LDS limits).  So the rule is capacity, not a tuned constant: two wavefronts iff
// N <= 16 384 x (pairs that fit one workgroup for this kind and action source).
template <int K, int SMODE> constexpr int split_pairs_max() {   // SMODE: ACT_RANDOM_SPLIT | ACT_CONTROLLER_SPLIT | ACT_BUFFER_SPLIT
    constexpr int by_lds = (int)((160u << 10) / (sizeof(float) * split_words_per_pair<K, SMODE>()));
    constexpr int cap = split_group_cap<K, split_feeds_actions(SMODE)>();   // threads / registers (rmav_kernels.hpp)
    return by_lds < cap ? by_lds : cap;
}
#define RMAV_PAIRS(SMODE) {split_pairs_max<QUAD2D, SMODE>(), split_pairs_max<QUAD2D_SL, SMODE>(), split_pairs_max<QUAD3D, SMODE>(), split_pairs_max<QUAD3D_SL, SMODE>()}
constexpr int kSplitPairsRandom[4] = RMAV_PAIRS(ACT_RANDOM_SPLIT);
constexpr int kSplitPairsController[4] = RMAV_PAIRS(ACT_CONTROLLER_SPLIT);
constexpr int kSplitPairsBuffer[4] = RMAV_PAIRS(ACT_BUFFER_SPLIT);
#undef RMAV_PAIRS
// pairs of one workgroup by the public action mode
inline const int *split_pairs_of(int action_mode) {
    return action_mode == RMAV_ACT_CONTROLLER ? kSplitPairsController : action_mode == RMAV_ACT_BUFFER ? kSplitPairsBuffer : kSplitPairsRandom;
}
constexpr int64_t kEnvsPerCuSlot = 16384;   // 256 CUs x 64 envs: one pair per CU
constexpr bool kSliceByDefault = false;     // sliced two-wavefront launches beyond the capacity: measured, see DESIGN.md

template <int K, int MODE, int ST>
int launch_rollout_kms(rmav_handle h, const RolloutArgs &a_in) {
    RolloutArgs a = a_in;
    take_armed_exchange(h, a, 64, publishes_start(MODE));
    const KindParams<K> kp = kind_params<K>(h);
    static_assert(!is_policy(MODE), "the policy-in-kernel rollouts are launched from rmav_policy_abi.hip");
    const size_t lds = (ST == ST_AOS_LDS) ? sizeof(float) * AosTile<Dims<K>::NS>::WORDS * (block_size(h) / 64) : 0;
    if constexpr (is_split(MODE)) {
        // (integrator, memory wavefront) pairs: as many per workgroup as make ONE workgroup per CU (256 workgroups),
        // within 1024 threads and the CU's 160 KiB of LDS.  RMAV_TUNE_SPLIT_GROUP = 1..8 overrides.
        constexpr size_t lds_per_pair = sizeof(float) * split_words_per_pair<K, MODE>();
        const int forced = h->tune[RMAV_TUNE_SPLIT_GROUP];
        constexpr int g_max = split_pairs_max<K, MODE>();
        const int64_t count = a.slice_count ? (int64_t)a.slice_count : h->n;   // envs of this launch
        // Round 3 (profiles/r03/pairs_per_workgroup.md): one s_barrier synchronises ALL pairs of a workgroup, so every pair
        // pays for the slowest one's reset path each step.  Where the step time is the integrator's latency (the 2-D kinds,
        // whose steps move half the bytes, and every controller-driven rollout: fp64 controller in the integrator) rather than
        // the store stream, ONE pair per workgroup is faster: 65 536 envs quadrotor2d-slungload 47.2 -> 43.1 us per 64-step launch,
        // controller-driven quadrotor3d 56.7 -> 52.3.  The store-bound combinations (3-D kinds with random / caller actions) keep
        // one workgroup per CU (adjacent pairs store adjacent 256-byte segments: 65 536 envs quadrotor3d 41.6 vs 50.7 us), and so
        // do the others at 131 072 envs, where two pairs share every SIMD anyway (quadrotor2d excepted: 51.6 vs 54.5).
        constexpr bool latency_bound = (K == QUAD2D || K == QUAD2D_SL) || MODE == ACT_CONTROLLER_SPLIT;
        const bool one_pair = latency_bound && (count <= 98304 || K == QUAD2D);
        int g = (forced >= 1 && forced <= g_max) ? forced : one_pair ? 1 : (int)((count + kEnvsPerCuSlot - 1) / kEnvsPerCuSlot);
        if (g < 1) g = 1;
        if (g > g_max) g = g_max;
        const int64_t per_wg = 64 * g;
        // lean addressing in the memory wavefront: feature-major, every trajectory array below 4 GiB (32-bit scalar step offsets)
        if (!(a.flags & F_AOS) && (int64_t)a.n_steps * Dims<K>::NS * a.pitch < ((int64_t)1 << 30)) a.flags |= F_LEAN;
        const dim3 grid((unsigned)((count + per_wg - 1) / per_wg)), block(128 * g);
        bool launched = false;
        if constexpr (ST == ST_WRITE_THROUGH) {   // the usual options, compiled in (k_rollout's FIXED)
            if ((a.flags & (F_AOS | F_TRACK | F_AUTO_RESET)) == (F_TRACK | F_AUTO_RESET)) {
                hipLaunchKernelGGL((k_rollout<K, MODE, ST, true>), grid, block, lds_per_pair * g, h->stream, a, kp.p, kp.pc);
                launched = true;
            }
        }
        if (!launched) hipLaunchKernelGGL((k_rollout<K, MODE, ST>), grid, block, lds_per_pair * g, h->stream, a, kp.p, kp.pc);
    } else if (const Rung r = rung_of(h)) {   // a handle on the feature ladder: the highest rung's kernels, which take what every rung below takes as well
        if constexpr (K != REINMAV && (MODE == ACT_BUFFER || MODE == ACT_RANDOM || MODE == ACT_CONTROLLER)) {
            if (int rc = kLadder[r].rollout(h, MODE, ST, a)) return rc;   // (the rungs above the tracking reward have one store policy and ignore ST)
        } else {
            return rmav_fail(RMAV_ERR_INVALID, "no %s kernel for action mode %d", kLadder[r].noun, MODE);
        }
    } else {
        if (h->time_limit > 0) {   // (one launch per chunk of a chunk-major call: launch_rollout_km)
            // (ACT_BUFFER_CTRL comes here only with n_steps > 1, which no entry point asks for: its single steps run k_step_tl)
            if constexpr (K != REINMAV && (MODE == ACT_BUFFER || MODE == ACT_RANDOM || MODE == ACT_CONTROLLER)) {
                const int64_t count = a.slice_count ? (int64_t)a.slice_count : h->n;
                const dim3 grid((unsigned)((count + block_size(h) - 1) / block_size(h)));
                hipLaunchKernelGGL((k_rollout_tl<K, MODE, ST>), grid, dim3(block_size(h)), lds, h->stream, a, kp.p, kp.pc, tl_args(h));
            } else {
                return rmav_fail(RMAV_ERR_INVALID, "no time-limited kernel for action mode %d", MODE);
            }
        } else {
            hipLaunchKernelGGL((k_rollout<K, MODE, ST>), grid_for(h), dim3(block_size(h)), lds, h->stream, a, kp.p, kp.pc);
        }
    }
    return check_rollout_launch(h, a);
}

// RMAV_TUNE_SPLIT = 0 | 1 overrides the rule.
// Batches beyond that capacity can still run on the two-wavefront kernel as a sequence of launches over balanced
// slices of the env range, each one workgroup per CU (`slices` > 1): see launch_rollout_km.  RMAV_TUNE_SLICE = 0 | 1 overrides.
bool use_split(rmav_handle h, const RolloutArgs &a, int action_mode, int *slices, bool random_actions) {
    const int forced = h->tune[RMAV_TUNE_SPLIT], slice_forced = h->tune[RMAV_TUNE_SLICE];
    *slices = 1;
    if (h->chunk > 0) {   // rmav_rollout_chunked: one two-wavefront launch per chunk, whatever the other rules say
        *slices = (int)((h->n + h->chunk - 1) / h->chunk);
        return true;
    }
    // the two-wavefront kernel also wins for short launches (2 .. 7 steps: -15 .. -30 %, measured)
    if (a.n_steps < 2 || h->kind > RMAV_QUAD3D_SL) return false;
    const int64_t cap = kEnvsPerCuSlot * split_pairs_of(action_mode)[h->kind];
    if (forced == 0) return false;
    if (h->n <= cap) return true;
    // Two rounds of the two-wavefront kernel - two launches over balanced halves of the env range - beat one launch of the
    // one-wavefront kernel for the slung-load kinds (fp64 integrator: the one-wavefront kernel holds only 3-4 of them per SIMD)
    // when both halves (nearly) fill the machine, 1.75 .. 2 x the capacity, random actions (profiles/r02/slice_two_rounds.md:
    // BASELINE C4 = quadrotor3d-slungload at 262 144 envs 269-292 -> 249-252 us, quadrotor2d-slungload 172 -> 158).  Smaller
    // second halves, more than two rounds, the plain kinds (quadrotor3d: +-4 %, quadrotor2d: slower) and the
    // controller-driven rollouts measured equal or slower, so they stay on one launch.
    const bool two_rounds = random_actions && (h->kind == RMAV_QUAD3D_SL || h->kind == RMAV_QUAD2D_SL) && h->n <= 2 * cap &&
                            4 * h->n >= 7 * cap;
    if (slice_forced == 1 || (slice_forced != 0 && (kSliceByDefault || two_rounds))) {
        *slices = (int)((h->n + cap - 1) / cap);
        return true;
    }
    return forced == 1;   // one launch beyond the capacity: only when asked for
}

// The launch over the envs [first, first + per) of a call that is cut into several: a slice of the env range, and with chunk-major
// trajectory arrays [n_chunks][T][dim][chunk] (rmav_rollout_chunked, per = chunk) the slice's chunk is a dense region of its own with
// column pitch `chunk`; the kernels index columns by the env's index in the handle, so the base pointers are moved back by `first`
// columns (a multiple of 64 elements: alignment is kept)
template <int K> RolloutArgs slice_args(rmav_handle h, const RolloutArgs &a, int64_t first, int64_t per) {
    RolloutArgs b = a;
    b.slice_first = (uint32_t)first;
    b.slice_count = (uint32_t)((h->n - first < per) ? h->n - first : per);
    if (h->chunk > 0) {
        const int64_t c = first / per, T = a.n_steps;
        constexpr int64_t NS = Dims<K>::NS, NA = Dims<K>::NA;
        b.pitch = per;
        if (a.act_in) b.act_in = a.act_in + c * T * NA * per - first;
        if (a.act_out) b.act_out = a.act_out + c * T * NA * per - first;
        if (a.obs_out) b.obs_out = a.obs_out + c * T * NS * per - first;
        if (a.rew_out) b.rew_out = a.rew_out + c * T * per - first;
        if (a.done_out) b.done_out = a.done_out + c * T * per - first;
    }
    return b;
}

template <int K, int MODE>
int launch_rollout_km(rmav_handle h, const RolloutArgs &a) {
    constexpr bool has_split = (MODE == ACT_RANDOM || MODE == ACT_CONTROLLER || MODE == ACT_BUFFER) && K != REINMAV;
    // A handle with an episode time limit runs the one-wavefront kernels (k_rollout_tl): the two-wavefront kernels have no time-limited
    // variant, so RMAV_TUNE_SPLIT / RMAV_TUNE_SLICE do not apply; a chunk-major call is one launch per chunk.
    // A handle on the feature ladder (rmav_ladder.hpp) likewise: the one-wavefront kernels of its rung, k_rollout_dr ... k_rollout_tc.
    if (K != REINMAV && (h->time_limit > 0 || rung_of(h) != RUNG_NONE)) {
        if (h->chunk > 0) {
            for (int64_t first = 0; first < h->n; first += h->chunk) {
                const RolloutArgs b = slice_args<K>(h, a, first, h->chunk);
                // (chunk-major is feature-major: ST_AOS_LDS does not come up)
                if (int rc = dispatch_store<ST_DEFAULT, ST_WRITE_THROUGH, ST_STREAM>(
                        pick_store_policy(h, b, false), [&](auto st) { return launch_rollout_kms<K, MODE, decltype(st)::value>(h, b); }))
                    return rc;
            }
            return RMAV_OK;
        }
    } else if constexpr (has_split) {
        constexpr int SMODE = (MODE == ACT_RANDOM) ? ACT_RANDOM_SPLIT : (MODE == ACT_BUFFER) ? ACT_BUFFER_SPLIT : ACT_CONTROLLER_SPLIT;
        int slices = 1;
        if (use_split(h, a, MODE == ACT_CONTROLLER ? RMAV_ACT_CONTROLLER : MODE == ACT_BUFFER ? RMAV_ACT_BUFFER : RMAV_ACT_RANDOM, &slices, MODE == ACT_RANDOM)) {
            // balanced slices, each a multiple of 64 envs
            const int64_t per = h->chunk > 0 ? h->chunk : slices > 1 ? (((h->n + slices - 1) / slices + 63) / 64) * 64 : h->n;
            RolloutArgs ap = a;
            if (h->chunk > 0) ap.pitch = per;   // chunk-major columns are `chunk` (a multiple of 64) apart whatever N is
            const int st = pick_store_policy(h, ap, true);
            for (int64_t first = 0; first < h->n; first += per) {
                const RolloutArgs b = (slices > 1 || h->chunk > 0) ? slice_args<K>(h, a, first, per) : a;
                if (int rc = dispatch_store<ST_WRITE_THROUGH, ST_STREAM, ST_DEFAULT>(
                        st, [&](auto s) { return launch_rollout_kms<K, SMODE, decltype(s)::value>(h, b); }))
                    return rc;
            }
            return RMAV_OK;
        }
    }
    // one launch of the one-wavefront kernel: every store policy
    return dispatch_store<ST_DEFAULT, ST_WRITE_THROUGH, ST_STREAM, ST_AOS_LDS>(
        pick_store_policy(h, a, false), [&](auto st) { return launch_rollout_kms<K, MODE, decltype(st)::value>(h, a); });
}

template <int K> int launch_rollout_k(rmav_handle h, int mode, const RolloutArgs &a) {
    switch (mode) {
    case RMAV_ACT_BUFFER: return launch_rollout_km<K, ACT_BUFFER>(h, a);
    case RMAV_ACT_RANDOM: return launch_rollout_km<K, ACT_RANDOM>(h, a);
    case RMAV_ACT_CONTROLLER: return launch_rollout_km<K, ACT_CONTROLLER>(h, a);
    case ACT_BUFFER_CTRL: return launch_rollout_kms<K, ACT_BUFFER_CTRL, ST_DEFAULT>(h, a);   // internal (rmav_step_control)
    }
    return rmav_fail(RMAV_ERR_INVALID, "unknown action_mode %d", mode);
}

// k_step's launch rules by batch size (profiles/r05/step_sweep.md; every variant writes the same bits).  Up to ~196 608 envs a
// launch is mostly launch latency: eager bookkeeping loads (a dependent round trip costs more than the 12 B it saves), 256-thread
// workgroups, write-back stores.  Up to ~786 432 envs: non-temporal stores (7.0 -> 6.7-6.9 us at 262 144).  Beyond: bookkeeping
// loaded only in lanes whose env terminates and 128-thread workgroups (1 048 576 envs 26.4 -> 23.5 us, 4 194 304: 92.9 -> 78.9).
// rmav_set_tuning(RMAV_TUNE_STEP_LAZY | _BLOCK | _STEP_STORE) overrides each.
inline bool step_lazy(rmav_handle h) {
    const int t = h->tune[RMAV_TUNE_STEP_LAZY];
    return t >= 0 ? t == 1 : h->n >= 786432;
}
inline int step_block(rmav_handle h) {
    const int v = h->tune[RMAV_TUNE_BLOCK];
    return (v == 64 || v == 128 || v == 256) ? v : (h->n >= 786432 ? 128 : 256);
}
inline int step_store(rmav_handle h) {
    const int v = h->tune[RMAV_TUNE_STEP_STORE];
    return v >= 0 ? v : ((h->n >= 196608 && h->n < 786432) ? (int)ST_STREAM : (int)ST_DEFAULT);
}

// k_step / k_step_tl / k_step_final at `bs` threads per workgroup.  The leading scalars are what the kernel's first loads need:
// preloaded into scalar registers, see StepHot in rmav_kernels.hpp; `tail` is what the kernel takes behind k_step's arguments.
template <int K, typename Kernel, typename... Tail>
void launch_step_hot(rmav_handle h, const RolloutArgs &a, const KindParams<K> &kp, int bs, Kernel kernel, const Tail &...tail) {
    const dim3 grid((unsigned)((h->n + bs - 1) / bs));
    hipLaunchKernelGGL(kernel, grid, dim3(bs), 0, h->stream, a.state, a.n, a.act_in, a.pitch, (uint32_t)bs, a.flags, a.ep_ret, a.rec, a, kp.p, kp.pc, tail...);
}

int launch_control(rmav_handle h, float *act_dev, int layout);

// n_steps == 1 with caller actions: the latency-cut single-step kernel
template <int K> int launch_step_k(rmav_handle h, const RolloutArgs &a, bool ctrl) {
    if (h->xchg.armed && h->xchg.fired) h->xchg.stale = true;   // the armed launch's snapshot is no longer the latest
    const KindParams<K> kp = kind_params<K>(h);
    const int st = step_store(h), bs = step_block(h);
    if (const Rung r = rung_of(h)) {   // a handle on the feature ladder: its rung's k_step_* for every batch size (eager record load, default store policy)
        if (int rc = kLadder[r].step(h, a, ctrl, bs, FinalArgs{})) return rc;
        if (ctrl && kLadder[r].control_behind)   // (only the ranged kernel has a form that ends with control(): k_control behind the others)
            if (int rc = launch_control(h, a.ctrl_out, (a.flags & F_AOS) ? RMAV_AOS : RMAV_SOA)) return rc;
    } else if (h->time_limit > 0) {   // every batch size: the eager record load, k_step's preloaded arguments (k_step_tl)
        const TimeLimitArgs tl = tl_args(h);
        if (ctrl) launch_step_hot(h, a, kp, bs, k_step_tl<K, true>, tl);
        else dispatch_store<ST_DEFAULT, ST_WRITE_THROUGH, ST_STREAM>(st, [&](auto s) { launch_step_hot(h, a, kp, bs, k_step_tl<K, false, decltype(s)::value>, tl); });
    } else if (ctrl) {
        launch_step_hot(h, a, kp, bs, k_step<K, true>);
    } else {
        const bool big = h->n >= 786432;   // no argument preloading for the big batches (k_step_big in rmav_kernels.hpp says why)
        dispatch_store<ST_DEFAULT, ST_WRITE_THROUGH, ST_STREAM>(st, [&](auto s) {
            constexpr int ST = decltype(s)::value;
            auto launch = [&](auto lazy) {
                constexpr bool LAZY = decltype(lazy)::value;
                if (big) hipLaunchKernelGGL((k_step_big<K, LAZY, ST>), dim3((unsigned)((h->n + bs - 1) / bs)), dim3(bs), 0, h->stream, a, kp.p, kp.pc);
                else launch_step_hot(h, a, kp, bs, k_step<K, false, LAZY, ST>);
            };
            if (step_lazy(h)) launch(std::true_type{});
            else launch(std::false_type{});
        });
    }
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

// rmav_step_final: k_step_final<K, TL, ST> at k_step_tl's launch shape (eager record load and preloaded leading arguments for every batch size)
template <int K> int launch_step_final_k(rmav_handle h, const RolloutArgs &a, const FinalArgs &fa) {
    if (h->xchg.armed && h->xchg.fired) h->xchg.stale = true;
    const KindParams<K> kp = kind_params<K>(h);
    const int bs = step_block(h);
    const TimeLimitArgs tl = tl_args(h);
    if (const Rung r = rung_of(h)) {
        if (int rc = kLadder[r].step(h, a, false, bs, fa)) return rc;
    } else dispatch_store<ST_DEFAULT, ST_WRITE_THROUGH, ST_STREAM>(step_store(h), [&](auto s) {
        constexpr int ST = decltype(s)::value;
        if (h->time_limit > 0) launch_step_hot(h, a, kp, bs, k_step_final<K, true, ST>, tl, fa);
        else launch_step_hot(h, a, kp, bs, k_step_final<K, false, ST>, tl, fa);
    });
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}
int launch_step_final(rmav_handle h, const RolloutArgs &a, const FinalArgs &fa) {
    return dispatch_kind<QUAD_KINDS>(h->kind, [&](auto k) { return launch_step_final_k<decltype(k)::value>(h, a, fa); });
}

int launch_rollout(rmav_handle h, int mode, const RolloutArgs &a) {
    if (a.n_steps == 1 && (mode == RMAV_ACT_BUFFER || mode == ACT_BUFFER_CTRL) && h->kind != RMAV_REINMAV)
        return dispatch_kind<QUAD_KINDS>(h->kind, [&](auto k) { return launch_step_k<decltype(k)::value>(h, a, mode == ACT_BUFFER_CTRL); });
    return dispatch_kind<ALL_KINDS>(h->kind, [&](auto k) { return launch_rollout_k<decltype(k)::value>(h, mode, a); });
}

int launch_reset(rmav_handle h, float *obs_dev, int layout) {
    if (h->start_on) return rmav_launch_start_reset(h, obs_dev, layout);   // a handle with a start-state spec: k_reset_ss
    const uint32_t fl = (h->flags & F_TRACK) | (layout == RMAV_AOS ? F_AOS : 0u);
    return dispatch_kind<ALL_KINDS>(h->kind, [&](auto k) {
        hipLaunchKernelGGL((k_reset<decltype(k)::value>), grid_for(h), dim3(block_size(h)), 0, h->stream, h->state, h->n, h->rec, h->ep_ret,
                           (uint32_t)h->t, obs_dev, h->seed, h->env_base, fl);
        HIP_TRY(hipGetLastError());
        return (int)RMAV_OK;
    });
}

// The running episode of every env starts at the handle's clock: ep_start = clock (what k_reset does when the handle tracks episodes).
int restart_episode_clocks(rmav_handle h) {
    hipLaunchKernelGGL(k_rec_fill, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, h->stream, h->rec, EnvRec{0, 0u, (uint32_t)h->t, 0}, 2,
                       (int64_t)h->n);
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

// rmav_reset: k_reset keeps ep_start only when the handle tracks episodes; a time-limited handle that does not gets it restarted by
// the record fill behind it (k_reset itself is unchanged)
// The device copy of the handle's ranges (k_rollout_nrm_dr reads them through a pointer): rewritten, in stream order, whenever they change.
int sync_range_dev(rmav_handle h) {
    if (!h->range_dev && hipMalloc((void **)&h->range_dev, sizeof(RangeArgs)) != hipSuccess) {
        (void)hipGetLastError();
        h->range_dev = nullptr;
        return rmav_fail(RMAV_ERR_ALLOC, "device allocation failed");
    }
    const RangeArgs r = range_args(h);
    HIP_TRY(hipMemcpyAsync(h->range_dev, &r, sizeof(r), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));   // (r is on this stack frame)
    return RMAV_OK;
}

// The constants of the running episodes of the parameters in `mask`, drawn from their ranges (k_range_draw).
int launch_range_draw(rmav_handle h, uint32_t mask) {
    hipLaunchKernelGGL(k_range_draw, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, h->stream, range_args(h, mask), (const EnvRec *)h->rec,
                       (int64_t)h->n, h->seed, h->env_base);
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

// ... and a handle with parameter ranges redraws its constants behind it, for the reset index k_reset has just used.
int launch_reset_tl(rmav_handle h, float *obs_dev, int layout) {
    if (int rc = launch_reset(h, obs_dev, layout)) return rc;
    if (h->range_mask)
        if (int rc = launch_range_draw(h, h->range_mask)) return rc;
    if (h->time_limit > 0 && !(h->flags & RMAV_F_TRACK_EPISODES)) return restart_episode_clocks(h);
    return RMAV_OK;
}

// last_trunc on first use: N zero bytes (no episode has been truncated yet)
int ensure_last_trunc(rmav_handle h) {
    if (h->last_trunc) return RMAV_OK;
    if (hipMalloc((void **)&h->last_trunc, (size_t)h->n) != hipSuccess) {
        (void)hipGetLastError();
        h->last_trunc = nullptr;
        return rmav_fail(RMAV_ERR_ALLOC, "device allocation of the truncated flags failed");
    }
    HIP_TRY(hipMemsetAsync(h->last_trunc, 0, (size_t)h->n, h->stream));
    return RMAV_OK;
}

int launch_control(rmav_handle h, float *act_dev, int layout) {
    const uint32_t fl = (layout == RMAV_AOS ? F_AOS : 0u);
    return dispatch_kind<ALL_KINDS>(h->kind, [&](auto k) {
        constexpr int K = decltype(k)::value;
        if constexpr (K == REINMAV)
            hipLaunchKernelGGL(k_control_reinmav, grid_for(h), dim3(block_size(h)), 0, h->stream, h->state, h->env_time, h->n, act_dev, fl,
                               derive_reinmav(h->params));
        else
            hipLaunchKernelGGL((k_control<K>), grid_for(h), dim3(block_size(h)), 0, h->stream, h->state, h->n, act_dev, fl,
                               derive<double>(h->params, K == QUAD2D || K == QUAD2D_SL), h->pe[0], h->pe[1], h->pe[2]);
        HIP_TRY(hipGetLastError());
        return (int)RMAV_OK;
    });
}

int check_mem_layout(int mem, int layout) {
    if (mem != RMAV_HOST && mem != RMAV_DEVICE) return rmav_fail(RMAV_ERR_INVALID, "mem must be RMAV_HOST or RMAV_DEVICE");
    if (layout != RMAV_SOA && layout != RMAV_AOS) return rmav_fail(RMAV_ERR_INVALID, "layout must be RMAV_SOA or RMAV_AOS");
    return RMAV_OK;
}

// Generic "copy a per-env array out of / into the handle".
template <typename T> int copy_out(rmav_handle h, const T *dev, T *out, size_t count, int mem) {
    if (!out) return rmav_fail(RMAV_ERR_INVALID, "output pointer is NULL");
    if (mem == RMAV_DEVICE) {
        HIP_TRY(hipMemcpyAsync(out, dev, count * sizeof(T), hipMemcpyDeviceToDevice, h->stream));
    } else if (count * sizeof(T) <= kPinnedMax && ensure_pinned(h, count * sizeof(T)) == RMAV_OK) {
        // pinned target: a true asynchronous DMA, then one synchronise (a pageable target makes the runtime stage and block)
        HIP_TRY(hipMemcpyAsync(h->pinned, dev, count * sizeof(T), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        memcpy(out, h->pinned, count * sizeof(T));
    } else {
        HIP_TRY(hipMemcpyAsync(out, dev, count * sizeof(T), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return RMAV_OK;
}
template <typename T> int copy_in(rmav_handle h, T *dev, const T *in, size_t count, int mem) {
    if (!in) return rmav_fail(RMAV_ERR_INVALID, "input pointer is NULL");
    if (mem == RMAV_DEVICE) {
        HIP_TRY(hipMemcpyAsync(dev, in, count * sizeof(T), hipMemcpyDeviceToDevice, h->stream));
    } else {
        HIP_TRY(hipMemcpyAsync(dev, in, count * sizeof(T), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return RMAV_OK;
}

// A kernel writes `bytes` to a device destination and the caller may have passed a host pointer: launch(dst) runs on the caller's device
// pointer, on the pinned block (zero-copy: up to kPinnedMax) or on device scratch that is then copied out.
template <typename F> int write_via_host(rmav_handle h, void *out, size_t bytes, int mem, F &&launch) {
    if (mem == RMAV_DEVICE || !out) return launch(out);
    if (bytes <= kPinnedMax && ensure_pinned(h, bytes) == RMAV_OK) {
        if (int rc = launch(h->pinned_dev)) return rc;
        HIP_TRY(hipStreamSynchronize(h->stream));
        memcpy(out, h->pinned, bytes);
        return RMAV_OK;
    }
    if (int rc = ensure_scratch(h, bytes)) return rc;
    if (int rc = launch(h->scratch)) return rc;
    return copy_out(h, (const char *)h->scratch, (char *)out, bytes, RMAV_HOST);
}

// One 32-bit field of the per-env records (EnvRec: 0 sbd, 1 reset_cnt, 2 ep_start, 3 last_len) as a dense array: the state accessors
// of the ABI gather / scatter it with one small kernel (host pointers: through device scratch)
int rec_field_get(rmav_handle h, int field, uint32_t *out, int mem) {
    if (!out) return rmav_fail(RMAV_ERR_INVALID, "output pointer is NULL");
    const size_t n = (size_t)h->n;
    uint32_t *dst = out;
    if (mem != RMAV_DEVICE) {
        if (int rc = ensure_scratch(h, n * sizeof(uint32_t))) return rc;
        dst = (uint32_t *)h->scratch;
    }
    hipLaunchKernelGGL(k_rec_get, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, dst, (const EnvRec *)h->rec, field, (int64_t)n);
    HIP_TRY(hipGetLastError());
    return mem == RMAV_DEVICE ? RMAV_OK : copy_out(h, (const uint32_t *)dst, out, n, RMAV_HOST);
}
int rec_field_set(rmav_handle h, int field, const uint32_t *in, int mem) {
    if (!in) return rmav_fail(RMAV_ERR_INVALID, "input pointer is NULL");
    const size_t n = (size_t)h->n;
    const uint32_t *src = in;
    if (mem != RMAV_DEVICE) {
        if (int rc = ensure_scratch(h, n * sizeof(uint32_t))) return rc;
        if (int rc = copy_in(h, (uint32_t *)h->scratch, in, n, RMAV_HOST)) return rc;
        src = (const uint32_t *)h->scratch;
    }
    hipLaunchKernelGGL(k_rec_set, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->rec, src, field, (int64_t)n);
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

// The handle's stream: the caller's, or one of its own when hip_stream is NULL.
int adopt_stream(rmav_handle h, void *hip_stream) {
    h->own_stream = false;
    if (hip_stream) {
        // (void*)1 names the legacy default stream, whose real handle is 0: use that (some runtime entry points -
        // hipEventRecord - do not accept the hipStreamLegacy constant)
        h->stream = (hip_stream == (void *)1) ? nullptr : (hipStream_t)hip_stream;
        return RMAV_OK;
    }
    HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->own_stream = true;
    return RMAV_OK;
}

void free_all(rmav_handle h) {
    void *ptrs[] = {h->arena, h->pe[0], h->pe[1], h->pe[2], h->scratch};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    if (h->pinned) (void)hipHostFree(h->pinned);
    if (h->done_flag) (void)hipHostFree(h->done_flag);
    if (h->last_trunc) (void)hipFree(h->last_trunc);
    if (h->range_dev) (void)hipFree(h->range_dev);
    if (h->ident_norm) (void)hipFree(h->ident_norm);
    if (h->boot_scratch) (void)hipFree(h->boot_scratch);
    if (h->actuator_m) (void)hipFree(h->actuator_m);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    h->magic = 0;
    delete h;
}

}  // namespace

int ensure_range_dev(rmav_handle h) { return h->range_dev ? (int)RMAV_OK : sync_range_dev(h); }

// =================================================================================================
extern "C" {

int rmav_version(void) { return RMAV_VERSION; }

const char *rmav_last_error(void) { return g_err; }

int rmav_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n < 0 ? 0 : n;
}

int rmav_state_dim(int kind) { return (kind < 0 || kind >= kNumKinds) ? -1 : kStateDim[kind]; }
int rmav_action_dim(int kind) { return (kind < 0 || kind >= kNumKinds) ? -1 : kActionDim[kind]; }

int rmav_algorithmic_bytes(int kind) {
    if (kind < 0 || kind >= kNumKinds) return -1;
    // read state + read action + write state + write reward (f32) + write done (u8)
    return 4 * (2 * kStateDim[kind] + kActionDim[kind] + 1) + 1;
}

int rmav_default_params(int kind, int reading_2d, rmav_params *p) {
    if (kind < 0 || kind >= kNumKinds) return rmav_fail(RMAV_ERR_INVALID, "bad kind %d", kind);
    if (!p) return rmav_fail(RMAV_ERR_INVALID, "out is NULL");
    if (reading_2d != 0 && reading_2d != 'A' && reading_2d != 'B')
        return rmav_fail(RMAV_ERR_INVALID, "reading_2d must be 0, 'A' or 'B'");
    memset(p, 0, sizeof(*p));
    p->mass = 1.0;
    p->load_mass = 0.1;
    p->dt = 0.01;
    p->g = 9.8;
    // self.g: (0, 0, -9.8) quadrotor3d.py:47, quadrotor3d_slungload.py:48; (0, -9.8) quadrotor2d.py:46, quadrotor2d_slungload.py:47
    p->g_vec[(kind == RMAV_QUAD2D || kind == RMAV_QUAD2D_SL) ? 1 : 2] = -9.8;
    p->thrust_scale = 1.0;
    p->kp = -5.0;
    p->kv = -4.0;
    p->act_lo = -10.0;
    p->act_hi = 10.0;
    switch (kind) {
    case RMAV_QUAD2D:
        p->pos_limit = 3.0;
        p->vel_limit = (reading_2d == 'A') ? 10.0 : 2.0;
        p->thrust_scale = 10.0;
        p->clamp_thrust = 1;
        p->tau = 0.1;
        break;
    case RMAV_QUAD2D_SL:
        p->tether_length = 0.5;
        p->pos_limit = 2.0;
        p->vel_limit = 10.0;
        p->tau = 0.1;
        break;
    case RMAV_QUAD3D:
        p->pos_limit = 3.0;
        p->vel_limit = 10.0;
        p->ref_pos[2] = 2.0;
        p->tau = 0.3;
        p->act_lo = 0.0;  // quadrotor3d.py:70 Box(low=0, high=10)
        break;
    case RMAV_QUAD3D_SL:
        p->tether_length = 1.5;
        p->pos_limit = 3.0;
        p->vel_limit = 10.0;
        p->ref_pos[2] = 1.0;
        p->tau = 0.3;
        break;
    case RMAV_REINMAV:       // reinmav_env.py:55-73; only mass, g and dt are read from this struct
        p->mass = 0.1800;
        p->load_mass = 0.0;
        p->g = 9.8100;
        p->g_vec[2] = 0.0;   // not read: ReinmavEnv's gravity is the scalar above
        p->dt = 1.0 / 100;
        p->tau = 1.0;        // unused (keeps check_params happy)
        p->act_lo = 0.0;     // RMAV_ACT_RANDOM range for (F, Mx, My, Mz): [0, max_force)
        p->act_hi = 3.5316;
        break;
    }
    return RMAV_OK;
}

int rmav_create(rmav_handle *out, int kind, int64_t n_envs, int device, uint64_t seed,
                uint64_t env_id_base, uint32_t flags, const rmav_params *params, void *hip_stream) {
    if (!out) return rmav_fail(RMAV_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (kind < 0 || kind >= kNumKinds) return rmav_fail(RMAV_ERR_INVALID, "bad kind %d", kind);
    if (n_envs <= 0 || n_envs > ((int64_t)1 << 25))  // 32-bit buffer offsets: one step of the widest array stays below 2^31 bytes (include/rmav.h, rmav_rollout_pitched)
        return rmav_fail(RMAV_ERR_INVALID, "n_envs out of range: %lld", (long long)n_envs);
    if (flags & ~(RMAV_F_AUTO_RESET | RMAV_F_TRACK_EPISODES))
        return rmav_fail(RMAV_ERR_INVALID, "unknown flag bits 0x%x", flags);
    const int ndev = rmav_device_count();
    if (ndev <= 0) return rmav_fail(RMAV_ERR_NO_DEVICE, "no HIP device visible; librmav has no CPU path");
    if (device < 0 || device >= ndev) return rmav_fail(RMAV_ERR_INVALID, "device %d out of range [0,%d)", device, ndev);
    rmav_params pr;
    if (params) pr = *params;
    else rmav_default_params(kind, 0, &pr);
    if (int rc = check_params(pr)) return rc;

    DeviceGuard guard(device);
    if (!guard.ok) return rmav_fail(RMAV_ERR_HIP, "hipSetDevice(%d) failed", device);

    rmav_handle h = new (std::nothrow) rmav_env_s();
    if (!h) return rmav_fail(RMAV_ERR_ALLOC, "host allocation failed");
    memset(h, 0, sizeof(*h));
    h->magic = kMagic;
    h->kind = kind;
    h->n = n_envs;
    h->device = device;
    h->seed = seed;
    h->env_base = env_id_base;
    h->flags = flags;
    h->params = pr;
    for (int i = 0; i < RMAV_TUNE_COUNT; ++i) h->tune[i] = -1;
    h->rule_lo = -__builtin_inff();   // the identity action rule (rmav_set_policy_action_rule)
    h->rule_hi = __builtin_inff();
    h->frame_skip = 1;
    if (adopt_stream(h, hip_stream)) {
        (void)hipGetLastError();
        free_all(h);
        return rmav_fail(RMAV_ERR_HIP, "hipStreamCreate failed");
    }
    const size_t n = (size_t)n_envs;
    const int nS = kStateDim[kind];
    // One arena for every per-env array.  A single-step launch at 65 536 envs is latency-bound and touches ten
    // small arrays (256 KB each); as separate hipMalloc blocks each of them sits in its own small-page mapping and
    // every launch pays their address translations, while one 2 MiB-aligned block is covered by a few large
    // fragments.  Sub-arrays start on 4 KiB boundaries.
    {
        auto up = [](size_t b) { return (b + 4095) & ~(size_t)4095; };
        const bool tr = (flags & RMAV_F_TRACK_EPISODES) != 0;
        size_t off = 0;
        const size_t o_state = off; off += up(n * nS * sizeof(float));
        const size_t o_rec = off; off += up(n * sizeof(EnvRec));
        const size_t o_tot = off; off += up(n_total_slots(n_envs) * sizeof(Totals));
        const size_t o_time = off; off += (kind == RMAV_REINMAV) ? up(n * sizeof(double)) : 0;
        const size_t o_er = off; off += tr ? up(n * sizeof(float)) : 0;
        const size_t o_lr = off; off += tr ? up(n * sizeof(float)) : 0;
        // (the device copy of a tracking reward's spec: here, so that rmav_set_reward never allocates - it may be captured into a graph)
        const size_t o_rw = off; off += (kind != RMAV_REINMAV) ? up(sizeof(RewardArgs)) : 0;
        // (... and of a disturbance's spec, for the same reason)
        const size_t o_ds = off; off += (kind != RMAV_REINMAV) ? up(sizeof(DisturbSpec)) : 0;
        // (... and of a sensor-noise spec)
        const size_t o_sn = off; off += (kind != RMAV_REINMAV) ? up(sizeof(SensorDev)) : 0;
        // (... and of an actuator spec's coefficients)
        const size_t o_al = off; off += (kind != RMAV_REINMAV) ? up(sizeof(ActuatorDev)) : 0;
        // (... and of a start-state spec's)
        const size_t o_ss = off; off += (kind != RMAV_REINMAV) ? up(sizeof(StartDev)) : 0;
        // (... and of a termination spec's)
        const size_t o_tc = off; off += (kind != RMAV_REINMAV) ? up(sizeof(TermDev)) : 0;
        if (hipMalloc(&h->arena, off) != hipSuccess) {
            (void)hipGetLastError();
            h->arena = nullptr;
            free_all(h);
            return rmav_fail(RMAV_ERR_ALLOC, "device allocation of %zu bytes failed for %lld envs", off, (long long)n_envs);
        }
        char *b = (char *)h->arena;
        h->state = (float *)(b + o_state);
        h->rec = (EnvRec *)(b + o_rec);
        h->totals = (Totals *)(b + o_tot);
        if (kind == RMAV_REINMAV) h->env_time = (double *)(b + o_time);
        else h->reward_dev = (RewardArgs *)(b + o_rw), h->disturb_dev = (DisturbSpec *)(b + o_ds), h->sensor_dev = (SensorDev *)(b + o_sn),
                 h->actuator_dev = (ActuatorDev *)(b + o_al), h->start_dev = (StartDev *)(b + o_ss),
                 h->term_dev = (TermDev *)(b + o_tc);
        if (tr) {
            h->ep_ret = (float *)(b + o_er);
            h->last_ret = (float *)(b + o_lr);
        }
    }
    // every record: steps_beyond_done = None (-1), no reset drawn yet, the episode clock starts at 0, no finished episode
    hipLaunchKernelGGL(k_rec_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->rec, EnvRec{-1, 0u, 0u, 0}, -1, (int64_t)n);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemsetAsync(h->totals, 0, n_total_slots(n_envs) * sizeof(Totals), h->stream);
    if (e == hipSuccess && (flags & RMAV_F_TRACK_EPISODES)) {
        e = hipMemsetAsync(h->ep_ret, 0, n * sizeof(float), h->stream);
        if (e == hipSuccess) e = hipMemsetAsync(h->last_ret, 0, n * sizeof(float), h->stream);
    }
    if (e != hipSuccess) {
        free_all(h);
        return rmav_fail(RMAV_ERR_HIP, "hipMemsetAsync failed: %s", hipGetErrorString(e));
    }
    if (kind == RMAV_REINMAV) {
        // ReinmavEnv.__init__ (reinmav_env.py:79-81): state = (0,0,0, 0,0,0, 1,0,0,0, 0,0,0), t = 0; no RNG
        const float one = 1.0f;
        uint32_t one_bits;
        memcpy(&one_bits, &one, 4);
        e = hipMemsetAsync(h->state, 0, n * nS * sizeof(float), h->stream);
        if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)(h->state + 6 * n), (int)one_bits, n, h->stream);
        if (e == hipSuccess) e = hipMemsetAsync(h->env_time, 0, n * sizeof(double), h->stream);
        if (e != hipSuccess) {
            free_all(h);
            return rmav_fail(RMAV_ERR_HIP, "initial state failed: %s", hipGetErrorString(e));
        }
    } else if (int rc = launch_reset(h, nullptr, RMAV_SOA)) {
        // the reference constructors call seed() then reset()  (quadrotor3d.py:73-74)
        free_all(h);
        return rc;
    }
    e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        free_all(h);
        return rmav_fail(RMAV_ERR_HIP, "initial reset failed: %s", hipGetErrorString(e));
    }
    *out = h;
    return RMAV_OK;
}

int rmav_destroy(rmav_handle h) {
    if (!valid(h)) return rmav_fail(RMAV_ERR_INVALID, "invalid rmav_handle");
    if (h->xchg.comm && h->xchg.comm->armed_by == h) h->xchg.comm->armed_by = nullptr;
    DeviceGuard guard(h->device);
    (void)hipStreamSynchronize(h->stream);
    free_all(h);
    return RMAV_OK;
}

// t is also the episode clock (rmav_kernels.hpp: ep_clock0): when a caller moves it, every env's episode start moves along,
// so running episode lengths carry over the jump
static int move_step_counter(rmav_handle h, uint64_t t) {
    const uint32_t delta = (uint32_t)t - (uint32_t)h->t;
    if (delta != 0u && ((h->flags & RMAV_F_TRACK_EPISODES) || h->time_limit > 0)) {
        hipLaunchKernelGGL(k_shift_ep_start, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, h->stream, h->rec, delta, (int64_t)h->n);
        HIP_TRY(hipGetLastError());
    }
    h->t = t;
    return RMAV_OK;
}

int rmav_seed(rmav_handle h, uint64_t seed) {
    CHECK_HANDLE(h);
    h->seed = seed;
    if (int rc = move_step_counter(h, 0)) return rc;
    hipLaunchKernelGGL(k_rec_fill, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, h->stream, h->rec, EnvRec{0, 0u, 0u, 0}, 1, (int64_t)h->n);   // reset_cnt = 0
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

int rmav_get_params(rmav_handle h, rmav_params *out) {
    if (!valid(h)) return rmav_fail(RMAV_ERR_INVALID, "invalid rmav_handle");
    if (!out) return rmav_fail(RMAV_ERR_INVALID, "out is NULL");
    *out = h->params;
    return RMAV_OK;
}

int rmav_set_params(rmav_handle h, const rmav_params *in) {
    if (!valid(h)) return rmav_fail(RMAV_ERR_INVALID, "invalid rmav_handle");
    if (!in) return rmav_fail(RMAV_ERR_INVALID, "in is NULL");
    if (int rc = check_params(*in)) return rc;
    const rmav_params old = h->params;
    h->params = *in;
    if (h->actuator_on && in->dt != old.dt) {   // actuator lag: alpha and beta follow the new dt (the policy kernels' copy, in stream order)
        DeviceGuard guard(h->device);
        if (int rc = rmav_sync_actuator_dev(h)) {
            h->params = old;
            return rc;
        }
    }
    return RMAV_OK;
}

int rmav_set_stream(rmav_handle h, void *hip_stream) {
    CHECK_HANDLE(h);
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->own_stream) (void)hipStreamDestroy(h->stream);
    return adopt_stream(h, hip_stream);
}

int rmav_set_env_param(rmav_handle h, int which, const float *values, int mem) {
    CHECK_HANDLE(h);
    if (int rc = check_mem_layout(mem, RMAV_SOA)) return rc;
    if (which < 0 || which > 2) return rmav_fail(RMAV_ERR_INVALID, "unknown env param %d", which);
    if (h->kind == RMAV_REINMAV) return rmav_fail(RMAV_ERR_INVALID, "per-env constants are for the quadrotor kinds");
    if (!values) {  // back to the shared value (and no range any more)
        if ((h->range_mask >> which) & 1u) {
            h->range_mask &= ~(1u << which);
            if (int rc = sync_range_dev(h)) return rc;
        }
        if (h->pe[which]) {
            HIP_TRY(hipStreamSynchronize(h->stream));
            HIP_TRY(hipFree(h->pe[which]));
            h->pe[which] = nullptr;
        }
        return RMAV_OK;
    }
    if (!h->pe[which] && hipMalloc((void **)&h->pe[which], (size_t)h->n * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        h->pe[which] = nullptr;
        return rmav_fail(RMAV_ERR_ALLOC, "device allocation failed");
    }
    return copy_in(h, h->pe[which], values, (size_t)h->n, mem);
}

int rmav_get_env_param(rmav_handle h, int which, float *out, int mem) {
    CHECK_HANDLE(h);
    if (int rc = check_mem_layout(mem, RMAV_SOA)) return rc;
    if (which < 0 || which > 2) return rmav_fail(RMAV_ERR_INVALID, "unknown env param %d", which);
    if (h->kind == RMAV_REINMAV) return rmav_fail(RMAV_ERR_INVALID, "per-env constants are for the quadrotor kinds");
    if (!out) return rmav_fail(RMAV_ERR_INVALID, "output pointer is NULL");
    if (h->pe[which]) return copy_out(h, (const float *)h->pe[which], out, (size_t)h->n, mem);
    // no array: every env has the shared value, rounded to fp32 as an uploaded array would hold it
    const float v = (float)(which == RMAV_PARAM_MASS ? h->params.mass : which == RMAV_PARAM_LOAD_MASS ? h->params.load_mass : h->params.tether_length);
    if (mem == RMAV_DEVICE) {
        uint32_t bits;
        memcpy(&bits, &v, 4);
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)out, (int)bits, (size_t)h->n, h->stream));
    } else {
        for (int64_t i = 0; i < h->n; ++i) out[i] = v;
    }
    return RMAV_OK;
}

int rmav_set_env_param_range(rmav_handle h, int which, float lo, float hi) {
    CHECK_HANDLE(h);
    if (which < 0 || which > 2) return rmav_fail(RMAV_ERR_INVALID, "unknown env param %d", which);
    if (h->kind == RMAV_REINMAV) return rmav_fail(RMAV_ERR_INVALID, "per-env constants are for the quadrotor kinds");
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo > 0.0f) || !(lo <= hi))
        return rmav_fail(RMAV_ERR_INVALID, "a parameter range needs finite 0 < lo <= hi, got [%g, %g]", (double)lo, (double)hi);
    if (!h->pe[which] && hipMalloc((void **)&h->pe[which], (size_t)h->n * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        h->pe[which] = nullptr;
        return rmav_fail(RMAV_ERR_ALLOC, "device allocation failed");
    }
    h->range_lo[which] = lo;
    h->range_hi[which] = hi;
    h->range_mask |= 1u << which;
    if (int rc = sync_range_dev(h)) return rc;
    return launch_range_draw(h, 1u << which);   // this parameter only: the others keep the values they have
}

int rmav_get_env_param_range(rmav_handle h, int which, float *lo, float *hi, int32_t *enabled) {
    if (!valid(h)) return rmav_fail(RMAV_ERR_INVALID, "invalid rmav_handle");
    if (which < 0 || which > 2) return rmav_fail(RMAV_ERR_INVALID, "unknown env param %d", which);
    const bool on = (h->range_mask >> which) & 1u;
    if (lo) *lo = on ? h->range_lo[which] : 0.0f;
    if (hi) *hi = on ? h->range_hi[which] : 0.0f;
    if (enabled) *enabled = on ? 1 : 0;
    return RMAV_OK;
}

int rmav_set_tuning(rmav_handle h, int key, int value) {
    if (!valid(h)) return rmav_fail(RMAV_ERR_INVALID, "invalid rmav_handle");
    if (key < 0 || key >= RMAV_TUNE_COUNT) return rmav_fail(RMAV_ERR_INVALID, "unknown tuning key %d", key);
    h->tune[key] = value;
    return RMAV_OK;
}
int rmav_get_tuning(rmav_handle h, int key, int *value_out) {
    if (!valid(h)) return rmav_fail(RMAV_ERR_INVALID, "invalid rmav_handle");
    if (key < 0 || key >= RMAV_TUNE_COUNT || !value_out) return rmav_fail(RMAV_ERR_INVALID, "unknown tuning key %d or NULL out", key);
    *value_out = h->tune[key];
    return RMAV_OK;
}

int64_t rmav_num_envs(rmav_handle h) {
    if (!valid(h)) return rmav_fail(RMAV_ERR_INVALID, "invalid rmav_handle");
    return h->n;
}

int rmav_sync(rmav_handle h) {
    CHECK_HANDLE(h);
    HIP_TRY(hipStreamSynchronize(h->stream));
    return RMAV_OK;
}

int rmav_reset(rmav_handle h, float *obs_out, int mem, int layout) {
    CHECK_HANDLE(h);
    if (int rc = check_mem_layout(mem, layout)) return rc;
    if (h->actuator_on)   // actuator lag: every env's m = init, in stream order in front of whatever steps next
        if (int rc = rmav_launch_actuator_fill(h)) return rc;
    return write_via_host(h, obs_out, (size_t)h->n * kStateDim[h->kind] * sizeof(float), mem, [&](void *dst) {
        if (!h->sensor_on || !dst) return launch_reset_tl(h, (float *)dst, layout);
        // a handle with sensor noise: the reset, then the observation of the fresh states at the handle's step counter (k_observe)
        if (int rc = launch_reset_tl(h, nullptr, layout)) return rc;
        return rmav_launch_observe(h, (float *)dst, layout);
    });
}

// rmav_rollout / rmav_step / rmav_step_control / rmav_control_step.  ctrl_out (nullable): control() of the state the
// call leaves behind, nA*N floats in `layout` (action_mode must be RMAV_ACT_BUFFER, n_steps 1).
static int rollout_impl(rmav_handle h, int32_t n_steps, int action_mode, const float *actions_in, float *actions_out,
                        float *obs_out, float *rew_out, uint8_t *done_out, float *ctrl_out, int mem, int layout,
                        int fused, int64_t pitch = 0, bool want_final = false, float *final_out = nullptr, uint8_t *trunc_out = nullptr) {
    // want_final (rmav_step_final: one step, caller actions, a quadrotor handle): the launch is k_step_final; final_out / trunc_out
    // are staged like the other outputs, and final_out - of which the kernel rewrites only the finished envs' elements - is staged IN too
    CHECK_HANDLE(h);
    if (int rc = check_mem_layout(mem, layout)) return rc;
    if (n_steps <= 0) return rmav_fail(RMAV_ERR_INVALID, "n_steps must be > 0");
    // (the bound of num_envs, for the same reason: the kernels add the in-step column offset c * 4 * pitch, c < nS <= 16, in 32 bits -
    // one step of the widest array stays below 2^31 bytes)
    if (pitch != 0 && (pitch < h->n || pitch > ((int64_t)1 << 25) || mem != RMAV_DEVICE || layout != RMAV_SOA))
        return rmav_fail(RMAV_ERR_INVALID, "a column pitch must be in [num_envs, 2^25 = 33554432] and needs device pointers and the feature-major layout");
    if (action_mode < RMAV_ACT_BUFFER || action_mode > RMAV_ACT_CONTROLLER)
        return rmav_fail(RMAV_ERR_INVALID, "unknown action_mode %d", action_mode);
    if (action_mode == RMAV_ACT_BUFFER && !actions_in)
        return rmav_fail(RMAV_ERR_INVALID, "RMAV_ACT_BUFFER needs actions_in");
    if (ctrl_out && h->kind == RMAV_REINMAV)
        return rmav_fail(RMAV_ERR_INVALID, "ReinmavEnv's controller runs inside its step (the controller action mode); there is no separate control()");
    if (ctrl_out && h->frame_skip > 1)
        return rmav_fail(RMAV_ERR_INVALID, "rmav_step_control has no frame-skip kernel: call rmav_control and rmav_step on a handle with a frame skip");
    const size_t n = pitch ? (size_t)pitch : (size_t)h->n, T = (size_t)n_steps;   // (the trajectory arrays' column pitch)
    const size_t nS = kStateDim[h->kind], nA = kActionDim[h->kind];
    const size_t b_act = T * nA * n * sizeof(float), b_obs = T * nS * n * sizeof(float);
    const size_t b_rew = T * n * sizeof(float), b_done = T * n, b_ctrl = nA * n * sizeof(float);
    const size_t b_fin = nS * n * sizeof(float), b_trunc = n;
    const bool want_aout = actions_out && action_mode != RMAV_ACT_BUFFER;

    // The arrays of the call: what the kernels get (dev: the caller's pointers with RMAV_DEVICE) and, with RMAV_HOST, how each array that
    // is present is staged - its place in the staging block, copied in before the launches and / or out behind them.
    enum { S_ACT_IN, S_ACT_OUT, S_OBS, S_REW, S_DONE, S_CTRL, S_FINAL, S_TRUNC, S_COUNT };
    struct Staged {
        void *host;   // nullptr: not staged
        size_t bytes;
        bool in, out;
        size_t off;
    } stg[S_COUNT] = {{action_mode == RMAV_ACT_BUFFER ? const_cast<float *>(actions_in) : nullptr, b_act, true, false, 0},
                      {want_aout ? actions_out : nullptr, b_act, false, true, 0},
                      {obs_out, b_obs, false, true, 0},
                      {rew_out, b_rew, false, true, 0},
                      {done_out, b_done, false, true, 0},
                      {ctrl_out, b_ctrl, false, true, 0},
                      {final_out, b_fin, true, true, 0},
                      {trunc_out, b_trunc, false, true, 0}};
    void *dev[S_COUNT] = {const_cast<float *>(actions_in), actions_out, obs_out, rew_out, done_out, ctrl_out, final_out, trunc_out};
    bool pinned = false;
    char *hbase = nullptr;   // host view of the staging block (pinned path only)
    if (mem == RMAV_HOST) {
        size_t off = 0;
        for (Staged &g : stg)
            if (g.host) {
                g.off = off;
                off += (g.bytes + 255) & ~(size_t)255;
            }
        if (!off) off = 256;
        char *base;
        if (off <= kPinnedMax && ensure_pinned(h, off) == RMAV_OK) {
            // zero-copy: the kernel reads / writes the pinned host block directly
            pinned = true;
            hbase = (char *)h->pinned;
            base = (char *)h->pinned_dev;
            for (const Staged &g : stg)
                if (g.host && g.in) memcpy(hbase + g.off, g.host, g.bytes);
        } else {   // bulk: stage through device scratch
            if (int rc = ensure_scratch(h, off)) return rc;
            base = (char *)h->scratch;
            for (const Staged &g : stg)
                if (g.host && g.in) HIP_TRY(hipMemcpyAsync(base + g.off, g.host, g.bytes, hipMemcpyHostToDevice, h->stream));
        }
        for (int i = 0; i < S_COUNT; ++i) dev[i] = stg[i].host ? base + stg[i].off : nullptr;
    }
    const float *const d_act_in = (const float *)dev[S_ACT_IN];
    float *const d_act_out = (float *)dev[S_ACT_OUT], *const d_obs = (float *)dev[S_OBS], *const d_rew = (float *)dev[S_REW];
    uint8_t *const d_done = (uint8_t *)dev[S_DONE];
    float *const d_ctrl = (float *)dev[S_CTRL];

    RolloutArgs a = base_args(h);
    if (layout == RMAV_AOS) a.flags |= F_AOS;
    if (pitch) a.pitch = pitch;
    a.ctrl_out = d_ctrl;
    const int kmode = d_ctrl ? (int)ACT_BUFFER_CTRL : action_mode;
    // One wavefront, one k_step launch, outputs in the pinned block: the kernel publishes its completion in a pinned word and
    // the host spins on that (bounded) instead of hipStreamSynchronize.  What the gym-shaped single env runs.
    bool flag_wait = false;
    // (not rmav_step_control of a handle from the tracking-reward rung up: k_control runs behind its k_step_*, which would publish too early)
    if (pinned && n_steps == 1 && h->n <= 64 && action_mode == RMAV_ACT_BUFFER && h->kind != RMAV_REINMAV && !(d_ctrl && kLadder[rung_of(h)].control_behind)) {
        if (!h->done_flag && hipHostMalloc((void **)&h->done_flag, 64, hipHostMallocMapped) == hipSuccess) {
            *h->done_flag = 0;
            if (hipHostGetDevicePointer((void **)&h->done_flag_dev, h->done_flag, 0) != hipSuccess) {
                (void)hipHostFree(h->done_flag);
                h->done_flag = nullptr;
            }
        }
        (void)hipGetLastError();
        if (h->done_flag) {
            a.done_flag = h->done_flag_dev;
            a.done_seq = ++h->done_seq;
            flag_wait = true;
        }
    }
    h->xchg.allow = fused != 0;   // one fused launch may carry an armed exchange's snapshot; the fused = 0 loop may not
    if (fused) {
        a.n_steps = n_steps;
        a.act_in = d_act_in;
        a.act_out = d_act_out;
        a.obs_out = d_obs;
        a.rew_out = d_rew;
        a.done_out = d_done;
        if (want_final) {
            if (int rc = launch_step_final(h, a, FinalArgs{(float *)dev[S_FINAL], (uint8_t *)dev[S_TRUNC]})) return rc;
        } else if (int rc = launch_rollout(h, kmode, a)) return rc;
    } else {
        for (size_t k = 0; k < T; ++k) {
            a.n_steps = 1;
            a.t0 = h->t + k;
            a.act_in = d_act_in ? d_act_in + k * nA * n : nullptr;
            a.act_out = d_act_out ? d_act_out + k * nA * n : nullptr;
            a.obs_out = d_obs ? d_obs + k * nS * n : nullptr;
            a.rew_out = d_rew ? d_rew + k * n : nullptr;
            a.done_out = d_done ? d_done + k * n : nullptr;
            if (int rc = launch_rollout(h, (k + 1 == T) ? kmode : action_mode, a)) return rc;
        }
    }
    h->t += T;

    if (mem == RMAV_HOST) {
        if (pinned) {
            bool seen = false;
            if (flag_wait) {   // ~10 us is the whole launch; 2 ms covers a cold first launch, then fall back to the stream
                timespec t0, t1;
                clock_gettime(CLOCK_MONOTONIC, &t0);
                const volatile uint32_t *f = h->done_flag;
                for (uint32_t spin = 0;; ++spin) {
                    if (*f == h->done_seq) { seen = true; break; }
                    if ((spin & 255u) == 255u) {
                        clock_gettime(CLOCK_MONOTONIC, &t1);
                        if ((t1.tv_sec - t0.tv_sec) * 1000000000ll + (t1.tv_nsec - t0.tv_nsec) > 2000000ll) break;
                    }
                }
                __atomic_thread_fence(__ATOMIC_ACQUIRE);
            }
            if (!seen) HIP_TRY(hipStreamSynchronize(h->stream));
            for (const Staged &g : stg)
                if (g.host && g.out) memcpy(g.host, hbase + g.off, g.bytes);
        } else {
            for (int i = 0; i < S_COUNT; ++i)
                if (stg[i].host && stg[i].out) HIP_TRY(hipMemcpyAsync(stg[i].host, dev[i], stg[i].bytes, hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
        }
        if (actions_out && action_mode == RMAV_ACT_BUFFER && actions_out != actions_in)
            memcpy(actions_out, actions_in, b_act);
    } else if (actions_out && action_mode == RMAV_ACT_BUFFER && actions_out != actions_in) {
        HIP_TRY(hipMemcpyAsync(actions_out, actions_in, b_act, hipMemcpyDeviceToDevice, h->stream));
    }
    return RMAV_OK;
}

int rmav_step(rmav_handle h, const float *actions, float *obs_out, float *rew_out,
              uint8_t *done_out, int mem, int layout) {
    if (!actions) return rmav_fail(RMAV_ERR_INVALID, "actions is NULL");
    return rmav_rollout(h, 1, RMAV_ACT_BUFFER, actions, nullptr, obs_out, rew_out, done_out, mem,
                        layout, 1);
}

int rmav_control(rmav_handle h, float *actions_out, int mem, int layout) {
    CHECK_HANDLE(h);
    if (int rc = check_mem_layout(mem, layout)) return rc;
    if (!actions_out) return rmav_fail(RMAV_ERR_INVALID, "actions_out is NULL");
    return write_via_host(h, actions_out, (size_t)h->n * kActionDim[h->kind] * sizeof(float), mem,
                          [&](void *dst) { return launch_control(h, (float *)dst, layout); });
}

int rmav_control_step(rmav_handle h, float *actions_out, float *obs_out, float *rew_out, uint8_t *done_out, int mem,
                      int layout) {
    return rollout_impl(h, 1, RMAV_ACT_CONTROLLER, nullptr, actions_out, obs_out, rew_out, done_out, nullptr, mem,
                        layout, 1);
}

int rmav_step_control(rmav_handle h, const float *actions, float *obs_out, float *rew_out, uint8_t *done_out,
                      float *next_actions_out, int mem, int layout) {
    if (!actions) return rmav_fail(RMAV_ERR_INVALID, "actions is NULL");
    if (!next_actions_out) return rmav_fail(RMAV_ERR_INVALID, "next_actions_out is NULL");
    return rollout_impl(h, 1, RMAV_ACT_BUFFER, actions, nullptr, obs_out, rew_out, done_out, next_actions_out, mem,
                        layout, 1);
}

int rmav_rollout(rmav_handle h, int32_t n_steps, int action_mode, const float *actions_in,
                 float *actions_out, float *obs_out, float *rew_out, uint8_t *done_out, int mem,
                 int layout, int fused) {
    return rollout_impl(h, n_steps, action_mode, actions_in, actions_out, obs_out, rew_out, done_out, nullptr, mem,
                        layout, fused);
}

int64_t rmav_trajectory_pitch(rmav_handle h) {
    if (!valid(h)) return rmav_fail(RMAV_ERR_INVALID, "invalid handle");
    return (h->n + 63) & ~(int64_t)63;
}

int rmav_rollout_pitched(rmav_handle h, int32_t n_steps, int action_mode, const float *actions_in, float *actions_out,
                         float *obs_out, float *rew_out, uint8_t *done_out, int64_t pitch, int fused) {
    if (pitch <= 0) return rmav_fail(RMAV_ERR_INVALID, "pitch must be > 0 (rmav_trajectory_pitch)");
    return rollout_impl(h, n_steps, action_mode, actions_in, actions_out, obs_out, rew_out, done_out, nullptr, RMAV_DEVICE,
                        RMAV_SOA, fused, pitch);
}

// Chunk-major trajectories: see include/rmav.h.  The recommended chunk is the batch the two-wavefront kernel runs best at for the
// kind whose launches are bound by the trajectory stores (65 536 envs = one (integrator, memory) pair per SIMD): profiles/r05/chunk_probe.md.
int64_t rmav_chunk_envs(rmav_handle h) {
    if (!valid(h)) return rmav_fail(RMAV_ERR_INVALID, "invalid handle");
    // measured: quadrotor3d with random / caller actions gains 5 - 9 % at 131 072 - 262 144 envs; every other kind loses 3 - 10 %
    // no chunking: ONE chunk whose width is N rounded up to the 64-env granule every chunk width must have (rmav_rollout_chunked
    // turns a chunk wider than N into the column pitch of the plain layout)
    return (h->kind == RMAV_QUAD3D && h->n > 65536) ? 65536 : ((h->n + 63) & ~(int64_t)63);
}

int rmav_rollout_chunked(rmav_handle h, int32_t n_steps, int action_mode, const float *actions_in, float *actions_out,
                         float *obs_out, float *rew_out, uint8_t *done_out, int64_t chunk_envs) {
    CHECK_HANDLE(h);
    if (chunk_envs <= 0 || (chunk_envs & 63)) return rmav_fail(RMAV_ERR_INVALID, "chunk_envs must be a positive multiple of 64 (rmav_chunk_envs)");
    if (chunk_envs >= h->n)   // one chunk: the plain feature-major layout
        return rollout_impl(h, n_steps, action_mode, actions_in, actions_out, obs_out, rew_out, done_out, nullptr, RMAV_DEVICE, RMAV_SOA, 1,
                            chunk_envs > h->n ? chunk_envs : 0);
    if (h->kind > RMAV_QUAD3D_SL) return rmav_fail(RMAV_ERR_INVALID, "chunk-major rollouts are for the quadrotor kinds");
    const int64_t cap = kEnvsPerCuSlot * split_pairs_of(action_mode)[h->kind];
    if (n_steps < 2 || chunk_envs > cap)
        return rmav_fail(RMAV_ERR_INVALID, "chunk-major rollouts need n_steps >= 2 and chunk_envs <= %lld for this kind and action source", (long long)cap);
    if (actions_out && action_mode == RMAV_ACT_BUFFER)   // (rollout_impl's echo copy is sized for the plain layout)
        return rmav_fail(RMAV_ERR_INVALID, "chunk-major rollouts do not echo caller actions: pass actions_out = NULL with RMAV_ACT_BUFFER");
    h->chunk = chunk_envs;
    const int rc = rollout_impl(h, n_steps, action_mode, actions_in, actions_out, obs_out, rew_out, done_out, nullptr, RMAV_DEVICE, RMAV_SOA, 1);
    h->chunk = 0;
    return rc;
}

int rmav_get_state(rmav_handle h, float *out, int mem, int layout) {
    CHECK_HANDLE(h);
    if (int rc = check_mem_layout(mem, layout)) return rc;
    if (!out) return rmav_fail(RMAV_ERR_INVALID, "out is NULL");
    const int nS = kStateDim[h->kind];
    const size_t cnt = (size_t)h->n * nS;
    if (layout == RMAV_SOA) return copy_out(h, (const float *)h->state, out, cnt, mem);
    if (mem == RMAV_DEVICE) {
        hipLaunchKernelGGL(k_soa_to_aos, grid_for(h), dim3(block_size(h)), 0, h->stream, h->state, out, h->n, nS);
        HIP_TRY(hipGetLastError());
        return RMAV_OK;
    }
    if (int rc = ensure_scratch(h, cnt * sizeof(float))) return rc;
    hipLaunchKernelGGL(k_soa_to_aos, grid_for(h), dim3(block_size(h)), 0, h->stream, h->state,
                       (float *)h->scratch, h->n, nS);
    HIP_TRY(hipGetLastError());
    return copy_out(h, (const float *)h->scratch, out, cnt, RMAV_HOST);
}

int rmav_set_state(rmav_handle h, const float *in, int mem, int layout) {
    CHECK_HANDLE(h);
    if (int rc = check_mem_layout(mem, layout)) return rc;
    if (!in) return rmav_fail(RMAV_ERR_INVALID, "in is NULL");
    const int nS = kStateDim[h->kind];
    const size_t cnt = (size_t)h->n * nS;
    if (layout == RMAV_SOA) return copy_in(h, h->state, in, cnt, mem);
    const float *src = in;
    if (mem == RMAV_HOST) {
        if (int rc = ensure_scratch(h, cnt * sizeof(float))) return rc;
        HIP_TRY(hipMemcpyAsync(h->scratch, in, cnt * sizeof(float), hipMemcpyHostToDevice, h->stream));
        src = (const float *)h->scratch;
    }
    hipLaunchKernelGGL(k_aos_to_soa, grid_for(h), dim3(block_size(h)), 0, h->stream, src, h->state, h->n, nS);
    HIP_TRY(hipGetLastError());
    if (mem == RMAV_HOST) HIP_TRY(hipStreamSynchronize(h->stream));
    return RMAV_OK;
}

int rmav_get_sbd(rmav_handle h, int32_t *out, int mem) {
    CHECK_HANDLE(h);
    if (int rc = check_mem_layout(mem, RMAV_SOA)) return rc;
    return rec_field_get(h, 0, reinterpret_cast<uint32_t *>(out), mem);
}
int rmav_set_sbd(rmav_handle h, const int32_t *in, int mem) {
    CHECK_HANDLE(h);
    if (int rc = check_mem_layout(mem, RMAV_SOA)) return rc;
    return rec_field_set(h, 0, reinterpret_cast<const uint32_t *>(in), mem);
}
int rmav_get_reset_counts(rmav_handle h, uint32_t *out, int mem) {
    CHECK_HANDLE(h);
    if (int rc = check_mem_layout(mem, RMAV_SOA)) return rc;
    return rec_field_get(h, 1, out, mem);
}
int rmav_set_reset_counts(rmav_handle h, const uint32_t *in, int mem) {
    CHECK_HANDLE(h);
    if (int rc = check_mem_layout(mem, RMAV_SOA)) return rc;
    return rec_field_set(h, 1, in, mem);
}

int rmav_get_time(rmav_handle h, double *out, int mem) {
    CHECK_HANDLE(h);
    if (int rc = check_mem_layout(mem, RMAV_SOA)) return rc;
    if (!h->env_time) return rmav_fail(RMAV_ERR_INVALID, "only reinmav envs carry their own clock");
    return copy_out(h, (const double *)h->env_time, out, (size_t)h->n, mem);
}
int rmav_set_time(rmav_handle h, const double *in, int mem) {
    CHECK_HANDLE(h);
    if (int rc = check_mem_layout(mem, RMAV_SOA)) return rc;
    if (!h->env_time) return rmav_fail(RMAV_ERR_INVALID, "only reinmav envs carry their own clock");
    return copy_in(h, h->env_time, in, (size_t)h->n, mem);
}

int rmav_get_step_count(rmav_handle h, uint64_t *out) {
    if (!valid(h)) return rmav_fail(RMAV_ERR_INVALID, "invalid rmav_handle");
    if (!out) return rmav_fail(RMAV_ERR_INVALID, "out is NULL");
    *out = h->t;
    return RMAV_OK;
}
int rmav_set_step_count(rmav_handle h, uint64_t t) {
    CHECK_HANDLE(h);
    return move_step_counter(h, t);
}

int rmav_episode_totals(rmav_handle h, rmav_ep_totals *out, int clear) {
    CHECK_HANDLE(h);
    if (!out) return rmav_fail(RMAV_ERR_INVALID, "out is NULL");
    if (!(h->flags & RMAV_F_TRACK_EPISODES))
        return rmav_fail(RMAV_ERR_INVALID, "handle was created without RMAV_F_TRACK_EPISODES");
    const size_t nw = n_total_slots(h->n);
    Totals *host = new (std::nothrow) Totals[nw];
    if (!host) return rmav_fail(RMAV_ERR_ALLOC, "host allocation failed");
    hipError_t e = hipMemcpyAsync(host, h->totals, nw * sizeof(Totals), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        delete[] host;
        return rmav_fail(RMAV_ERR_HIP, "reading episode totals failed: %s", hipGetErrorString(e));
    }
    out->episodes = 0;
    out->return_sum = 0.0;
    out->length_sum = 0;
    for (size_t i = 0; i < nw; ++i) {
        out->episodes += host[i].episodes;
        out->return_sum += host[i].return_sum;
        out->length_sum += host[i].length_sum;
    }
    delete[] host;
    if (clear) HIP_TRY(hipMemsetAsync(h->totals, 0, nw * sizeof(Totals), h->stream));
    return RMAV_OK;
}

int rmav_episode_buffers(rmav_handle h, float *last_return, int32_t *last_length, float *cur_return,
                         int32_t *cur_length, int mem) {
    CHECK_HANDLE(h);
    if (int rc = check_mem_layout(mem, RMAV_SOA)) return rc;
    if (!(h->flags & RMAV_F_TRACK_EPISODES))
        return rmav_fail(RMAV_ERR_INVALID, "handle was created without RMAV_F_TRACK_EPISODES");
    const size_t n = (size_t)h->n;
    const hipMemcpyKind kind = (mem == RMAV_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (last_return) HIP_TRY(hipMemcpyAsync(last_return, h->last_ret, n * sizeof(float), kind, h->stream));
    if (cur_return) HIP_TRY(hipMemcpyAsync(cur_return, h->ep_ret, n * sizeof(float), kind, h->stream));
    // lengths live in the per-env records (EnvRec): last_len as it is, the running length = episode clock - the episode's start
    if (last_length)
        if (int rc = rec_field_get(h, 3, reinterpret_cast<uint32_t *>(last_length), mem)) return rc;
    if (cur_length) {
        const uint32_t clock = (uint32_t)h->t;
        int32_t *dst = cur_length;
        if (mem != RMAV_DEVICE) {
            if (int rc = ensure_scratch(h, n * sizeof(int32_t))) return rc;
            dst = (int32_t *)h->scratch;
        }
        hipLaunchKernelGGL(k_cur_length, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, dst, (const EnvRec *)h->rec, clock, (int64_t)n);
        HIP_TRY(hipGetLastError());
        if (mem != RMAV_DEVICE)
            if (int rc = copy_out(h, (const int32_t *)dst, cur_length, n, RMAV_HOST)) return rc;
    }
    if (mem == RMAV_HOST) HIP_TRY(hipStreamSynchronize(h->stream));
    return RMAV_OK;
}

// Frame skip: handle state, host only.  Every stepping launch reads it (launch_rollout_kms, launch_step_k, launch_step_final_k;
// rmav_policy_abi.hip) and passes it to its kernel as an argument.
int rmav_set_frame_skip(rmav_handle h, int32_t k) {
    if (!valid(h)) return rmav_fail(RMAV_ERR_INVALID, "invalid rmav_handle");
    if (k < 1 || k > 1024) return rmav_fail(RMAV_ERR_INVALID, "the frame skip must be in [1, 1024] (1 = none), got %d", (int)k);
    if (h->kind == RMAV_REINMAV && k > 1)
        return rmav_fail(RMAV_ERR_INVALID, "ReinmavEnv sub-steps inside its own step: it takes no frame skip");
    h->frame_skip = k;
    return RMAV_OK;
}

int rmav_get_frame_skip(rmav_handle h, int32_t *out) {
    if (!valid(h)) return rmav_fail(RMAV_ERR_INVALID, "invalid rmav_handle");
    if (!out) return rmav_fail(RMAV_ERR_INVALID, "out is NULL");
    *out = h->frame_skip;
    return RMAV_OK;
}

// Tracking reward: the spec on the handle (what the step and one-wavefront rollout launches pass by value) and its device copy (what the
// policy rollouts read by pointer), rewritten on the handle's stream.  Every stepping launch reads reward_on (launch_rollout_kms,
// launch_step_k, launch_step_final_k; rmav_policy_abi.hip).
int rmav_set_reward(rmav_handle h, const rmav_reward_spec *spec) {
    CHECK_HANDLE(h);
    if (!spec) {   // back to the reference's reward: the launches of a handle that never had a spec
        h->reward_on = 0;
        return RMAV_OK;
    }
    if (h->kind == RMAV_REINMAV) return rmav_fail(RMAV_ERR_INVALID, "ReinmavEnv's reward is its own (100 - 10 every step): it takes no tracking reward");
    const float *v = &spec->goal[0];
    static_assert(sizeof(rmav_reward_spec) == 12 * sizeof(float), "twelve floats");
    for (int i = 0; i < 12; ++i)
        if (!(v[i] - v[i] == 0.0f)) return rmav_fail(RMAV_ERR_INVALID, "every value of a reward spec must be finite (value %d is not)", i);
    const rmav_reward_spec old = h->reward;
    h->reward = *spec;
    if (int rc = rmav_sync_reward_dev(h)) {
        h->reward = old;
        return rc;
    }
    h->reward_on = 1;
    return RMAV_OK;
}

int rmav_get_reward(rmav_handle h, rmav_reward_spec *out, int32_t *enabled) {
    if (!valid(h)) return rmav_fail(RMAV_ERR_INVALID, "invalid rmav_handle");
    if (out) *out = h->reward;   // (the last spec set - zeros before the first - also while it is switched off)
    if (enabled) *enabled = h->reward_on;
    return RMAV_OK;
}

// Wind / gust disturbance: the spec on the handle, passed by value by every stepping launch (launch_rollout_kms, launch_step_k,
// launch_step_final_k read disturb_on) and, for the policy kernels (rmav_policy_abi.hip), copied to the handle's arena by one small launch in
// stream order.  No allocation, no synchronisation: ordering and capture as rmav_set_reward.
int rmav_set_disturbance(rmav_handle h, const rmav_disturbance_spec *spec) {
    CHECK_HANDLE(h);
    if (!spec) {   // none: the launches of a handle that never had a spec
        h->disturb_on = 0;
        return RMAV_OK;
    }
    if (h->kind == RMAV_REINMAV) return rmav_fail(RMAV_ERR_INVALID, "ReinmavEnv integrates its own rigid body: it takes no disturbance");
    for (int i = 0; i < 3; ++i) {
        const float lo = spec->wind_lo[i], hi = spec->wind_hi[i], g = spec->gust[i];
        if (!(lo - lo == 0.0f) || !(hi - hi == 0.0f) || !(g - g == 0.0f))
            return rmav_fail(RMAV_ERR_INVALID, "every value of a disturbance spec must be finite (axis %d is not)", i);
        if (!(lo <= hi)) return rmav_fail(RMAV_ERR_INVALID, "wind_lo[%d] = %g exceeds wind_hi[%d] = %g", i, (double)lo, i, (double)hi);
        if (!(hi - lo - (hi - lo) == 0.0f)) return rmav_fail(RMAV_ERR_INVALID, "wind_hi[%d] - wind_lo[%d] overflows", i, i);
        if (!(g >= 0.0f)) return rmav_fail(RMAV_ERR_INVALID, "gust[%d] = %g is negative", i, (double)g);
        if (!(g + g - (g + g) == 0.0f)) return rmav_fail(RMAV_ERR_INVALID, "2 * gust[%d] overflows", i);
    }
    if (spec->gust_hold < 1 || spec->gust_hold > 1048576)
        return rmav_fail(RMAV_ERR_INVALID, "gust_hold = %d is outside [1, 1048576]", (int)spec->gust_hold);
    const rmav_disturbance_spec old = h->disturb;
    h->disturb = *spec;
    if (int rc = rmav_sync_disturb_dev(h)) {   // the policy kernels' copy, in stream order
        h->disturb = old;
        return rc;
    }
    h->disturb_on = 1;
    return RMAV_OK;
}

int rmav_get_disturbance(rmav_handle h, rmav_disturbance_spec *out, int32_t *enabled) {
    if (!valid(h)) return rmav_fail(RMAV_ERR_INVALID, "invalid rmav_handle");
    if (out) *out = h->disturb;   // (the last spec set - zeros before the first - also while it is switched off)
    if (enabled) *enabled = h->disturb_on;
    return RMAV_OK;
}

int rmav_disturbance_now(rmav_handle h, float *out, int mem) {
    CHECK_HANDLE(h);
    if (mem != RMAV_HOST && mem != RMAV_DEVICE) return rmav_fail(RMAV_ERR_INVALID, "bad mem %d", mem);
    if (!out) return rmav_fail(RMAV_ERR_INVALID, "out is NULL");
    if (!h->disturb_on) return rmav_fail(RMAV_ERR_INVALID, "the handle has no disturbance (rmav_set_disturbance)");
    return write_via_host(h, out, (size_t)3 * (size_t)h->n * sizeof(float), mem, [&](void *dst) { return rmav_launch_disturbance_now(h, (float *)dst); });
}

// Sensor noise: the spec on the handle, passed by value by every launch that emits an observation (launch_rollout_kms, launch_step_k,
// launch_step_final_k and rmav_reset read sensor_on) and, for the policy kernel (rmav_sensor_policy_abi.hip), copied to the handle's arena by
// one small launch in stream order.  No allocation, no synchronisation: ordering and capture as rmav_set_disturbance.
int rmav_set_sensor_noise(rmav_handle h, const rmav_sensor_noise_spec *spec) {
    CHECK_HANDLE(h);
    if (!spec) {   // none: the launches of a handle that never had a spec
        h->sensor_on = 0;
        return RMAV_OK;
    }
    if (h->kind == RMAV_REINMAV) return rmav_fail(RMAV_ERR_INVALID, "ReinmavEnv takes no sensor noise");
    const int nS = kStateDim[h->kind];
    for (int c = 0; c < 16; ++c) {
        const float g = spec->sigma[c];
        if (!(g - g == 0.0f)) return rmav_fail(RMAV_ERR_INVALID, "every sigma of a sensor-noise spec must be finite (component %d is not)", c);
        if (!(g >= 0.0f)) return rmav_fail(RMAV_ERR_INVALID, "sigma[%d] = %g is negative", c, (double)g);
        if (c >= nS && g != 0.0f) return rmav_fail(RMAV_ERR_INVALID, "sigma[%d] = %g: the kind has %d observation components, the others must be 0", c, (double)g, nS);
    }
    const rmav_sensor_noise_spec old = h->sensor;
    h->sensor = *spec;
    if (int rc = rmav_sync_sensor_dev(h)) {   // the policy kernels' copy, in stream order
        h->sensor = old;
        return rc;
    }
    h->sensor_on = 1;
    return RMAV_OK;
}

int rmav_get_sensor_noise(rmav_handle h, rmav_sensor_noise_spec *out, int32_t *enabled) {
    if (!valid(h)) return rmav_fail(RMAV_ERR_INVALID, "invalid rmav_handle");
    if (out) *out = h->sensor;   // (the last spec set - zeros before the first - also while it is switched off)
    if (enabled) *enabled = h->sensor_on;
    return RMAV_OK;
}

int rmav_observe(rmav_handle h, float *obs_out, int mem, int layout) {
    CHECK_HANDLE(h);
    if (int rc = check_mem_layout(mem, layout)) return rc;
    if (!obs_out) return rmav_fail(RMAV_ERR_INVALID, "obs_out is NULL");
    if (!h->sensor_on) return rmav_get_state(h, obs_out, mem, layout);   // no spec: the state itself
    return write_via_host(h, obs_out, (size_t)h->n * kStateDim[h->kind] * sizeof(float), mem,
                          [&](void *dst) { return rmav_launch_observe(h, (float *)dst, layout); });
}

// Actuator lag: the spec on the handle and the per-env filter state m [nA][N] behind it.  Every stepping launch reads actuator_on
// (launch_rollout_kms, launch_step_k, launch_step_final_k; rmav_ppo_abi.hip) and derives alpha / beta from the spec and params.dt when it is
// enqueued; the policy kernels read the device copy in the arena, which every set rewrites in stream order with one small launch.  The FIRST set
// on a handle allocates m; every set that switches the feature on fills it with init in stream order; a set on a handle whose spec is in
// force keeps the running m.  Later sets neither allocate nor synchronise.
int rmav_set_actuator(rmav_handle h, const rmav_actuator_spec *spec) {
    CHECK_HANDLE(h);
    if (!spec) {   // none: the launches of a handle that never had a spec (m stays allocated, unread)
        h->actuator_on = 0;
        return RMAV_OK;
    }
    if (h->kind == RMAV_REINMAV) return rmav_fail(RMAV_ERR_INVALID, "ReinmavEnv takes no actuator lag");
    const int nA = kActionDim[h->kind];
    for (int c = 0; c < 4; ++c) {
        const float tau = spec->tau[c], m0 = spec->init[c];
        if (!(tau - tau == 0.0f)) return rmav_fail(RMAV_ERR_INVALID, "every tau of an actuator spec must be finite (component %d is not)", c);
        if (!(tau >= 0.0f)) return rmav_fail(RMAV_ERR_INVALID, "actuator tau[%d] = %g is negative", c, (double)tau);
        if (!(m0 - m0 == 0.0f)) return rmav_fail(RMAV_ERR_INVALID, "every init of an actuator spec must be finite (component %d is not)", c);
        if (c >= nA && (tau != 0.0f || m0 != 0.0f))
            return rmav_fail(RMAV_ERR_INVALID, "actuator tau[%d] = %g, init[%d] = %g: the kind has %d action components, the others must be 0", c, (double)tau, c,
                             (double)m0, nA);
    }
    if (!h->actuator_m) {
        const hipError_t e = hipMalloc((void **)&h->actuator_m, (size_t)nA * (size_t)h->n * sizeof(float));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            h->actuator_m = nullptr;
            return rmav_fail(RMAV_ERR_HIP, "the actuator state of %lld envs: %s", (long long)h->n, hipGetErrorString(e));
        }
    }
    const rmav_actuator_spec old = h->actuator;
    h->actuator = *spec;
    int rc = rmav_sync_actuator_dev(h);   // the policy kernels' copy, in stream order
    if (!rc && !h->actuator_on) rc = rmav_launch_actuator_fill(h);   // switched on: m = init for every env
    if (rc) {
        h->actuator = old;
        if (h->actuator_on) (void)rmav_sync_actuator_dev(h);
        return rc;
    }
    h->actuator_on = 1;
    return RMAV_OK;
}

int rmav_get_actuator(rmav_handle h, rmav_actuator_spec *out, int32_t *enabled) {
    if (!valid(h)) return rmav_fail(RMAV_ERR_INVALID, "invalid rmav_handle");
    if (out) *out = h->actuator;   // (the last spec set - zeros before the first - also while it is switched off)
    if (enabled) *enabled = h->actuator_on;
    return RMAV_OK;
}

// m as rmav_get_state / rmav_set_state move the state: [nA][N] feature-major as it is stored, or batch-major through the layout kernels
int rmav_get_actuator_state(rmav_handle h, float *out, int mem, int layout) {
    CHECK_HANDLE(h);
    if (int rc = check_mem_layout(mem, layout)) return rc;
    if (!out) return rmav_fail(RMAV_ERR_INVALID, "out is NULL");
    if (!h->actuator_on) return rmav_fail(RMAV_ERR_INVALID, "the handle has no actuator spec (rmav_set_actuator): there is no actuator state");
    const int nA = kActionDim[h->kind];
    const size_t cnt = (size_t)h->n * nA;
    if (layout == RMAV_SOA) return copy_out(h, (const float *)h->actuator_m, out, cnt, mem);
    float *dst = out;
    if (mem != RMAV_DEVICE) {
        if (int rc = ensure_scratch(h, cnt * sizeof(float))) return rc;
        dst = (float *)h->scratch;
    }
    hipLaunchKernelGGL(k_soa_to_aos, grid_for(h), dim3(block_size(h)), 0, h->stream, h->actuator_m, dst, h->n, nA);
    HIP_TRY(hipGetLastError());
    return mem == RMAV_DEVICE ? (int)RMAV_OK : copy_out(h, (const float *)dst, out, cnt, RMAV_HOST);
}

int rmav_set_actuator_state(rmav_handle h, const float *in, int mem, int layout) {
    CHECK_HANDLE(h);
    if (int rc = check_mem_layout(mem, layout)) return rc;
    if (!in) return rmav_fail(RMAV_ERR_INVALID, "in is NULL");
    if (!h->actuator_on) return rmav_fail(RMAV_ERR_INVALID, "the handle has no actuator spec (rmav_set_actuator): there is no actuator state to set");
    const int nA = kActionDim[h->kind];
    const size_t cnt = (size_t)h->n * nA;
    if (layout == RMAV_SOA) return copy_in(h, h->actuator_m, in, cnt, mem);
    const float *src = in;
    if (mem == RMAV_HOST) {
        if (int rc = ensure_scratch(h, cnt * sizeof(float))) return rc;
        HIP_TRY(hipMemcpyAsync(h->scratch, in, cnt * sizeof(float), hipMemcpyHostToDevice, h->stream));
        src = (const float *)h->scratch;
    }
    hipLaunchKernelGGL(k_aos_to_soa, grid_for(h), dim3(block_size(h)), 0, h->stream, src, h->actuator_m, h->n, nA);
    HIP_TRY(hipGetLastError());
    if (mem == RMAV_HOST) HIP_TRY(hipStreamSynchronize(h->stream));
    return RMAV_OK;
}

// Start-state ranges: the spec on the handle.  Every stepping launch and rmav_reset read start_on (launch_rollout_kms, launch_step_k,
// launch_step_final_k, launch_reset; rmav_ppo_abi.hip) and derive h / m from the spec when they are enqueued; the policy kernels read the
// device copy in the arena, which every set rewrites in stream order with one small launch.  Nothing is drawn, allocated or synchronised.
int rmav_set_start_state(rmav_handle h, const rmav_start_state_spec *spec) {
    CHECK_HANDLE(h);
    if (!spec) {   // none: the launches of a handle that never had a spec
        h->start_on = 0;
        return RMAV_OK;
    }
    if (h->kind == RMAV_REINMAV) return rmav_fail(RMAV_ERR_INVALID, "ReinmavEnv takes no start-state spec (its reset() is a no-op)");
    const int nS = kStateDim[h->kind];
    for (int c = 0; c < 16; ++c) {
        const float lo = spec->lo[c], hi = spec->hi[c];
        if (!(lo - lo == 0.0f) || !(hi - hi == 0.0f))
            return rmav_fail(RMAV_ERR_INVALID, "every lo and hi of a start-state spec must be finite (component %d is not)", c);
        if (!(lo <= hi)) return rmav_fail(RMAV_ERR_INVALID, "start-state lo[%d] = %g is above hi[%d] = %g", c, (double)lo, c, (double)hi);
        if (c >= nS && (lo != 0.0f || hi != 0.0f))
            return rmav_fail(RMAV_ERR_INVALID, "start-state lo[%d] = %g, hi[%d] = %g: the kind has %d state components, the others must be 0", c, (double)lo, c,
                             (double)hi, nS);
    }
    const rmav_start_state_spec old = h->start;
    h->start = *spec;
    if (int rc = rmav_sync_start_dev(h)) {   // the policy kernels' copy, in stream order
        h->start = old;
        if (h->start_on) (void)rmav_sync_start_dev(h);
        return rc;
    }
    h->start_on = 1;
    return RMAV_OK;
}

int rmav_get_start_state(rmav_handle h, rmav_start_state_spec *out, int32_t *enabled) {
    if (!valid(h)) return rmav_fail(RMAV_ERR_INVALID, "invalid rmav_handle");
    if (out) *out = h->start;   // (the last spec set - zeros before the first - also while it is switched off)
    if (enabled) *enabled = h->start_on;
    return RMAV_OK;
}

// Termination rules: the spec on the handle.  Every stepping launch reads term_on (launch_rollout_kms, launch_step_k, launch_step_final_k;
// rmav_ppo_abi.hip) and derives the thresholds from the spec when it is enqueued; the policy kernels read the device copy in the arena,
// which every set rewrites in stream order with one small launch.  Nothing is allocated or synchronised; rmav_reset does not look here.
int rmav_set_termination(rmav_handle h, const rmav_termination_spec *spec) {
    CHECK_HANDLE(h);
    if (!spec) {   // none: the launches of a handle that never had a spec
        h->term_on = 0;
        return RMAV_OK;
    }
    if (h->kind == RMAV_REINMAV) return rmav_fail(RMAV_ERR_INVALID, "ReinmavEnv takes no termination spec (its step() ends every episode)");
    for (int i = 0; i < 3; ++i) {
        const float lo = spec->pos_lo[i], hi = spec->pos_hi[i];
        if (lo != lo || hi != hi) return rmav_fail(RMAV_ERR_INVALID, "termination pos_lo[%d] / pos_hi[%d] is NaN", i, i);
        if (!(lo <= hi)) return rmav_fail(RMAV_ERR_INVALID, "termination pos_lo[%d] = %g is above pos_hi[%d] = %g", i, (double)lo, i, (double)hi);
    }
    const float mt = spec->max_tilt;
    if (!((mt >= 0.0f && mt <= 3.14159274101257324f) || mt == __builtin_inff()))   // (pi as fp32 rounds it)
        return rmav_fail(RMAV_ERR_INVALID, "termination max_tilt = %g must lie in [0, pi] or be +inf (none)", (double)mt);
    if (spec->_reserved != 0) return rmav_fail(RMAV_ERR_INVALID, "termination _reserved must be 0");
    const rmav_termination_spec old = h->term;
    h->term = *spec;
    if (int rc = rmav_sync_term_dev(h)) {   // the policy kernels' copy, in stream order
        h->term = old;
        if (h->term_on) (void)rmav_sync_term_dev(h);
        return rc;
    }
    h->term_on = 1;
    return RMAV_OK;
}

int rmav_get_termination(rmav_handle h, rmav_termination_spec *out, int32_t *enabled) {
    if (!valid(h)) return rmav_fail(RMAV_ERR_INVALID, "invalid rmav_handle");
    if (out) *out = h->term;   // (the last spec set - zeros before the first - also while it is switched off)
    if (enabled) *enabled = h->term_on;
    return RMAV_OK;
}

int rmav_set_time_limit(rmav_handle h, int32_t max_episode_steps) {
    CHECK_HANDLE(h);
    if (h->kind == RMAV_REINMAV && max_episode_steps != 0)
        return rmav_fail(RMAV_ERR_INVALID, "ReinmavEnv ends an episode on every step: it takes no time limit");
    if (max_episode_steps < 0 || max_episode_steps > (1 << 30))
        return rmav_fail(RMAV_ERR_INVALID, "max_episode_steps must be in [0, 2^30] (0 = no limit), got %d", (int)max_episode_steps);
    if (max_episode_steps > 0) {
        if (int rc = ensure_last_trunc(h)) return rc;
        // without episode tracking ep_start is not kept up to date: the running episodes count from this call
        if (!(h->flags & RMAV_F_TRACK_EPISODES))
            if (int rc = restart_episode_clocks(h)) return rc;
    }
    h->time_limit = max_episode_steps;
    return RMAV_OK;
}

int rmav_get_time_limit(rmav_handle h, int32_t *out) {
    CHECK_HANDLE(h);
    if (!out) return rmav_fail(RMAV_ERR_INVALID, "out is NULL");
    *out = h->time_limit;
    return RMAV_OK;
}

int rmav_episode_truncated(rmav_handle h, uint8_t *out, int mem) {
    CHECK_HANDLE(h);
    if (int rc = check_mem_layout(mem, RMAV_SOA)) return rc;
    if (int rc = ensure_last_trunc(h)) return rc;
    return copy_out(h, (const uint8_t *)h->last_trunc, out, (size_t)h->n, mem);
}

int rmav_step_final(rmav_handle h, const float *actions, float *obs_out, float *rew_out, uint8_t *done_out, float *final_obs_out,
                    uint8_t *trunc_out, int mem, int layout) {
    CHECK_HANDLE(h);
    if (!actions) return rmav_fail(RMAV_ERR_INVALID, "actions is NULL");
    if (h->kind == RMAV_REINMAV)
        return rmav_fail(RMAV_ERR_INVALID, "ReinmavEnv takes no time limit and never resets: rmav_step's obs is its terminal observation");
    return rollout_impl(h, 1, RMAV_ACT_BUFFER, actions, nullptr, obs_out, rew_out, done_out, nullptr, mem, layout, 1, 0, true, final_obs_out,
                        trunc_out);
}

}  // extern "C"

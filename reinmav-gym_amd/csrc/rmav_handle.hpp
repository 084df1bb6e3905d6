// rmav_handle.hpp - the one internal header of the translation units behind the C ABI: the handle / communicator structs, the error
// helper, the handle check, the launch helpers, and the functions that cross a unit boundary.  librmav.so is built from one unit per
// public header (rmav_abi.hip, rmav_ppo_abi.hip, rmav_comm_abi.hip) plus thirteen that only launch kernels (rmav_policy_abi.hip,
// rmav_range_abi.hip, rmav_skip_abi.hip, rmav_reward_abi.hip, rmav_disturb_abi.hip, rmav_sensor_abi.hip, rmav_sensor_policy_abi.hip,
// rmav_actuator_abi.hip, rmav_actuator_policy_abi.hip, rmav_start_abi.hip, rmav_start_policy_abi.hip, rmav_term_abi.hip, rmav_term_policy_abi.hip), so that they compile side by side; all of them take the same compiler flags but for ABIFLAGS (Makefile).
#pragma once

#include "../../include/rmav.h"

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <type_traits>

#include <rccl/rccl.h>   // types only: the RCCL entry points are resolved with dlopen/dlsym on first use

#include "rmav_derive.hpp"
#include "rmav_kernels.hpp"

#define RMAV_INTERNAL __attribute__((visibility("hidden")))

// sets the thread-local message rmav_last_error() returns and hands `code` back (defined in rmav_abi.hip)
RMAV_INTERNAL int rmav_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return rmav_fail(RMAV_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),  \
                             __FILE__, __LINE__);                                                  \
    } while (0)

constexpr uint32_t kMagic = 0x524d4156u;  // 'RMAV'
constexpr int kNumKinds = 5;
constexpr int kStateDim[kNumKinds] = {5, 9, 10, 16, 13};
constexpr int kActionDim[kNumKinds] = {2, 2, 4, 4, 4};

struct rmav_env_s {
    uint32_t magic;
    int kind;
    int64_t n;
    int device;
    uint64_t seed;
    uint64_t env_base;
    uint32_t flags;
    rmav_params params;
    hipStream_t stream;
    bool own_stream;
    uint64_t t;  // global step counter
    int64_t chunk;  // > 0 only inside rmav_rollout_chunked: the call's trajectory arrays are chunk-major [n_chunks][T][dim][chunk]
    // device-resident env data
    float *state;
    rmav::EnvRec *rec;   // per-env termination record {sbd, reset_cnt, ep_start, last_len} (rmav_kernels.hpp: EnvRec, ep_clock0)
    float *ep_ret, *last_ret;
    rmav::Totals *totals;
    double *env_time;  // RMAV_REINMAV only
    void *arena;       // ONE allocation behind all of the arrays above (see rmav_create)
    float *pe[3];      // per-env constants (rmav_set_env_param), nullptr = shared
    // scratch for host-pointer calls and layout conversion (grown on demand)
    void *scratch;
    size_t scratch_bytes;
    // small host-pointer calls (the gym-shaped single env, batch <= a few thousand): one block of pinned,
    // device-mapped host memory.  The kernel reads the actions from it and writes obs / reward / done into it
    // over PCIe, so such a call is one launch + one stream synchronise - no staging copies at all.
    void *pinned;
    void *pinned_dev;
    size_t pinned_bytes;
    // completion word of single-wavefront k_step launches through the pinned block (RolloutArgs::done_flag)
    uint32_t *done_flag, *done_flag_dev;
    uint32_t done_seq;
    // statistics exchange armed for the next fused rollout launch (rmav_allgather_stats_arm): where that launch's wavefronts
    // snapshot their envs' statistics and publish their arrival; `fired` once a launch has taken it
    struct {
        bool armed, fired;
        bool allow;   // the call in progress is ONE fused launch over all envs (set by rollout_impl / rmav_rollout_policy)
        bool stale;   // another stepping launch followed the one that took the snapshot: _post must pack again
        bool no_start;   // the launch that took it does not publish a start word (rmav::publishes_start): bounded by the overall limit only
        struct rmav_comm_s *comm;
        int slot;
        int64_t cmax;
        uint32_t seq, expected;
    } xchg;
    // explicit per-handle overrides of the launch heuristics (rmav_set_tuning); -1 / 0 = automatic
    int tune[RMAV_TUNE_COUNT];
    // episode time limit (rmav_set_time_limit): 0 = none; > 0 routes every stepping launch to the *_tl kernels.  last_trunc: u8 [N]
    // truncated flags of the last finished episodes, allocated (zero-filled) on first use
    int32_t time_limit;
    uint8_t *last_trunc;
    // per-episode domain randomisation (rmav_set_env_param_range): bit `which` of range_mask = pe[which] is redrawn from
    // [range_lo, range_hi] whenever its env's state is; != 0 routes every stepping launch to the *_dr kernels
    uint32_t range_mask;
    float range_lo[3], range_hi[3];
    // what the ranged policy kernels (the *_nrm bodies) are fed when the caller passed none: identity tables (allocated on first use)
    // and, on a time-limited handle, a boot_out nobody reads (grown on demand)
    rmav::RangeArgs *range_dev;   // device copy of range_args(h) for the kernels that take it by pointer (k_rollout_nrm_dr); kept current by sync_range_dev
    float *ident_norm;
    float *boot_scratch;
    size_t boot_scratch_bytes;
    // action rule of the policy rollouts (rmav_set_policy_action_rule): deterministic = the mean action, [lo, hi] = what the dynamics
    // clip the action to.  The identity (0, -inf, +inf; rmav_create) launches what a handle without a rule launches; any other rule
    // routes rmav_rollout_policy / _boot / _norm as a parameter range does - to the normalised kernels, which take it (ActRuleArgs)
    int32_t rule_det;
    float rule_lo, rule_hi;
    // frame skip (rmav_set_frame_skip): dynamics sub-steps per agent step, 1 = none (rmav_create).  > 1 routes every stepping launch to the
    // *_fs kernels - before the range and the time limit, which those kernels take as well
    int32_t frame_skip;
    // tracking reward (rmav_set_reward): the spec, whether one is set, and its device copy for the kernels that take it by pointer (the
    // policy rollouts; a piece of the arena, rewritten in stream order by every set).  reward_on routes every stepping launch to
    // the *_rw kernels - before the skip, the range and the time limit, which those kernels take as well
    int32_t reward_on;
    rmav_reward_spec reward;
    rmav::RewardArgs *reward_dev;
    // wind / gust disturbance (rmav_set_disturbance): the spec and whether one is set.  disturb_on routes every stepping launch to the
    // *_ds kernels - before the reward, the skip, the range and the time limit, which those kernels take as well
    int32_t disturb_on;
    rmav_disturbance_spec disturb;
    rmav::DisturbSpec *disturb_dev;   // the policy kernels' copy of the spec, in the arena next to reward_dev (k_set_disturbance rewrites it)
    // sensor noise (rmav_set_sensor_noise): the spec and whether one is set.  sensor_on routes every stepping launch to the *_sn kernels -
    // before the disturbance, which those kernels take as well (the all-zero one without a spec) - and rmav_reset's observation to k_observe.
    // The step kernels, the one-wavefront rollouts and k_observe take the spec by value; the policy kernels read sensor_dev.
    int32_t sensor_on;
    rmav_sensor_noise_spec sensor;
    rmav::SensorDev *sensor_dev;   // the policy kernels' copy of the spec, in the arena next to disturb_dev (k_set_sensor_noise rewrites it)
    // actuator lag (rmav_set_actuator): the spec, whether one is set, and the per-env filter state m [nA][N] (allocated and filled with init
    // by the first set; kept, unread, while the feature is off).  actuator_on routes every stepping launch to the *_al kernels - before the
    // sensor noise, which those kernels take as well (switched off by a wave-uniform flag without a spec).  The step kernels and the
    // one-wavefront rollouts take alpha / beta / init by value, derived from the spec and params.dt at the launch; the policy kernels read
    // actuator_dev, which every set - and rmav_set_params - rewrites in stream order.
    int32_t actuator_on;
    rmav_actuator_spec actuator;
    float *actuator_m;
    rmav::ActuatorDev *actuator_dev;   // in the arena next to sensor_dev (k_set_actuator rewrites it)
    // start-state ranges (rmav_set_start_state): the spec and whether one is set.  start_on routes every stepping launch to the *_ss
    // kernels - before the actuator lag, which those kernels take as well (switched off by a wave-uniform flag without a spec) - and
    // rmav_reset to k_reset_ss.  The step kernels, the one-wavefront rollouts and k_reset_ss take h / m by value, derived from the spec at the
    // launch; the policy kernels read start_dev, which every set rewrites in stream order.
    int32_t start_on;
    rmav_start_state_spec start;
    rmav::StartDev *start_dev;   // in the arena next to actuator_dev (k_set_start_state rewrites it)
    // termination rules (rmav_set_termination): the spec and whether one is set.  term_on routes every stepping launch to the *_tc kernels -
    // before the start-state spec, which those kernels take as well (the identity coefficients without one).  The step kernels and the
    // one-wavefront rollouts take the thresholds by value, derived from the spec at the launch; the policy kernels read term_dev, which
    // every set rewrites in stream order.  rmav_reset is untouched: the rule is evaluated on states a step produces.
    int32_t term_on;
    rmav_termination_spec term;
    rmav::TermDev *term_dev;   // in the arena next to start_dev (k_set_termination rewrites it)
};
static_assert(sizeof(rmav_termination_spec) == 32, "seven floats and the reserved word");
// the seven thresholds as the *_tc kernels take them (the 3-D kinds: the cosine of max_tilt, fp64, rounded once)
inline rmav::TermArgs term_args(const rmav_env_s *h) {
    rmav::TermArgs t{};
    for (int i = 0; i < 3; ++i) t.v[i] = h->term.pos_lo[i], t.v[3 + i] = h->term.pos_hi[i];
    t.v[6] = rmav::term_tilt(h->kind, h->term.max_tilt);
    return t;
}
// the identity start coefficients (h = 1, m = 0 below 16: fma(1, v, 0) = v, the bits of a handle without a start-state spec)
inline rmav::StartCoef start_identity() {
    rmav::StartCoef c{};
    for (int i = 0; i < 16; ++i) c.h[i] = 1.0f, c.m[i] = 0.0f;
    return c;
}
static_assert(sizeof(rmav_start_state_spec) == 128, "thirty-two floats");
// h and m of every component (from the spec's lo and hi, in fp64, each rounded once), as the *_ss kernels take them
inline rmav::StartCoef start_coef(const rmav_env_s *h) {
    rmav::StartCoef c{};
    for (int i = 0; i < 16; ++i) rmav::start_coeffs(h->start.lo[i], h->start.hi[i], c.h[i], c.m[i]);
    return c;
}
inline rmav::StartArgs start_args(const rmav_env_s *h) { return rmav::StartArgs{start_coef(h), h->actuator_on ? 1u : 0u, 0u}; }
static_assert(sizeof(rmav_actuator_spec) == 32, "eight floats");
// alpha, beta (from the spec's tau and the dt in force) and init, as the *_al kernels take them
inline rmav::ActuatorCoef actuator_coef(const rmav_env_s *h) {
    rmav::ActuatorCoef c{};
    for (int i = 0; i < 4; ++i) {
        rmav::actuator_coeffs((double)h->actuator.tau[i], (double)h->params.dt, c.alpha[i], c.beta[i]);
        c.init[i] = h->actuator.init[i];
    }
    return c;
}
inline rmav::ActuatorArgs actuator_args(const rmav_env_s *h) { return rmav::ActuatorArgs{actuator_coef(h), h->actuator_m, h->sensor_on ? 1u : 0u, 0u}; }
static_assert(sizeof(rmav_sensor_noise_spec) == 64 && sizeof(rmav::SensorArgs) == 64, "sixteen floats");
// what the *_sn kernels and k_observe take
inline rmav::SensorArgs sensor_args(const rmav_env_s *h) {
    rmav::SensorArgs s{};
    for (int c = 0; c < 16; ++c) s.sigma[c] = h->sensor.sigma[c];
    return s;
}
static_assert(sizeof(rmav_disturbance_spec) == 40, "nine floats and the hold");
// what the *_ds kernels take for a launch whose first step has the step counter t0: the wind as (lo, hi - lo), the gust block and phase of t0
inline rmav::DisturbArgs disturb_args(const rmav_env_s *h, uint64_t t0) {
    rmav::DisturbArgs d{};
    for (int i = 0; i < 3; ++i) {
        d.v.lo[i] = h->disturb.wind_lo[i];
        d.v.span[i] = h->disturb.wind_hi[i] - h->disturb.wind_lo[i];
        d.v.gust[i] = h->disturb.gust[i];
    }
    d.v.hold = h->disturb.gust_hold;
    d.b0 = t0 / (uint64_t)h->disturb.gust_hold;
    d.phase0 = (int32_t)(t0 % (uint64_t)h->disturb.gust_hold);
    return d;
}
// what the *_sn kernels take in the disturbance's place: the handle's spec, or - without one - the all-zero spec (d = +0 leaves g_vec's bits)
// at the longest hold, so that no launch redraws a gust inside its loop
constexpr int32_t kCalmHold = 1048576;
inline rmav::DisturbArgs disturb_or_calm(const rmav_env_s *h, uint64_t t0) {
    if (h->disturb_on) return disturb_args(h, t0);
    rmav::DisturbArgs d{};
    d.v.hold = kCalmHold;
    d.b0 = t0 / (uint64_t)kCalmHold;
    d.phase0 = (int32_t)(t0 % (uint64_t)kCalmHold);
    return d;
}
static_assert(sizeof(rmav_reward_spec) == sizeof(rmav::RewardArgs) && offsetof(rmav_reward_spec, act_ref) == offsetof(rmav::RewardArgs, act_ref) &&
                  offsetof(rmav_reward_spec, terminal) == offsetof(rmav::RewardArgs, terminal),
              "RewardArgs is rmav_reward_spec, field for field");
inline rmav::RewardArgs reward_args(const rmav_env_s *h) {
    rmav::RewardArgs r;
    memcpy(&r, &h->reward, sizeof(r));
    return r;
}
inline rmav::FrameSkipArgs skip_args(const rmav_env_s *h) { return rmav::FrameSkipArgs{h->frame_skip}; }
inline bool has_act_rule(const rmav_env_s *h) { return h->rule_det != 0 || h->rule_lo != -__builtin_inff() || h->rule_hi != __builtin_inff(); }
inline rmav::ActRuleArgs act_rule_args(const rmav_env_s *h) { return rmav::ActRuleArgs{h->rule_det ? 0.0f : 1.0f, h->rule_lo, h->rule_hi}; }
inline rmav::PolicySkipArgs policy_skip_args(const rmav_env_s *h) {
    const rmav::ActRuleArgs r = act_rule_args(h);
    return rmav::PolicySkipArgs{r.noise, r.lo, r.hi, h->frame_skip};
}
inline rmav::PolicyRewardArgs policy_reward_args(const rmav_env_s *h) {
    const rmav::ActRuleArgs r = act_rule_args(h);
    return rmav::PolicyRewardArgs{r.noise, r.lo, r.hi, h->frame_skip, h->reward_dev};
}
// what the disturbed policy kernels take in PolicyRewardArgs' place (the launch's first step has the step counter t0)
inline rmav::PolicyDisturbArgs policy_disturb_args(const rmav_env_s *h, uint64_t t0) {
    const rmav::ActRuleArgs r = act_rule_args(h);
    const rmav::DisturbArgs d = disturb_args(h, t0);
    return rmav::PolicyDisturbArgs{r.noise, r.lo, r.hi, h->frame_skip, h->reward_dev, h->disturb_dev, d.b0, d.phase0, 0};
}
// what the noisy policy kernels take in PolicyDisturbArgs' place: the device copy of the disturbance spec, or the calm one beside the sigmas
inline rmav::PolicySensorArgs policy_sensor_args(const rmav_env_s *h, uint64_t t0) {
    const rmav::ActRuleArgs r = act_rule_args(h);
    const rmav::DisturbArgs d = disturb_or_calm(h, t0);
    return rmav::PolicySensorArgs{r.noise, r.lo, r.hi, h->frame_skip, h->reward_dev, h->disturb_on ? h->disturb_dev : &h->sensor_dev->calm, d.b0, d.phase0, 0,
                                  &h->sensor_dev->sn};
}
// what the lagged policy kernels take in PolicySensorArgs' place: the calm disturbance spec of a handle without one sits in actuator_dev
// (k_set_actuator writes it; sensor_dev's copy exists only once a sensor-noise spec was set); sn is read only with sn_on
inline rmav::PolicyActuatorArgs policy_actuator_args(const rmav_env_s *h, uint64_t t0) {
    const rmav::ActRuleArgs r = act_rule_args(h);
    const rmav::DisturbArgs d = disturb_or_calm(h, t0);
    return rmav::PolicyActuatorArgs{r.noise, r.lo, r.hi, h->frame_skip, h->reward_dev, h->disturb_on ? h->disturb_dev : &h->actuator_dev->calm, d.b0, d.phase0,
                                    h->sensor_on ? 1u : 0u, &h->sensor_dev->sn, &h->actuator_dev->c, h->actuator_m};
}
// what the *_ss kernels take in ActuatorArgs' place: the handle's, or - without actuator lag - zeros and no array (StartArgs::al_on = 0: unread)
inline rmav::ActuatorArgs start_actuator_args(const rmav_env_s *h) {
    if (h->actuator_on) return actuator_args(h);
    return rmav::ActuatorArgs{rmav::ActuatorCoef{}, nullptr, h->sensor_on ? 1u : 0u, 0u};
}
// what the policy kernels of a handle with a start spec take: PolicyActuatorArgs - the calm disturbance spec of a handle without a disturbance
// sits in actuator_dev if the handle has actuator lag (k_set_actuator wrote it), else in start_dev (k_set_start_state did); without actuator
// lag al points at memory of the arena nobody wrote, whose values the kernels load and do not use, and m is NULL and untouched - then the
// device copy of h / m
inline rmav::PolicyStartArgs policy_start_args(const rmav_env_s *h, uint64_t t0) {
    rmav::PolicyActuatorArgs pa = policy_actuator_args(h, t0);
    if (!h->actuator_on) {
        if (!h->disturb_on) pa.ds = &h->start_dev->calm;
        pa.m = nullptr;
    }
    return rmav::PolicyStartArgs{pa, &h->start_dev->c, h->actuator_on ? 1u : 0u, 0u};
}
// what the *_tc kernels take in StartArgs' place: the handle's, or - without a start-state spec - the identity coefficients
inline rmav::StartArgs term_start_args(const rmav_env_s *h) {
    if (h->start_on) return start_args(h);
    return rmav::StartArgs{start_identity(), h->actuator_on ? 1u : 0u, 0u};
}
// what the policy kernels of a handle with a termination spec take: PolicyStartArgs - without a start-state spec the identity coefficients
// and, for a handle with neither a disturbance nor an actuator spec, the calm disturbance spec sit in term_dev (k_set_termination wrote
// them) - then the device copy of the thresholds
inline rmav::PolicyTermArgs policy_term_args(const rmav_env_s *h, uint64_t t0) {
    rmav::PolicyStartArgs ps = policy_start_args(h, t0);
    if (!h->start_on) {
        ps.ss = &h->term_dev->ident;
        if (!h->actuator_on && !h->disturb_on) ps.pa.ds = &h->term_dev->calm;
    }
    return rmav::PolicyTermArgs{ps, &h->term_dev->t};
}
inline rmav::TimeLimitArgs tl_args(const rmav_env_s *h) { return rmav::TimeLimitArgs{h->last_trunc, h->time_limit}; }
// what the *_dr kernels take: the arrays of the ranged parameters (allocated while their bit is set) and the ranges as (lo, hi - lo)
inline rmav::RangeArgs range_args(const rmav_env_s *h, uint32_t mask) {
    rmav::RangeArgs r{};
    for (int w = 0; w < 3; ++w) {
        r.pe[w] = h->pe[w];
        r.lo[w] = h->range_lo[w];
        r.span[w] = h->range_hi[w] - h->range_lo[w];
    }
    r.mask = mask;
    return r;
}
inline rmav::RangeArgs range_args(const rmav_env_s *h) { return range_args(h, h->range_mask); }

RMAV_INTERNAL inline bool valid(rmav_handle h) { return h && h->magic == kMagic; }

// makes the handle's device current for the duration of an entry point
struct RMAV_INTERNAL DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = (hipSetDevice(dev) == hipSuccess);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

#define CHECK_HANDLE(h)                                                                            \
    if (!valid(h)) return rmav_fail(RMAV_ERR_INVALID, "invalid rmav_handle");                           \
    DeviceGuard guard_(h->device);                                                                 \
    if (!guard_.ok) return rmav_fail(RMAV_ERR_HIP, "hipSetDevice(%d) failed", h->device)

// rmav_abi.hip, for rmav_ppo_abi.hip as well: the argument block every stepping launch starts from; the handle's scratch grown to
// `bytes`; and what a ranged handle's policy kernels are fed when the caller passed none (identity tables, an unread boot_out)
RMAV_INTERNAL rmav::RolloutArgs base_args(rmav_handle h);
RMAV_INTERNAL int ensure_scratch(rmav_handle h, size_t bytes);
RMAV_INTERNAL int ensure_ident_norm(rmav_handle h);
RMAV_INTERNAL int ensure_boot_scratch(rmav_handle h, size_t bytes);
// ... and the device copy of the handle's ranges on first use (the kernels that take the range by pointer: k_rollout_nrm_dr / _fs)
RMAV_INTERNAL int ensure_range_dev(rmav_handle h);

constexpr int kExchangeDepth = 8;   // buffer pairs of the overlapped statistics exchange
// bounds of k_wait_arrivals, in ticks of the 100 MHz wall clock: 2 s once the armed launch has begun, 10 min overall
constexpr unsigned long long kArrivalWaitTicks = 200000000ull, kArrivalTotalTicks = 60000000000ull;
struct rmav_comm_s {
    uint32_t magic;
    int rank, world, device;
    ncclComm_t comm;
    // overlapped exchange: the collective runs on the communicator's own stream, double-buffered
    hipStream_t stream;
    hipEvent_t ready[kExchangeDepth], done[kExchangeDepth];
    bool used[kExchangeDepth];
    int32_t *send[kExchangeDepth], *recv[kExchangeDepth];
    int depth;         // buffer pairs in use (RMAV_EXCHANGE_DEPTH, 2 .. kExchangeDepth)
    uint32_t *arrive;  // arrival words of armed launches, one per wavefront: ceil(cmax / 32) of them
    uint32_t *flag;    // signal word (hipMallocSignalMemory): the compute stream publishes post numbers, the comm stream waits
    int64_t cmax;      // capacity of the buffers (per-rank slots of 2 * cmax int32)
    int posts;         // number of posts so far (buffer pair of post i is i % depth)
    struct rmav_env_s *armed_by;   // the handle whose armed exchange points at this communicator (cleared by _post)
    uint32_t *started;             // device word: the armed launch's first workgroup publishes its post number here
    // pinned host words (device-mapped), one per buffer pair: k_wait_arrivals writes the post number it gave up on
    uint32_t *timeout_seq, *timeout_seq_dev;
    uint32_t slot_seq[kExchangeDepth];   // post number that last used each buffer pair
    bool armed_slot[kExchangeDepth];     // ... and whether that post went through the waiter (an armed launch)
};


// Workgroup size of the one-wavefront-per-64-envs kernels: 256, or rmav_set_tuning(RMAV_TUNE_BLOCK, 64 | 128 | 256).
inline int block_size(rmav_handle h) {
    const int v = h->tune[RMAV_TUNE_BLOCK];
    return (v == 64 || v == 128 || v == 256) ? v : 256;
}
inline dim3 grid_for(rmav_handle h) { return dim3((unsigned)((h->n + block_size(h) - 1) / block_size(h))); }

// An armed statistics exchange rides on the first call after rmav_allgather_stats_arm that is ONE fused launch over all
// envs (xchg.allow: rollout_impl with fused != 0 / rmav_rollout_policy; not the fused = 0 loop of single-step launches,
// whose first launch would snapshot the statistics T - 1 steps early, and not a sliced launch).  Any later stepping
// launch makes that snapshot stale, and _post then packs afresh.  envs_per_word: envs behind one arrival word (64; 32 for
// the fp32-MFMA actor's half-wavefront layout).
inline void take_armed_exchange(rmav_handle h, rmav::RolloutArgs &a, int envs_per_word, bool publishes_start = true) {
    if (h->xchg.armed && h->xchg.fired) h->xchg.stale = true;
    if (h->xchg.armed && !h->xchg.fired && h->xchg.allow && a.slice_count == 0 && (a.flags & rmav::F_TRACK)) {
        rmav_comm_s *c = h->xchg.comm;
        a.xsend = c->send[h->xchg.slot];
        a.xcmax = h->xchg.cmax;
        a.xarrive = c->arrive;
        a.xseq = h->xchg.seq;
        a.xstarted = c->started;
        h->xchg.expected = (uint32_t)((h->n + envs_per_word - 1) / envs_per_word);
        h->xchg.fired = true;
        h->xchg.no_start = !publishes_start;
    }
}

// Right after the hipLaunchKernelGGL of a rollout that may have taken the armed exchange: a launch that failed will never publish
// its arrival words, so the exchange goes back to "armed, not fired" and rmav_allgather_stats_post packs as usual.  (One copy, out of
// line: every instantiation of the rollout launchers ends with it.)
__attribute__((noinline)) inline int check_rollout_launch(rmav_handle h, const rmav::RolloutArgs &a) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return RMAV_OK;
    if (a.xsend) h->xchg.fired = false;
    return rmav_fail(RMAV_ERR_HIP, "rollout kernel launch failed: %s", hipGetErrorString(e));
}

// ---- runtime value -> compile-time constant ------------------------------------------------------------------------------------
// The handle's kind as std::integral_constant<int, K>: f is a generic lambda, `constexpr int K = decltype(k)::value` inside it.
// ALL_KINDS = the four quadrotor kinds and ReinmavEnv, QUAD_KINDS = the quadrotor kinds only (no kernel of f's family exists for
// ReinmavEnv, and f is not instantiated for it).  A plain switch over inlined lambdas: nothing is stored, nothing allocates.
enum KindSet : bool { QUAD_KINDS = false, ALL_KINDS = true };
template <KindSet SET, typename F> inline auto dispatch_kind(int kind, F &&f) -> decltype(f(std::integral_constant<int, rmav::QUAD2D>{})) {
    switch (kind) {
    case RMAV_QUAD2D: return f(std::integral_constant<int, rmav::QUAD2D>{});
    case RMAV_QUAD2D_SL: return f(std::integral_constant<int, rmav::QUAD2D_SL>{});
    case RMAV_QUAD3D: return f(std::integral_constant<int, rmav::QUAD3D>{});
    case RMAV_QUAD3D_SL: return f(std::integral_constant<int, rmav::QUAD3D_SL>{});
    case RMAV_REINMAV:
        if constexpr (SET == ALL_KINDS) return f(std::integral_constant<int, rmav::REINMAV>{});
        break;
    }
    return rmav_fail(RMAV_ERR_INVALID, "bad kind %d", kind);
}
// A store policy (rmav_kernels.hpp: ST_*) as std::integral_constant<int, ST>.  The call site names the policies its kernel family is
// instantiated for: FALLBACK, which also takes every value outside the set, then the others.  f is instantiated for those only.
template <int FALLBACK, int... OTHERS, typename F> inline auto dispatch_store(int st, F &&f) {
    constexpr auto allowed = [](int v) { return ((v == OTHERS) || ...); };
    switch (st) {
    case rmav::ST_DEFAULT:
        if constexpr (allowed(rmav::ST_DEFAULT)) return f(std::integral_constant<int, rmav::ST_DEFAULT>{});
        break;
    case rmav::ST_WRITE_THROUGH:
        if constexpr (allowed(rmav::ST_WRITE_THROUGH)) return f(std::integral_constant<int, rmav::ST_WRITE_THROUGH>{});
        break;
    case rmav::ST_STREAM:
        if constexpr (allowed(rmav::ST_STREAM)) return f(std::integral_constant<int, rmav::ST_STREAM>{});
        break;
    case rmav::ST_AOS_LDS:
        if constexpr (allowed(rmav::ST_AOS_LDS)) return f(std::integral_constant<int, rmav::ST_AOS_LDS>{});
        break;
    }
    return f(std::integral_constant<int, FALLBACK>{});
}

// The per-kind constants every stepping kernel takes: the env's own (Env<K>::P) and the fp64 controller's.
template <int K> struct KindParams {
    typename rmav::Env<K>::P p;
    rmav::ParamsT<double> pc;
};
template <int K> RMAV_INTERNAL inline KindParams<K> kind_params(const rmav_env_s *h) {
    return {rmav::derive_env<K>(h->params), rmav::derive<double>(h->params, h->kind == RMAV_QUAD2D || h->kind == RMAV_QUAD2D_SL)};
}

// The policy actors.  policy_kmode: the kernel mode of an rmav_policy_precision, -1 for a value outside the enum.
// policy_has_variants: THE capability rule - the fp32-MFMA actor, the f16 pair and the shared-trunk pair have *_tl / *_boot / *_nrm / *_dr
// kernels (on a quadrotor kind); the fp32 vector-ALU and bf16 actors have the plain kernel only.
constexpr int policy_kmode(int precision) {
    switch (precision) {
    case RMAV_POLICY_FP32: return RMAV_ACT_POLICY;
    case RMAV_POLICY_BF16_MFMA: return RMAV_ACT_POLICY_BF16;
    case RMAV_POLICY_FP32_MFMA: return rmav::ACT_POLICY_F32M;
    case RMAV_POLICY_F16_MFMA: return rmav::ACT_POLICY_F16;
    case RMAV_POLICY_F16_SHARED: return rmav::ACT_POLICY_F16_SHARED;
    }
    return -1;
}
constexpr bool policy_has_variants(int kmode) {
    return kmode == rmav::ACT_POLICY_F32M || kmode == rmav::ACT_POLICY_F16 || kmode == rmav::ACT_POLICY_F16_SHARED;
}

// rmav_policy_abi.hip: launches the kernel of rmav_rollout_policy / _boot / _norm for kmode = RMAV_ACT_POLICY | RMAV_ACT_POLICY_BF16 |
// ACT_POLICY_F32M | ACT_POLICY_F16 | ACT_POLICY_F16_SHARED on the handle's stream.
// bt (rmav_rollout_policy_boot): the launch also leaves the bootstrap term of its truncated steps - the *_boot kernels; nullptr otherwise.
// nm (rmav_rollout_policy_norm): the *_nrm kernels; kmode = ACT_POLICY_F32M | ACT_POLICY_F16 | ACT_POLICY_F16_SHARED, a quadrotor kind; bt is
// required with it when the handle has a time limit and ignored otherwise.
RMAV_INTERNAL int rmav_launch_policy_rollout(rmav_handle h, int kmode, const rmav::RolloutArgs &a, const rmav::BootArgs *bt = nullptr,
                                             const rmav::NormArgs *nm = nullptr);

// The rung units (the feature ladder: rmav_ladder.hpp has the order, the table of these launchers and what routes through it).  Every rung
// has a unit rmav_<x>_abi.hip with two launchers of one shape, and the kernels of a rung take the arguments of every rung below as well
// (rmav_rung_launch.hpp: rung_tail; a feature the handle lacks is passed switched off - mask = 0, k = 1, the all-zero disturbance, ...):
//   _rollout  ONE launch of k_rollout_<x> over the envs a names: mode = ACT_BUFFER | ACT_RANDOM | ACT_CONTROLLER; st = a store policy for
//             the rungs up to the tracking reward (ST_AOS_LDS runs the write-through kernel), ignored above (one store policy).  a.t0 is the
//             step counter of the launch's first step.
//   _step     k_step_<x> at bs threads per workgroup; fa = what rmav_step_final wants (NULL pointers otherwise); ctrl = the launch ends with
//             control(): the ranged kernel alone has that form, the others ignore it.
// The rungs from the sensor noise up also have a policy unit rmav_<x>_policy_abi.hip whose _policy_rollout launches k_rollout_nrm_<x>,
// k_rollout_pair_<x> or k_rollout_pair_shared_<x> with rmav_launch_policy_rollout's arguments (kmode = ACT_POLICY_F32M | ACT_POLICY_F16 |
// ACT_POLICY_F16_SHARED, any other is RMAV_ERR_INVALID; nm is required, bt on a time-limited handle); the rungs below are variants of
// rmav_policy_abi.hip's kernels.  The _sync functions rewrite the handle's device copy of a spec (what the policy kernels read by pointer)
// with one small launch on the handle's stream: no allocation, no synchronisation.  The caller checks hipGetLastError.
// a parameter range (rmav_set_env_param_range): k_rollout_dr<K, mode, st, time limit?>, k_step_dr<K, ctrl, time limit?>
RMAV_INTERNAL int rmav_launch_ranged_rollout(rmav_handle h, int mode, int st, const rmav::RolloutArgs &a);
RMAV_INTERNAL int rmav_launch_ranged_step(rmav_handle h, const rmav::RolloutArgs &a, bool ctrl, int bs, const rmav::FinalArgs &fa);
// a frame skip (rmav_set_frame_skip): k_rollout_fs, k_step_fs<K, time limit?> (rollout_impl refuses the control() form)
RMAV_INTERNAL int rmav_launch_skip_rollout(rmav_handle h, int mode, int st, const rmav::RolloutArgs &a);
RMAV_INTERNAL int rmav_launch_skip_step(rmav_handle h, const rmav::RolloutArgs &a, bool ctrl, int bs, const rmav::FinalArgs &fa);
// a tracking reward (rmav_set_reward): k_rollout_rw, k_step_rw; _sync: k_set_reward (reward_dev)
RMAV_INTERNAL int rmav_launch_reward_rollout(rmav_handle h, int mode, int st, const rmav::RolloutArgs &a);
RMAV_INTERNAL int rmav_launch_reward_step(rmav_handle h, const rmav::RolloutArgs &a, bool ctrl, int bs, const rmav::FinalArgs &fa);
RMAV_INTERNAL int rmav_sync_reward_dev(rmav_handle h);
// a disturbance (rmav_set_disturbance): k_rollout_ds<K, mode, time limit?, reward?>, k_step_ds<K, time limit?, reward?> - the shape of every rung
// from here up; _now: k_disturbance_now into out [3][N] (device memory); _sync: k_set_disturbance (disturb_dev)
RMAV_INTERNAL int rmav_launch_disturb_rollout(rmav_handle h, int mode, int st, const rmav::RolloutArgs &a);
RMAV_INTERNAL int rmav_launch_disturb_step(rmav_handle h, const rmav::RolloutArgs &a, bool ctrl, int bs, const rmav::FinalArgs &fa);
RMAV_INTERNAL int rmav_launch_disturbance_now(rmav_handle h, float *out_dev);
RMAV_INTERNAL int rmav_sync_disturb_dev(rmav_handle h);
// sensor noise (rmav_set_sensor_noise): k_rollout_sn, k_step_sn; _observe: k_observe of the current state at the handle's step counter into
// out (device memory, nS * N floats in `layout`); _sync: k_set_sensor_noise (sensor_dev)
RMAV_INTERNAL int rmav_launch_sensor_rollout(rmav_handle h, int mode, int st, const rmav::RolloutArgs &a);
RMAV_INTERNAL int rmav_launch_sensor_step(rmav_handle h, const rmav::RolloutArgs &a, bool ctrl, int bs, const rmav::FinalArgs &fa);
RMAV_INTERNAL int rmav_launch_sensor_policy_rollout(rmav_handle h, int kmode, const rmav::RolloutArgs &a, const rmav::BootArgs *bt, const rmav::NormArgs *nm);
RMAV_INTERNAL int rmav_launch_observe(rmav_handle h, float *out_dev, int layout);
RMAV_INTERNAL int rmav_sync_sensor_dev(rmav_handle h);
// actuator lag (rmav_set_actuator): k_rollout_al, k_step_al; _fill: k_actuator_fill, which sets every env's m to the spec's init, in stream
// order; _sync: k_set_actuator (actuator_dev)
RMAV_INTERNAL int rmav_launch_actuator_rollout(rmav_handle h, int mode, int st, const rmav::RolloutArgs &a);
RMAV_INTERNAL int rmav_launch_actuator_step(rmav_handle h, const rmav::RolloutArgs &a, bool ctrl, int bs, const rmav::FinalArgs &fa);
RMAV_INTERNAL int rmav_launch_actuator_policy_rollout(rmav_handle h, int kmode, const rmav::RolloutArgs &a, const rmav::BootArgs *bt, const rmav::NormArgs *nm);
RMAV_INTERNAL int rmav_launch_actuator_fill(rmav_handle h);
RMAV_INTERNAL int rmav_sync_actuator_dev(rmav_handle h);
// a start-state spec (rmav_set_start_state): k_rollout_ss, k_step_ss; _reset: k_reset_ss, launch_reset's arguments; _sync: k_set_start_state (start_dev)
RMAV_INTERNAL int rmav_launch_start_rollout(rmav_handle h, int mode, int st, const rmav::RolloutArgs &a);
RMAV_INTERNAL int rmav_launch_start_step(rmav_handle h, const rmav::RolloutArgs &a, bool ctrl, int bs, const rmav::FinalArgs &fa);
RMAV_INTERNAL int rmav_launch_start_policy_rollout(rmav_handle h, int kmode, const rmav::RolloutArgs &a, const rmav::BootArgs *bt, const rmav::NormArgs *nm);
RMAV_INTERNAL int rmav_launch_start_reset(rmav_handle h, float *obs_dev, int layout);
RMAV_INTERNAL int rmav_sync_start_dev(rmav_handle h);
// a termination spec (rmav_set_termination): k_rollout_tc, k_step_tc; _sync: k_set_termination (term_dev)
RMAV_INTERNAL int rmav_launch_term_rollout(rmav_handle h, int mode, int st, const rmav::RolloutArgs &a);
RMAV_INTERNAL int rmav_launch_term_step(rmav_handle h, const rmav::RolloutArgs &a, bool ctrl, int bs, const rmav::FinalArgs &fa);
RMAV_INTERNAL int rmav_launch_term_policy_rollout(rmav_handle h, int kmode, const rmav::RolloutArgs &a, const rmav::BootArgs *bt, const rmav::NormArgs *nm);
RMAV_INTERNAL int rmav_sync_term_dev(rmav_handle h);

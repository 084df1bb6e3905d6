// rmav_ppo_abi.hip - the C ABI of include/rmav_ppo.h: policy weights, the policy-in-kernel rollouts (their kernels are launched from
// rmav_policy_abi.hip), GAE, the observation / return normalisers, the fused learners (rmav_ppo_grad, rmav_ppo_grad_shared, rmav_ppo_grad_shared_mfma) and what
// runs around them in a minibatch (rmav_adv_moments, rmav_ppo_adam).
#include <cmath>
#include <cstdint>
#include <cstring>

#include "rmav_ladder.hpp"
#include "rmav_pack_policy.hpp"
#include "rmav_obs_norm.hpp"
#include "rmav_ret_norm.hpp"   // (brings rmav_gae.hpp)
#include "rmav_learner.hpp"
#include "rmav_learner_shared.hpp"
#include "rmav_learner_mfma.hpp"
#include "rmav_optim.hpp"

using namespace rmav;

// =================================================================================================
extern "C" {

int64_t rmav_policy_weight_count(int kind) {
    return dispatch_kind<ALL_KINDS>(kind, [](auto k) { return (int64_t)PolicyLayout<Dims<decltype(k)::value>::NS>::TOTAL; });
}

int64_t rmav_policy_weight_count_bf16(void) { return MfmaLayout::TOTAL; }
int64_t rmav_policy_weight_count_f32_mfma(void) { return Mfma32Layout::TOTAL; }
int64_t rmav_policy_weight_count_shared(void) { return MfmaLayout::NET + 4; }

static int pack_policy_impl(rmav_handle h, int n_params, const float *const *params, const int64_t *sizes, const int32_t *idx_lo,
                            const int32_t *idx_hi, int64_t n_out, float *weights_out, bool f16) {
    CHECK_HANDLE(h);
    if (n_params <= 0 || n_params > kPackMaxParams) return rmav_fail(RMAV_ERR_INVALID, "n_params must be in [1, %d]", kPackMaxParams);
    if (!params || !sizes || !idx_lo || !idx_hi || !weights_out || n_out <= 0)
        return rmav_fail(RMAV_ERR_INVALID, "params, sizes, idx_lo, idx_hi, weights_out are required and n_out > 0");
    PackSrc src;
    memset(&src, 0, sizeof(src));
    int64_t end = 0;
    for (int k = 0; k < n_params; ++k) {
        if (!params[k] || sizes[k] < 0) return rmav_fail(RMAV_ERR_INVALID, "parameter %d is NULL or has a negative size", k);
        end += sizes[k];
        if (end > 0x7fffffff) return rmav_fail(RMAV_ERR_INVALID, "too many parameter elements");
        src.p[k] = params[k];
        src.end[k] = (int32_t)end;
    }
    src.n = n_params;
    const dim3 grid((unsigned)((n_out + 255) / 256));
    if (f16) {
        if (n_out != MfmaLayout::TOTAL && n_out != MfmaLayout::NET + 4)
            return rmav_fail(RMAV_ERR_INVALID, "n_out must be rmav_policy_weight_count_bf16() = %d or rmav_policy_weight_count_shared() = %d",
                             (int)MfmaLayout::TOTAL, (int)MfmaLayout::NET + 4);
        hipLaunchKernelGGL(k_pack_policy<true>, grid, dim3(256), 0, h->stream, src, idx_lo, idx_hi, n_out, weights_out, (int32_t)MfmaLayout::NET,
                           (int32_t)MfmaLayout::A2, (int32_t)MfmaLayout::A3, (int32_t)MfmaLayout::B1, -2.0f * kTanhScale, -2.0f);
    } else {
        hipLaunchKernelGGL(k_pack_policy<false>, grid, dim3(256), 0, h->stream, src, idx_lo, idx_hi, n_out, weights_out, 1, 0, 0, 0, 1.0f, 1.0f);
    }
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

int rmav_pack_policy(rmav_handle h, int n_params, const float *const *params, const int64_t *sizes, const int32_t *idx_lo,
                     const int32_t *idx_hi, int64_t n_out, float *weights_out) {
    return pack_policy_impl(h, n_params, params, sizes, idx_lo, idx_hi, n_out, weights_out, false);
}
int rmav_pack_policy_f16(rmav_handle h, int n_params, const float *const *params, const int64_t *sizes, const int32_t *idx_lo,
                         const int32_t *idx_hi, int64_t n_out, float *weights_out) {
    return pack_policy_impl(h, n_params, params, sizes, idx_lo, idx_hi, n_out, weights_out, true);
}

// ---- rmav_rollout_policy / _boot / _norm: the checks all three make, in the order they make them, and the launch ------------------
// The refusal of an actor without variant kernels (policy_has_variants, rmav_handle.hpp): `who` = the entry point or the handle's feature,
// `what` = the kind of kernel the fp32 vector-ALU and bf16 actors lack.  RMAV_OK for the three actors that have them.
static int need_variants(int precision, const char *who, const char *what) {
    if (policy_has_variants(policy_kmode(precision))) return RMAV_OK;
    return rmav_fail(RMAV_ERR_INVALID, "%s runs RMAV_POLICY_FP32_MFMA, RMAV_POLICY_F16_MFMA or RMAV_POLICY_F16_SHARED "
                                       "(the fp32 vector-ALU and bf16 actors have no %s kernel), got precision %d", who, what, precision);
}
// boot_out: checked (and named) only when the entry point requires it
static int check_policy_args(int32_t n_steps, const float *weights, const float *logp_out, const float *value_out, bool need_boot, const float *boot_out) {
    if (n_steps <= 0) return rmav_fail(RMAV_ERR_INVALID, "n_steps must be > 0");
    if (!weights || !logp_out || !value_out || (need_boot && !boot_out))
        return rmav_fail(RMAV_ERR_INVALID, need_boot ? "weights, logp_out, value_out and boot_out are required (device pointers)"
                                                     : "weights, logp_out and value_out are required (device pointers)");
    if ((reinterpret_cast<uintptr_t>(weights) & 15u) != 0) return rmav_fail(RMAV_ERR_INVALID, "weights must be 16-byte aligned");
    return RMAV_OK;
}
// one fused launch over all envs (it may carry an armed exchange's snapshot), then the step counter
static int launch_policy_call(rmav_handle h, int32_t n_steps, const float *weights, float *actions_out, float *obs_out, float *rew_out,
                              uint8_t *done_out, float *logp_out, float *value_out, int precision, const BootArgs *bt, const NormArgs *nm) {
    RolloutArgs a = base_args(h);
    a.n_steps = n_steps;
    a.act_out = actions_out;
    a.obs_out = obs_out;
    a.rew_out = rew_out;
    a.done_out = done_out;
    a.policy_w = weights;
    a.logp_out = logp_out;
    a.val_out = value_out;
    h->xchg.allow = true;
    // A handle with a parameter range runs ONE ranged kernel per actor, the normalised one: a call without
    // statistics gets identity tables - z then has the bits of x (rmav_ppo.h) - and a call on a time-limited handle that asked for no
    // bootstrap term a boot_out of the handle's own.  A handle whose policy action rule is not the identity goes the same way: the
    // normalised kernels are the ones that take the rule.
    BootArgs bt_r{};
    NormArgs nm_r{};
    const bool ruled = has_act_rule(h);
    if (ruled) {
        if (h->kind == RMAV_REINMAV)
            return rmav_fail(RMAV_ERR_INVALID, "a handle with a policy action rule (rmav_set_policy_action_rule) runs the four quadrotor kinds, "
                                               "not RMAV_REINMAV: there is no action-rule kernel for it");
        if (int rc = need_variants(precision, "a handle with a policy action rule (rmav_set_policy_action_rule)", "action-rule")) return rc;
    }
    // ... and so does a handle on a rung above the range (rmav_ladder.hpp): the policy kernels of every rung from the frame skip up are cut
    // from the ranged normalised ones, and those of the rung below them
    const Rung r = rung_of(h);
    const bool skipped = r >= RUNG_SKIP;
    if (skipped) {
        if (int rc = need_variants(precision, kLadder[r].who, kLadder[r].noun)) return rc;
        if (int rc = ensure_range_dev(h)) return rc;
    }
    if (h->range_mask || ruled || skipped) {
        if (h->range_mask)
            if (int rc = need_variants(precision, kLadder[RUNG_RANGE].who, kLadder[RUNG_RANGE].noun)) return rc;
        if (!nm) {
            if (int rc = ensure_ident_norm(h)) return rc;
            nm_r.tab = h->ident_norm;
            nm = &nm_r;
        }
        if (h->time_limit > 0 && !bt) {
            if (int rc = ensure_boot_scratch(h, (size_t)n_steps * (size_t)h->n * sizeof(float))) return rc;
            bt_r.boot_out = h->boot_scratch;
            bt = &bt_r;
        }
    }
    if (int rc = kLadder[r].policy(h, policy_kmode(precision), a, bt, nm)) return rc;   // (the rungs below the sensor noise: rmav_policy_abi.hip's kernels)
    h->t += (uint64_t)n_steps;
    return RMAV_OK;
}

int rmav_rollout_policy(rmav_handle h, int32_t n_steps, const float *weights, float *actions_out,
                        float *obs_out, float *rew_out, uint8_t *done_out, float *logp_out,
                        float *value_out, int precision) {
    CHECK_HANDLE(h);
    if (precision < RMAV_POLICY_FP32 || precision > RMAV_POLICY_F16_SHARED)
        return rmav_fail(RMAV_ERR_INVALID, "precision must be one of RMAV_POLICY_FP32 ... RMAV_POLICY_F16_SHARED (rmav_policy_precision)");
    if (int rc = check_policy_args(n_steps, weights, logp_out, value_out, false, nullptr)) return rc;
    if (h->time_limit > 0)
        if (int rc = need_variants(precision, "a time-limited handle", "time-limited")) return rc;
    return launch_policy_call(h, n_steps, weights, actions_out, obs_out, rew_out, done_out, logp_out, value_out, precision, nullptr, nullptr);
}

int rmav_rollout_policy_boot(rmav_handle h, int32_t n_steps, const float *weights, float *actions_out, float *obs_out, float *rew_out,
                             uint8_t *done_out, float *logp_out, float *value_out, float *boot_out, uint8_t *trunc_out, int precision) {
    CHECK_HANDLE(h);
    if (h->kind == RMAV_REINMAV)
        return rmav_fail(RMAV_ERR_INVALID, "ReinmavEnv takes no time limit: there is no truncated step to bootstrap");
    if (h->time_limit <= 0)
        return rmav_fail(RMAV_ERR_INVALID, "rmav_rollout_policy_boot needs an episode time limit on the handle (rmav_set_time_limit)");
    if (int rc = need_variants(precision, "rmav_rollout_policy_boot", "time-limited")) return rc;
    if (int rc = check_policy_args(n_steps, weights, logp_out, value_out, true, boot_out)) return rc;
    const BootArgs bt{boot_out, trunc_out};
    return launch_policy_call(h, n_steps, weights, actions_out, obs_out, rew_out, done_out, logp_out, value_out, precision, &bt, nullptr);
}

// ---- the action rule of the three entry points above and rmav_rollout_policy_norm: handle state, host only ----------------------------
int rmav_set_policy_action_rule(rmav_handle h, int32_t deterministic, float clip_lo, float clip_hi) {
    CHECK_HANDLE(h);
    if (deterministic != 0 && deterministic != 1) return rmav_fail(RMAV_ERR_INVALID, "deterministic must be 0 or 1, got %d", (int)deterministic);
    if (!(clip_lo <= clip_hi))   // (false for a NaN on either side)
        return rmav_fail(RMAV_ERR_INVALID, "the policy action rule needs clip_lo <= clip_hi, neither NaN (-inf / +inf = no bound), got [%g, %g]",
                         (double)clip_lo, (double)clip_hi);
    h->rule_det = deterministic;
    h->rule_lo = clip_lo;
    h->rule_hi = clip_hi;
    return RMAV_OK;
}

int rmav_get_policy_action_rule(rmav_handle h, int32_t *deterministic, float *clip_lo, float *clip_hi) {
    CHECK_HANDLE(h);
    if (!deterministic || !clip_lo || !clip_hi) return rmav_fail(RMAV_ERR_INVALID, "deterministic, clip_lo and clip_hi are required");
    *deterministic = h->rule_det;
    *clip_lo = h->rule_lo;
    *clip_hi = h->rule_hi;
    return RMAV_OK;
}

// ---- learner-side helpers on the trajectory ----------------------------------------------------
// The one launcher of the GAE family.  with_boot (rmav_gae_boot): k_gae_boot, which adds the bootstrap term `boot` of the truncated steps;
// stats (rmav_gae_norm): k_gae_norm<with_boot>, which normalises every reward as it is loaded (csrc/rmav_ret_norm.hpp)
static int gae_impl(rmav_handle h, int32_t n_steps, const float *rew, const uint8_t *done, const float *values, bool with_boot, const float *boot,
                    const RetNormStats *stats, float gamma, float lam, float reward_scale, float *adv_out, float *ret_out, double *sums_out) {
    if (n_steps <= 0) return rmav_fail(RMAV_ERR_INVALID, "n_steps must be > 0");
    if (!rew || !done || !values || (with_boot && !boot) || !adv_out || !ret_out)
        return rmav_fail(RMAV_ERR_INVALID, with_boot ? "rew, done, values, boot, adv_out and ret_out are required (device pointers)"
                                                     : "rew, done, values, adv_out and ret_out are required (device pointers)");
    const unsigned nblk = (unsigned)((h->n + 255) / 256);
    double *partial = nullptr;
    if (sums_out) {
        if (int rc = ensure_scratch(h, (size_t)nblk * 2 * sizeof(double))) return rc;
        partial = (double *)h->scratch;
    }
    if (stats && with_boot)
        hipLaunchKernelGGL(k_gae_norm<true>, dim3(nblk), dim3(256), 0, h->stream, rew, done, values, boot, stats, adv_out, ret_out, h->n, n_steps,
                           gamma, lam, reward_scale, partial);
    else if (stats)
        hipLaunchKernelGGL(k_gae_norm<false>, dim3(nblk), dim3(256), 0, h->stream, rew, done, values, boot, stats, adv_out, ret_out, h->n, n_steps,
                           gamma, lam, reward_scale, partial);
    else if (with_boot)
        hipLaunchKernelGGL(k_gae_boot, dim3(nblk), dim3(256), 0, h->stream, rew, done, values, boot, adv_out, ret_out, h->n, n_steps, gamma, lam,
                           reward_scale, partial);
    else
        hipLaunchKernelGGL(k_gae, dim3(nblk), dim3(256), 0, h->stream, rew, done, values, adv_out, ret_out, h->n, n_steps, gamma, lam, reward_scale,
                           partial);
    HIP_TRY(hipGetLastError());
    if (sums_out) {
        hipLaunchKernelGGL(k_gae_fold, dim3(1), dim3(256), 0, h->stream, (const double *)partial, (int)nblk, sums_out);
        HIP_TRY(hipGetLastError());
    }
    return RMAV_OK;
}

int rmav_gae(rmav_handle h, int32_t n_steps, const float *rew, const uint8_t *done, const float *values,
             float gamma, float lam, float reward_scale, float *adv_out, float *ret_out, double *sums_out) {
    CHECK_HANDLE(h);
    return gae_impl(h, n_steps, rew, done, values, false, nullptr, nullptr, gamma, lam, reward_scale, adv_out, ret_out, sums_out);
}

int rmav_gae_boot(rmav_handle h, int32_t n_steps, const float *rew, const uint8_t *done, const float *values, const float *boot,
                  float gamma, float lam, float reward_scale, float *adv_out, float *ret_out, double *sums_out) {
    CHECK_HANDLE(h);
    if (h->kind == RMAV_REINMAV)
        return rmav_fail(RMAV_ERR_INVALID, "ReinmavEnv takes no time limit: there is no truncated step to bootstrap (use rmav_gae)");
    return gae_impl(h, n_steps, rew, done, values, true, boot, nullptr, gamma, lam, reward_scale, adv_out, ret_out, sums_out);
}

int rmav_normalize(rmav_handle h, float *x, int64_t count, float mean, float rstd) {
    CHECK_HANDLE(h);
    if (!x || count < 0) return rmav_fail(RMAV_ERR_INVALID, "x is NULL or count < 0");
    if ((reinterpret_cast<uintptr_t>(x) & 15u) != 0) return rmav_fail(RMAV_ERR_INVALID, "x must be 16-byte aligned");
    if (count == 0) return RMAV_OK;
    int64_t blocks = (count / 4 + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 4096) blocks = 4096;   // grid-stride: 16 blocks per CU keep the memory system full
    hipLaunchKernelGGL(k_affine, dim3((unsigned)blocks), dim3(256), 0, h->stream, x, count, mean, rstd);
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

// ---- observation normalisation (VecNormalize): running statistics on the device, csrc/rmav_obs_norm.hpp ------------------
// the settings both _init entry points take (observation and return statistics)
static int check_norm_settings(float clip, double eps, double count0) {
    if (!(clip > 0.0f) || !(eps >= 0.0) || !(count0 > 0.0) || eps - eps != 0.0 || count0 - count0 != 0.0)
        return rmav_fail(RMAV_ERR_INVALID, "clip must be > 0 (+inf = no clip), eps finite and >= 0, count0 finite and > 0");
    return RMAV_OK;
}
namespace {
int check_norm_handle(rmav_handle h, const char *what) {
    if (h->kind == RMAV_REINMAV) return rmav_fail(RMAV_ERR_INVALID, "%s runs the four quadrotor kinds, not RMAV_REINMAV", what);
    return RMAV_OK;
}
// a statistics buffer of either normaliser; bytes_fn = the function that gives its size
int check_stats(const void *stats, const char *bytes_fn) {
    if (!stats) return rmav_fail(RMAV_ERR_INVALID, "stats is NULL (a device buffer of %s() bytes)", bytes_fn);
    if ((reinterpret_cast<uintptr_t>(stats) & 15u) != 0) return rmav_fail(RMAV_ERR_INVALID, "stats must be 16-byte aligned");
    return RMAV_OK;
}
// the addressing of an observation array (ObsShape); n_rows >= 1 checked by the caller
int obs_shape(rmav_handle h, int layout, int32_t n_rows, int64_t pitch, ObsShape &sh) {
    const int ns = kStateDim[h->kind];
    if (layout != RMAV_SOA && layout != RMAV_AOS) return rmav_fail(RMAV_ERR_INVALID, "layout must be RMAV_SOA or RMAV_AOS");
    if (layout == RMAV_SOA) {
        if (pitch == 0) pitch = h->n;
        if (pitch < h->n || pitch > (int64_t)0x3fffffff) return rmav_fail(RMAV_ERR_INVALID, "pitch must be 0 (= N) or in [N, 2^30)");
        sh = ObsShape{h->n, (int64_t)ns * pitch, pitch, 1, n_rows, ns};
    } else {
        if (pitch != 0) return rmav_fail(RMAV_ERR_INVALID, "pitch must be 0 with RMAV_AOS");
        sh = ObsShape{h->n, h->n * ns, 1, ns, n_rows, ns};
    }
    return RMAV_OK;
}
}  // namespace

int64_t rmav_obs_norm_bytes(void) { return (int64_t)sizeof(ObsNormStats); }

int rmav_obs_norm_init(rmav_handle h, void *stats, float clip, double eps, double count0) {
    CHECK_HANDLE(h);
    if (int rc = check_norm_handle(h, "rmav_obs_norm_init")) return rc;
    if (int rc = check_stats(stats, "rmav_obs_norm_bytes")) return rc;
    if (int rc = check_norm_settings(clip, eps, count0)) return rc;
    hipLaunchKernelGGL(k_obs_norm_init, dim3(1), dim3(64), 0, h->stream, (ObsNormStats *)stats, (int32_t)kStateDim[h->kind], clip, eps, count0);
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

int rmav_obs_moments(rmav_handle h, const float *obs, int layout, int32_t n_rows, int64_t pitch, double *batch_out) {
    CHECK_HANDLE(h);
    if (int rc = check_norm_handle(h, "rmav_obs_moments")) return rc;
    if (!obs || !batch_out) return rmav_fail(RMAV_ERR_INVALID, "obs and batch_out are required (device pointers)");
    if (n_rows < 0) return rmav_fail(RMAV_ERR_INVALID, "n_rows must be >= 0");
    ObsShape sh;
    if (int rc = obs_shape(h, layout, n_rows > 0 ? n_rows : 1, pitch, sh)) return rc;
    sh.n_rows = n_rows;   // 0 rows: an empty record (count 0), which rmav_obs_norm_merge skips
    const bool vec = layout == RMAV_SOA && (reinterpret_cast<uintptr_t>(obs) & 15u) == 0 && (sh.feat & 3) == 0;
    const int64_t cols = vec ? (sh.n + 3) / 4 : sh.n;
    const int64_t xenv = (cols + 255) / 256;
    // enough blocks for 256 CUs (8 per CU) when the rows allow it; a thread then walks every rgroups-th row
    int64_t rgroups = (2048 + xenv * sh.ns - 1) / (xenv * sh.ns);
    if (rgroups > n_rows) rgroups = n_rows;
    if (rgroups < 1) rgroups = 1;
    const int64_t nblk = xenv * rgroups;
    if (int rc = ensure_scratch(h, (size_t)nblk * sh.ns * sizeof(Moment))) return rc;
    const dim3 grid((unsigned)nblk, (unsigned)sh.ns);
    if (vec) hipLaunchKernelGGL(k_obs_moments<true>, grid, dim3(256), 0, h->stream, obs, sh, (int32_t)xenv, (int32_t)rgroups, (Moment *)h->scratch);
    else hipLaunchKernelGGL(k_obs_moments<false>, grid, dim3(256), 0, h->stream, obs, sh, (int32_t)xenv, (int32_t)rgroups, (Moment *)h->scratch);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_obs_moments_fold, dim3(kNormFeat), dim3(256), 0, h->stream, (const Moment *)h->scratch, (int32_t)nblk, (int32_t)sh.ns, batch_out);
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

int rmav_obs_norm_merge(rmav_handle h, void *stats, const double *batch, int32_t n_batches) {
    CHECK_HANDLE(h);
    if (int rc = check_norm_handle(h, "rmav_obs_norm_merge")) return rc;
    if (int rc = check_stats(stats, "rmav_obs_norm_bytes")) return rc;
    if (n_batches < 0) return rmav_fail(RMAV_ERR_INVALID, "n_batches must be >= 0");
    if (n_batches == 0) return RMAV_OK;
    if (!batch) return rmav_fail(RMAV_ERR_INVALID, "batch is NULL (n_batches records of 33 doubles on the device)");
    hipLaunchKernelGGL(k_obs_norm_merge, dim3(1), dim3(64), 0, h->stream, (ObsNormStats *)stats, batch, n_batches, (int32_t)kStateDim[h->kind]);
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

int rmav_obs_normalize(rmav_handle h, const void *stats, const float *in, float *out, int layout, int32_t n_rows, int64_t pitch) {
    CHECK_HANDLE(h);
    if (int rc = check_norm_handle(h, "rmav_obs_normalize")) return rc;
    if (int rc = check_stats(stats, "rmav_obs_norm_bytes")) return rc;
    if (n_rows < 0) return rmav_fail(RMAV_ERR_INVALID, "n_rows must be >= 0");
    if (n_rows == 0) return RMAV_OK;
    if (!in || !out) return rmav_fail(RMAV_ERR_INVALID, "in and out are required (device pointers; out == in is allowed)");
    ObsShape sh;
    if (int rc = obs_shape(h, layout, n_rows, pitch, sh)) return rc;
    const int64_t total = sh.n * sh.ns * (int64_t)n_rows;
    if ((total + 255) / 256 > (int64_t)0x7fffffff) return rmav_fail(RMAV_ERR_INVALID, "too many elements for one launch");
    hipLaunchKernelGGL(k_obs_normalize, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, (const ObsNormStats *)stats, in, out, sh);
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

int rmav_rollout_policy_norm(rmav_handle h, int32_t n_steps, const float *weights, const void *stats, float *actions_out, float *obs_out,
                             float *rew_out, uint8_t *done_out, float *logp_out, float *value_out, float *boot_out, uint8_t *trunc_out,
                             int precision) {
    CHECK_HANDLE(h);
    if (int rc = check_norm_handle(h, "rmav_rollout_policy_norm")) return rc;
    if (int rc = need_variants(precision, "rmav_rollout_policy_norm", "normalised")) return rc;
    if (int rc = check_stats(stats, "rmav_obs_norm_bytes")) return rc;
    if (int rc = check_policy_args(n_steps, weights, logp_out, value_out, false, nullptr)) return rc;
    if (h->time_limit > 0 && !boot_out)
        return rmav_fail(RMAV_ERR_INVALID, "boot_out is required on a handle with an episode time limit (as rmav_rollout_policy_boot)");
    if (h->time_limit <= 0 && (boot_out || trunc_out))
        return rmav_fail(RMAV_ERR_INVALID, "boot_out / trunc_out need an episode time limit on the handle (rmav_set_time_limit); pass NULL");
    const BootArgs bt{boot_out, trunc_out};
    const NormArgs nm{((const ObsNormStats *)stats)->mean_f};
    return launch_policy_call(h, n_steps, weights, actions_out, obs_out, rew_out, done_out, logp_out, value_out, precision, &bt, &nm);
}

// ---- return normalisation (the reward half of VecNormalize): one scalar RunningMeanStd on the device, csrc/rmav_ret_norm.hpp -----------
int64_t rmav_ret_norm_bytes(void) { return (int64_t)sizeof(RetNormStats); }

int rmav_ret_norm_init(rmav_handle h, void *stats, float clip, double eps, double count0) {
    CHECK_HANDLE(h);
    if (int rc = check_stats(stats, "rmav_ret_norm_bytes")) return rc;
    if (int rc = check_norm_settings(clip, eps, count0)) return rc;
    hipLaunchKernelGGL(k_ret_norm_init, dim3(1), dim3(64), 0, h->stream, (RetNormStats *)stats, clip, eps, count0);
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

int rmav_ret_moments(rmav_handle h, int32_t n_steps, const float *rew, const uint8_t *done, float reward_scale, float gamma, float *carry,
                     double *batch_out) {
    CHECK_HANDLE(h);
    if (n_steps < 0) return rmav_fail(RMAV_ERR_INVALID, "n_steps must be >= 0");
    if (!batch_out) return rmav_fail(RMAV_ERR_INVALID, "batch_out is required (3 doubles on the device)");
    if (n_steps > 0 && (!rew || !done || !carry)) return rmav_fail(RMAV_ERR_INVALID, "rew, done and carry are required (device pointers)");
    const unsigned nblk = n_steps > 0 ? (unsigned)((h->n + 255) / 256) : 0u;   // 0 steps: an empty record, carry untouched
    if (nblk) {
        if (int rc = ensure_scratch(h, (size_t)nblk * sizeof(Moment))) return rc;
        hipLaunchKernelGGL(k_ret_moments, dim3(nblk), dim3(256), 0, h->stream, rew, done, carry, h->n, n_steps, reward_scale, gamma,
                           (Moment *)h->scratch);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_ret_moments_fold, dim3(1), dim3(256), 0, h->stream, (const Moment *)h->scratch, (int32_t)nblk, batch_out);
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

int rmav_ret_norm_merge(rmav_handle h, void *stats, const double *batch, int32_t n_batches) {
    CHECK_HANDLE(h);
    if (int rc = check_stats(stats, "rmav_ret_norm_bytes")) return rc;
    if (n_batches < 0) return rmav_fail(RMAV_ERR_INVALID, "n_batches must be >= 0");
    if (n_batches == 0) return RMAV_OK;
    if (!batch) return rmav_fail(RMAV_ERR_INVALID, "batch is NULL (n_batches records of 3 doubles on the device)");
    hipLaunchKernelGGL(k_ret_norm_merge, dim3(1), dim3(64), 0, h->stream, (RetNormStats *)stats, batch, n_batches);
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

int rmav_ret_normalize(rmav_handle h, const void *stats, const float *in, float *out, int64_t count, float reward_scale) {
    CHECK_HANDLE(h);
    if (int rc = check_stats(stats, "rmav_ret_norm_bytes")) return rc;
    if (count < 0) return rmav_fail(RMAV_ERR_INVALID, "count must be >= 0");
    if (count == 0) return RMAV_OK;
    if (!in || !out) return rmav_fail(RMAV_ERR_INVALID, "in and out are required (device pointers; out == in is allowed)");
    if ((count + 255) / 256 > (int64_t)0x7fffffff) return rmav_fail(RMAV_ERR_INVALID, "too many elements for one launch");
    hipLaunchKernelGGL(k_ret_normalize, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream, (const RetNormStats *)stats, in, out, count,
                       reward_scale);
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

int rmav_gae_norm(rmav_handle h, int32_t n_steps, const float *rew, const uint8_t *done, const float *values, const float *boot,
                  const void *stats, float gamma, float lam, float reward_scale, float *adv_out, float *ret_out, double *sums_out) {
    CHECK_HANDLE(h);
    if (boot && h->kind == RMAV_REINMAV)
        return rmav_fail(RMAV_ERR_INVALID, "ReinmavEnv takes no time limit: there is no truncated step to bootstrap (pass boot = NULL)");
    if (int rc = check_stats(stats, "rmav_ret_norm_bytes")) return rc;
    return gae_impl(h, n_steps, rew, done, values, boot != nullptr, boot, (const RetNormStats *)stats, gamma, lam, reward_scale, adv_out, ret_out,
                    sums_out);
}

// ---- the fused learners: loss and gradient of one PPO minibatch, csrc/rmav_learner.hpp (value_network="copy": one launch per net) and
// csrc/rmav_learner_shared.hpp ("shared": one launch; on the matrix cores: csrc/rmav_learner_mfma.hpp), then the one fold ----------------------------------------------------------------
// The flat gradient of either learner (the ABI order of include/rmav_ppo.h): n tensors, their offsets, the total in off[n]; logstd is last
struct FlatLayout {
    int32_t n;
    int32_t off[kLrnParams + 1];
};
static FlatLayout flat_layout(bool shared, int ns, int na) {
    const int copy[kLrnParams] = {64 * ns, 64, 64 * 64, 64, na * 64, na, 64 * ns, 64, 64 * 64, 64, 64, 1, na};
    const int trunk[kTrkParams] = {64 * ns, 64, 64 * 64, 64, na * 64, na, 64, 1, na};
    FlatLayout L;
    L.n = shared ? kTrkParams : kLrnParams;
    L.off[0] = 0;
    for (int k = 0; k < L.n; ++k) L.off[k + 1] = L.off[k] + (shared ? trunk : copy)[k];
    return L;
}
static int64_t grad_param_count(bool shared, int kind) {
    if (kind < 0 || kind >= kNumKinds) return -1;
    const FlatLayout lay = flat_layout(shared, kStateDim[kind], kActionDim[kind]);
    return lay.off[lay.n];
}
// (matrix: the shared-trunk learner on the matrix cores, csrc/rmav_learner_mfma.hpp - another net kernel with a geometry of its own)
static int grad_groups(bool matrix, int64_t batch) { return matrix ? matrix_groups(batch) : learner_groups(batch); }
static int64_t grad_workspace_bytes(bool shared, int kind, int64_t batch, bool matrix = false) {
    if (kind < 0 || kind >= kNumKinds || batch < 1) return -1;
    return (int64_t)grad_groups(matrix, batch) * (grad_param_count(shared, kind) + kLrnStats) * (int64_t)sizeof(float);
}

static int ppo_grad_impl(rmav_handle h, bool shared, bool matrix, int64_t batch, const int64_t *idx, const float *obs, int64_t obs_pitch, const float *act,
                         int64_t act_pitch, const float *logp_old, const float *val_old, const float *adv, const float *ret,
                         const float *adv_norm, const float *const *params, const void *obs_stats, const rmav_ppo_grad_spec *spec,
                         void *workspace, float *grad_out, float *stats_out) {
    CHECK_HANDLE(h);
    if (batch < 1 || batch > (int64_t)0x7fffffff) return rmav_fail(RMAV_ERR_INVALID, "batch must be in [1, 2^31), got %lld", (long long)batch);
    const struct {
        const void *p;
        const char *name;
    } need[] = {{obs, "obs"}, {act, "act"}, {logp_old, "logp_old"}, {val_old, "val_old"}, {adv, "adv"}, {ret, "ret"}, {adv_norm, "adv_norm"},
                {params, "params"}, {spec, "spec"}, {workspace, "workspace"}, {grad_out, "grad_out"}, {stats_out, "stats_out"}};
    for (const auto &n : need)
        if (!n.p) return rmav_fail(RMAV_ERR_INVALID, "%s is NULL (required)", n.name);
    const int32_t ns = kStateDim[h->kind], na = kActionDim[h->kind];
    const FlatLayout lay = flat_layout(shared, ns, na);
    for (int k = 0; k < lay.n; ++k)
        if (!params[k])
            return rmav_fail(RMAV_ERR_INVALID, shared ? "params[%d] is NULL (9 device pointers: pi W1 b1 W2 b2 W3 b3, vf W b, logstd)"
                                                      : "params[%d] is NULL (13 device pointers: pi W1 b1 W2 b2 W3 b3, vf the same, logstd)", k);
    const int64_t min_pitch = idx ? 1 : batch;
    if (obs_pitch < min_pitch) return rmav_fail(RMAV_ERR_INVALID, "obs_pitch must be >= %lld, got %lld", (long long)min_pitch, (long long)obs_pitch);
    if (act_pitch < min_pitch) return rmav_fail(RMAV_ERR_INVALID, "act_pitch must be >= %lld, got %lld", (long long)min_pitch, (long long)act_pitch);
    if (spec->clip - spec->clip != 0.0f || spec->clip < 0.0f) return rmav_fail(RMAV_ERR_INVALID, "clip must be finite and >= 0, got %g", (double)spec->clip);
    if (spec->vf_coef - spec->vf_coef != 0.0f) return rmav_fail(RMAV_ERR_INVALID, "vf_coef must be finite, got %g", (double)spec->vf_coef);
    if (spec->ent_coef - spec->ent_coef != 0.0f) return rmav_fail(RMAV_ERR_INVALID, "ent_coef must be finite, got %g", (double)spec->ent_coef);
    if ((reinterpret_cast<uintptr_t>(workspace) & 15u) != 0) return rmav_fail(RMAV_ERR_INVALID, "workspace must be 16-byte aligned");
    if (obs_stats && (reinterpret_cast<uintptr_t>(obs_stats) & 15u) != 0) return rmav_fail(RMAV_ERR_INVALID, "obs_stats must be 16-byte aligned");
    const auto fill = [&](auto &a) {   // the fields LearnerArgs and TrunkArgs have in common
        memset(&a, 0, sizeof(a));
        a.idx = idx;
        a.obs = obs;
        a.act = act;
        a.obs_pitch = obs_pitch;
        a.act_pitch = act_pitch;
        a.logp_old = logp_old;
        a.val_old = val_old;
        a.adv = adv;
        a.ret = ret;
        a.adv_norm = adv_norm;
        a.norm_tab = obs_stats ? ((const ObsNormStats *)obs_stats)->mean_f : nullptr;
        a.partial = (float *)workspace;
        a.clip = spec->clip;
        a.vf_coef = spec->vf_coef;
        a.batch = (int32_t)batch;
        a.ns = ns;
        a.na = na;
    };
    const int32_t n_params = lay.off[lay.n], off_logstd = lay.off[lay.n - 1], pstride = n_params + kLrnStats;
    const float *logstd = params[lay.n - 1];
    const dim3 grid((unsigned)grad_groups(matrix, batch));   // (kind, batch) alone decide the geometry
    if (shared) {
        TrunkArgs a;
        fill(a);
        for (int k = 0; k < kTrkParams; ++k) a.p[k] = params[k];
        if (matrix) hipLaunchKernelGGL(k_matrix_grad, grid, dim3(kMatThreads), 0, h->stream, a);
        else hipLaunchKernelGGL(k_trunk_grad, grid, dim3(kLrnThreads), 0, h->stream, a);
        HIP_TRY(hipGetLastError());
    } else {
        LearnerArgs a;
        fill(a);
        a.pstride = pstride;
        a.logstd = logstd;
        a.off_logstd = off_logstd;
        a.off_stats = n_params;
        for (int net = 0; net < 2; ++net) {
            for (int k = 0; k < 6; ++k) {
                a.p[k] = params[6 * net + k];
                a.goff[k] = lay.off[6 * net + k];
            }
            if (net == 0) hipLaunchKernelGGL(k_learner_grad<false>, grid, dim3(kLrnThreads), 0, h->stream, a);
            else hipLaunchKernelGGL(k_learner_grad<true>, grid, dim3(kLrnThreads), 0, h->stream, a);
            HIP_TRY(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(k_learner_fold, dim3((unsigned)((n_params + 255) / 256)), dim3(256), 0, h->stream, (const float *)workspace, (int32_t)grid.x,
                       pstride, n_params, off_logstd, na, (int32_t)batch, spec->vf_coef, spec->ent_coef, logstd, grad_out, stats_out);
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

int64_t rmav_ppo_grad_param_count(int kind) { return grad_param_count(false, kind); }
int64_t rmav_ppo_grad_workspace_bytes(int kind, int64_t batch) { return grad_workspace_bytes(false, kind, batch); }
int64_t rmav_ppo_grad_shared_param_count(int kind) { return grad_param_count(true, kind); }
int64_t rmav_ppo_grad_shared_workspace_bytes(int kind, int64_t batch) { return grad_workspace_bytes(true, kind, batch); }
int64_t rmav_ppo_grad_shared_mfma_workspace_bytes(int kind, int64_t batch) { return grad_workspace_bytes(true, kind, batch, true); }

int rmav_ppo_grad(rmav_handle h, int64_t batch, const int64_t *idx, const float *obs, int64_t obs_pitch, const float *act, int64_t act_pitch,
                  const float *logp_old, const float *val_old, const float *adv, const float *ret, const float *adv_norm,
                  const float *const *params, const void *obs_stats, const rmav_ppo_grad_spec *spec, void *workspace, float *grad_out,
                  float *stats_out) {
    return ppo_grad_impl(h, false, false, batch, idx, obs, obs_pitch, act, act_pitch, logp_old, val_old, adv, ret, adv_norm, params, obs_stats, spec,
                         workspace, grad_out, stats_out);
}
int rmav_ppo_grad_shared(rmav_handle h, int64_t batch, const int64_t *idx, const float *obs, int64_t obs_pitch, const float *act,
                         int64_t act_pitch, const float *logp_old, const float *val_old, const float *adv, const float *ret,
                         const float *adv_norm, const float *const *params, const void *obs_stats, const rmav_ppo_grad_spec *spec,
                         void *workspace, float *grad_out, float *stats_out) {
    return ppo_grad_impl(h, true, false, batch, idx, obs, obs_pitch, act, act_pitch, logp_old, val_old, adv, ret, adv_norm, params, obs_stats, spec,
                         workspace, grad_out, stats_out);
}
int rmav_ppo_grad_shared_mfma(rmav_handle h, int64_t batch, const int64_t *idx, const float *obs, int64_t obs_pitch, const float *act,
                              int64_t act_pitch, const float *logp_old, const float *val_old, const float *adv, const float *ret,
                              const float *adv_norm, const float *const *params, const void *obs_stats, const rmav_ppo_grad_spec *spec,
                              void *workspace, float *grad_out, float *stats_out) {
    return ppo_grad_impl(h, true, true, batch, idx, obs, obs_pitch, act, act_pitch, logp_old, val_old, adv, ret, adv_norm, params, obs_stats, spec,
                         workspace, grad_out, stats_out);
}

// ---- around the fused learner: the advantage moments it takes and the optimiser step on its gradient, csrc/rmav_optim.hpp ----------------
int64_t rmav_adv_moments_workspace_bytes(int64_t batch) {
    if (batch < 1) return -1;
    return (int64_t)adv_groups(batch) * (int64_t)sizeof(Moment);
}

int rmav_adv_moments(rmav_handle h, int64_t batch, const int64_t *idx, const float *adv, void *workspace, float *adv_norm_out) {
    CHECK_HANDLE(h);
    if (batch < 1) return rmav_fail(RMAV_ERR_INVALID, "batch must be >= 1, got %lld", (long long)batch);
    if (!adv) return rmav_fail(RMAV_ERR_INVALID, "adv is NULL (required)");
    if (!workspace) return rmav_fail(RMAV_ERR_INVALID, "workspace is NULL (required)");
    if (!adv_norm_out) return rmav_fail(RMAV_ERR_INVALID, "adv_norm_out is NULL (required)");
    if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) return rmav_fail(RMAV_ERR_INVALID, "workspace must be 8-byte aligned");
    const int groups = adv_groups(batch);   // batch alone decides the geometry
    hipLaunchKernelGGL(k_adv_moments, dim3((unsigned)groups), dim3(256), 0, h->stream, idx, adv, batch, (Moment *)workspace);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_adv_moments_fold, dim3(1), dim3(256), 0, h->stream, (const Moment *)workspace, (int32_t)groups, batch, adv_norm_out);
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

int rmav_ppo_adam(rmav_handle h, int shared, const float *grad, float *const *params, float *exp_avg, float *exp_avg_sq, int64_t step,
                  const rmav_ppo_adam_spec *spec, float *stats_out) {
    CHECK_HANDLE(h);
    if (shared != 0 && shared != 1) return rmav_fail(RMAV_ERR_INVALID, "shared must be 0 or 1, got %d", shared);
    const struct {
        const void *p;
        const char *name;
    } need[] = {{grad, "grad"}, {params, "params"}, {exp_avg, "exp_avg"}, {exp_avg_sq, "exp_avg_sq"}, {spec, "spec"}};
    for (const auto &n : need)
        if (!n.p) return rmav_fail(RMAV_ERR_INVALID, "%s is NULL (required)", n.name);
    const FlatLayout lay = flat_layout(shared != 0, kStateDim[h->kind], kActionDim[h->kind]);
    const int n_tensors = lay.n;
    for (int k = 0; k < n_tensors; ++k)
        if (!params[k]) return rmav_fail(RMAV_ERR_INVALID, "params[%d] is NULL (%d device pointers, in the order of %s)", k, n_tensors,
                                         shared ? "rmav_ppo_grad_shared" : "rmav_ppo_grad");
    if (step < 1) return rmav_fail(RMAV_ERR_INVALID, "step must be >= 1 (the number of this update), got %lld", (long long)step);
    const auto finite = [](float x) { return x - x == 0.0f; };
    if (!finite(spec->lr) || spec->lr < 0.0f) return rmav_fail(RMAV_ERR_INVALID, "lr must be finite and >= 0, got %g", (double)spec->lr);
    if (!(spec->beta1 >= 0.0f && spec->beta1 < 1.0f)) return rmav_fail(RMAV_ERR_INVALID, "beta1 must be in [0, 1), got %g", (double)spec->beta1);
    if (!(spec->beta2 >= 0.0f && spec->beta2 < 1.0f)) return rmav_fail(RMAV_ERR_INVALID, "beta2 must be in [0, 1), got %g", (double)spec->beta2);
    if (!finite(spec->eps) || spec->eps < 0.0f) return rmav_fail(RMAV_ERR_INVALID, "eps must be finite and >= 0, got %g", (double)spec->eps);
    if (!(spec->max_grad_norm > 0.0f))   // (false for a NaN)
        return rmav_fail(RMAV_ERR_INVALID, "max_grad_norm must be > 0 (+inf = no clip), got %g", (double)spec->max_grad_norm);
    if (!finite(spec->grad_scale) || !(spec->grad_scale > 0.0f))
        return rmav_fail(RMAV_ERR_INVALID, "grad_scale must be finite and > 0, got %g", (double)spec->grad_scale);
    if (spec->_reserved[0] != 0 || spec->_reserved[1] != 0) return rmav_fail(RMAV_ERR_INVALID, "_reserved must be 0");
    AdamArgs a;
    memset(&a, 0, sizeof(a));
    for (int k = 0; k < kAdamMaxTensors; ++k) {
        a.p[k] = k < n_tensors ? params[k] : nullptr;
        a.off[k] = k < n_tensors ? lay.off[k] : 0x7fffffff;
    }
    a.n = lay.off[n_tensors];
    a.grad = grad;
    a.m = exp_avg;
    a.v = exp_avg_sq;
    a.stats = stats_out;
    a.grad_scale = spec->grad_scale;
    a.max_norm = spec->max_grad_norm;
    a.omb1 = 1.0f - spec->beta1;
    a.beta2 = spec->beta2;
    a.omb2 = 1.0f - spec->beta2;
    // the two bias corrections: fp64 from the fp32 hyperparameters, each scalar rounded to fp32 once
    const double bc1 = 1.0 - pow((double)spec->beta1, (double)step), bc2 = 1.0 - pow((double)spec->beta2, (double)step);
    a.step_size = (float)((double)spec->lr / bc1);
    a.bc2_sqrt = (float)sqrt(bc2);
    a.eps = spec->eps;
    hipLaunchKernelGGL(k_ppo_adam, dim3(1), dim3(kAdamThreads), 0, h->stream, a);
    HIP_TRY(hipGetLastError());
    return RMAV_OK;
}

}  // extern "C"

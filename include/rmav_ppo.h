/* rmav_ppo.h - the PPO2 rollout loop behind the boundary: baselines ppo2 Runner.run() = model.step(obs) ->
 * env.step(actions) (gym_reinmav/run.py:63-68) as ONE fused launch with the policy inside the kernel, and the learner-side passes (GAE).
 * Part of the C ABI of librmav.so; included by rmav.h (conventions, rmav_handle, status codes: there). */
#ifndef RMAV_PPO_H
#define RMAV_PPO_H

#include "rmav.h"

#ifdef __cplusplus
extern "C" {
#endif

enum rmav_policy_precision {
    RMAV_POLICY_FP32 = 0,       /* fp32 FMAs on the vector ALU */
    RMAV_POLICY_BF16_MFMA = 1,  /* bf16 operands, fp32 accumulate on the matrix cores */
    RMAV_POLICY_FP32_MFMA = 2,  /* fp32 operands and accumulate on the fp32-input matrix instructions: same precision
                                   class as RMAV_POLICY_FP32 (only the summation order differs), ~2x its speed */
    RMAV_POLICY_F16_MFMA = 3,   /* f16 operands (11-bit mantissa), fp32 accumulate, tanh folded into the next layer's weights
                                   (csrc/rmav_policy_pair.hpp): ~8x closer to the fp32 policy than bf16 and faster.
                                   Weight buffer: rmav_pack_policy_f16 */
    RMAV_POLICY_F16_SHARED = 4  /* a DIFFERENT architecture, same arithmetic as RMAV_POLICY_F16_MFMA: ONE 2x64 tanh trunk with a mean head
                                   and a scalar value head on its latent - baselines' value_network = 'shared', what ppo2 builds for an env
                                   type without a defaults entry (the native envs of gym_reinmav: env_type 'native'); the other precisions
                                   evaluate a policy net and a separate value net (value_network = 'copy', baselines' MuJoCo default).
                                   Weight buffer: rmav_policy_weight_count_shared() floats = ONE net of the bf16 fragment layout with
                                   output rows 0..3 = the mean head, row 4 = the value head, then logstd [4]; built by rmav_pack_policy_f16 */
};

/* PPO2-style rollout with the policy inside the kernel (the caller loop of gym_reinmav/run.py:63-68:
 * baselines ppo2 Runner = model.step(obs) -> env.step(actions), network='mlp').  Policy: two 64-unit tanh
 * layers -> Gaussian mean (state-independent log-std), plus a value net of the same shape.  All pointers
 * are DEVICE pointers, layout is SoA, nothing synchronises (capturable in a hipGraph).
 * weights: rmav_policy_weight_count(kind) floats, 16-byte aligned, layout (H = 64, NSP = nS rounded up
 *   to a multiple of 4), policy net then value net, each:
 *     W1 [H][NSP] (row = hidden unit, zero padded) | b1 [H] | W2T [H][H] (W2T[i][j] = W2[j][i]) | b2 [H] |
 *     W3T [H][4] (W3T[j][k] = W3[k][j], zero padded to 4 outputs) | b3 [4]
 *   then logstd [4] (zero padded).
 * Per step t: a = mean(obs_t) + exp(logstd) * z_t with z_t standard normal from the counter RNG
 * (stream tag 3, Box-Muller; see csrc/rmav_policy.hpp), logp_out[t] = log N(a; mean, std),
 * value_out[t] = V(obs_t); value_out[n_steps] = V(obs after the last step) for bootstrapping.
 * actions_out [n_steps][nA][N], obs_out [n_steps][nS][N], rew_out / done_out [n_steps][N] may be NULL.
 * precision = RMAV_POLICY_BF16_MFMA evaluates the same two nets with v_mfma_f32_32x32x16_bf16 (bf16
 * weights and activations, fp32 accumulation; means / values within ~1e-2 of the fp32 policy).  Its weight
 * buffer is rmav_policy_weight_count_bf16() floats of pre-arranged MFMA fragments: per net
 *   A1 [2][64 lanes][8 bf16] | A2 [2][4][64][8] | A3 [4][64][8] | b1 [64] | b2 [64] | b3 [32] (fp32)
 * then logstd [4]; fragment (.., lane = (m = lane & 31, h = lane >> 5), j) holds
 *   layer 1: W1p[32 Mt + m][8 h + j]              (W1 zero-padded to 16 inputs)
 *   layer 2: W2 [32 Mt + m][rowmap(s, h, j)]
 *   layer 3: W3p[m][rowmap(s, h, j)]               (W3 zero-padded to 32 outputs)
 *   rowmap(s, h, j) = 32 (s >> 1) + (r & 3) + 8 (r >> 2) + 4 h,  r = 8 (s & 1) + j
 * (csrc/rmav_policy_mfma.hpp explains why; gym_reinmav_amd.ppo.pack_policy_weights_bf16 builds it). */
int64_t rmav_policy_weight_count(int kind);
int64_t rmav_policy_weight_count_bf16(void);
/* RMAV_POLICY_FP32_MFMA: rmav_policy_weight_count_f32_mfma() floats of pre-arranged A operands of
 * v_mfma_f32_32x32x2_f32, per net (policy, then value):
 *   A1 [2 T][2 sq][64 lanes][4]          lane (m, h), entry j: W1p[32 T + m][2 (4 sq + j) + h]   (W1 zero-padded to 16 inputs)
 *   A2 [2 To][2 Tin][4 rq][64 lanes][4]  lane (m, h), entry j: W2[32 To + m][32 Tin + row(4 rq + j, h)]
 *   W3 [2 h][4 outputs][32]              entry 16 Tin + r:      W3p[o][32 Tin + row(r, h)]        (W3 zero-padded to 4 outputs)
 *   b1 [64] | b2 [64] | b3 [4]
 * then logstd [4];  row(r, h) = (r & 3) + 8 (r >> 2) + 4 h  (csrc/rmav_policy_mfma32.hpp explains why;
 * gym_reinmav_amd.ppo.pack_policy_weights_f32_mfma builds it). */
int64_t rmav_policy_weight_count_f32_mfma(void);
int64_t rmav_policy_weight_count_shared(void);   /* RMAV_POLICY_F16_SHARED */
/* Builds such a weight buffer on the device in ONE launch on the handle's stream: with `flat` = the concatenation of the
 * n_params (<= 16) parameter tensors `params[k]` (DEVICE pointers in a HOST array; sizes[k] elements each) followed by zeros,
 * weights_out[i] = flat[idx_lo[i]] when idx_hi[i] < 0, else the two bf16 roundings of flat[idx_lo[i]] (low half) and
 * flat[idx_hi[i]] (high half) in one 32-bit word.  idx_lo / idx_hi: int32 [n_out] on the DEVICE - the fixed permutation of a
 * layout above (gym_reinmav_amd.ppo._PolicyPacker builds them once).  Replaces the chain of small tensor operations a
 * learner would otherwise run before every rollout (baselines: model.step reads the live variables; here the actor's copy
 * is re-derived from the learner's parameters). */
int rmav_pack_policy(rmav_handle h, int n_params, const float *const *params, const int64_t *sizes, const int32_t *idx_lo,
                     const int32_t *idx_hi, int64_t n_out, float *weights_out);
/* RMAV_POLICY_F16_MFMA: the bf16 layout above with f16 pairs in the fragment words (same idx_lo / idx_hi maps, n_out =
 * rmav_policy_weight_count_bf16()), and the fragments of layers 2 and 3 pre-multiplied (in fp32, before the one rounding to
 * f16) by -2 k and -2, k = 2 log2(e): the kernel hands r = 1 / (1 + e^(2z)) = (1 - tanh z) / 2 to the next layer instead of
 * tanh z and derives the matching biases b' = b + rowsum(W) from these rounded weights when it stages them
 * (gym_reinmav_amd.ppo.pack_policy_weights_f16 is the torch form of the same buffer). */
int rmav_pack_policy_f16(rmav_handle h, int n_params, const float *const *params, const int64_t *sizes, const int32_t *idx_lo,
                         const int32_t *idx_hi, int64_t n_out, float *weights_out);
/* A handle with an episode time limit (rmav_set_time_limit) runs RMAV_POLICY_FP32_MFMA, RMAV_POLICY_F16_MFMA and RMAV_POLICY_F16_SHARED;
 * RMAV_POLICY_FP32 and RMAV_POLICY_BF16_MFMA return RMAV_ERR_INVALID there (no time-limited kernel: they already sit at their register
 * limit).  A truncated step has done = 1 and its ordinary reward: rmav_gae treats it as an episode boundary without a bootstrap
 * (rmav_rollout_policy_boot + rmav_gae_boot below add it). */
int rmav_rollout_policy(rmav_handle h, int32_t n_steps, const float *weights, float *actions_out,
                        float *obs_out, float *rew_out, uint8_t *done_out, float *logp_out,
                        float *value_out, int precision);

/* rmav_rollout_policy, plus the bootstrap term of truncated steps.  The auto-reset runs inside the launch, so the state a truncated
 * episode ended in never reaches the caller; here the launch evaluates its own value net on it:
 *   boot_out  [n_steps][N] (required): V(s_final) where step t was truncated by the time limit (s_final = the state after the
 *             dynamics, before the reset; the same device function that produces value_out), 0.0f everywhere else - running and
 *             terminated steps (termination wins over truncation, so a terminated step has boot = 0).
 *   trunc_out u8 [n_steps][N] (nullable): 1 where the time limit ended the episode with step t.
 * Needs a time limit on the handle and one of the three precisions a time-limited handle accepts (RMAV_POLICY_FP32_MFMA,
 * RMAV_POLICY_F16_MFMA, RMAV_POLICY_F16_SHARED); anything else, and RMAV_REINMAV, is RMAV_ERR_INVALID.  Everything else the launch
 * does - states, actions, rewards, done, logp, values, statistics, reset counters, truncated flags of the handle - is bit-identical
 * to rmav_rollout_policy on the same handle.  Cost: one 4-byte and one 1-byte store per env-step, and one more value-net pass of a
 * wavefront on the steps in which one of its envs is truncated (about one step in max_episode_steps). */
int rmav_rollout_policy_boot(rmav_handle h, int32_t n_steps, const float *weights, float *actions_out, float *obs_out,
                             float *rew_out, uint8_t *done_out, float *logp_out, float *value_out, float *boot_out,
                             uint8_t *trunc_out, int precision);

/* ---- learner-side passes over a trajectory (DEVICE pointers, enqueued on the handle's stream) -------- */
/* Generalised advantage estimation, the backward pass of baselines ppo2 Runner.run():
 *   delta_t = reward_scale * r_t + gamma V_{t+1} (1 - done_t) - V_t,  A_t = delta_t + gamma lam (1 - done_t) A_{t+1}
 * rew [n_steps][N], done u8 [n_steps][N] (1 = the episode ended with step t), values [n_steps + 1][N]
 * (values[n_steps] = bootstrap value; exactly what rmav_rollout_policy writes); adv_out, ret_out [n_steps][N]
 * (ret = A + V).  sums_out (nullable): 2 doubles on the device <- (sum A, sum A^2) over all n_steps*N samples,
 * for the advantage normalisation (all-reduce them across ranks first when data parallel).  fp32 FMAs;
 * agrees with a float64 per-env recursion to ~1e-6 relative. */
int rmav_gae(rmav_handle h, int32_t n_steps, const float *rew, const uint8_t *done, const float *values,
             float gamma, float lam, float reward_scale, float *adv_out, float *ret_out, double *sums_out);
/* rmav_gae with the bootstrap term of truncated steps (boot [n_steps][N], what rmav_rollout_policy_boot writes):
 *   delta_t = reward_scale r_t + gamma ((1 - done_t) V_{t+1} + boot_t) - V_t ;  A_t as in rmav_gae (the recursion still stops at
 * every done): the return target of a truncated step becomes r + gamma V(s_final) instead of r alone.  boot all zero gives
 * rmav_gae's values.  RMAV_REINMAV: RMAV_ERR_INVALID. */
int rmav_gae_boot(rmav_handle h, int32_t n_steps, const float *rew, const uint8_t *done, const float *values, const float *boot,
                  float gamma, float lam, float reward_scale, float *adv_out, float *ret_out, double *sums_out);
/* x[i] <- (x[i] - mean) * rstd for i < count (x 16-byte aligned): advantage normalisation in place. */
int rmav_normalize(rmav_handle h, float *x, int64_t count, float mean, float rstd);

/* ---- observation normalisation: baselines' VecNormalize(ob=True, ret=False) in front of the nets ------------------------------------
 * RunningMeanStd (third-party behaviour restated from memory): mean = 0, var = 1, count = epsilon; update(batch of B rows) merges the
 * batch's mean / population variance / B into them (Chan's parallel formula); normalise(x) = clip((x - mean) / sqrt(var + eps), +-clip).
 * The four quadrotor kinds; RMAV_REINMAV is RMAV_ERR_INVALID in every call below.
 *
 * The statistics live in ONE caller-owned DEVICE buffer of rmav_obs_norm_bytes() bytes, 16-byte aligned (not handle state: several
 * collectors and a learner share it, and it outlives rmav_destroy).  Every call below is a launch on the handle's stream: nothing
 * synchronises, and a captured rollout sees the current statistics through the fixed pointer.  Fields (byte offset):
 *     0  double count          samples seen (starts at count0)
 *     8  double mean[16]       running mean per feature; features >= nS stay 0
 *   136  double m2[16]         running sum of squared deviations: var = m2 / count; features >= nS stay at var 1
 *   264  double eps            the epsilon under the square root
 *   272  float  clip           the clip (+inf = none), 3 pad words
 *   288  float  mean_f[16]     \  the tables the kernels read, rewritten by every merge:  mean_f = (float)mean,
 *   352  float  rstd_f[16]      | rstd_f = (float)(1 / sqrt(var + eps)) (computed in fp64, rounded once); features >= nS: 0 and 1
 *   416  float  clip_f         /   3 pad words
 * THE arithmetic, wherever an observation is normalised (rmav_obs_normalize, the rollout below), in fp32, uncontracted, in this order:
 *     z = (x - mean_f[c]) * rstd_f[c];   z = min(max(z, -clip), clip)
 * so torch's clamp((obs - mean_f) * rstd_f, -clip, clip) in fp32 reproduces it bit for bit for finite x, and identity statistics
 * (mean 0, rstd 1, clip +inf) leave the bits of x. */
int64_t rmav_obs_norm_bytes(void);
/* mean 0, var 1, count = count0 (baselines: 1e-4), clip > 0 (baselines: 10; +inf allowed), eps >= 0 (baselines: 1e-8); tables from that
 * state: mean_f = 0, rstd_f = (float)(1 / sqrt(1 + eps)) (= 1.0f for eps <= 5e-8). */
int rmav_obs_norm_init(rmav_handle h, void *stats, float clip, double eps, double count0);
/* Batch moments of a stored observation array: batch_out <- 33 doubles on the device (count, mean[16], m2[16]; m2 = sum of squared
 * deviations from the batch mean; features >= nS zero).  obs: layout RMAV_SOA = [n_rows][nS][pitch] (what the rollouts write; pitch = 0
 * means N, the first N of every pitch are read) or RMAV_AOS = [n_rows * N][nS] (what rmav_step writes; pitch must be 0).  count =
 * n_rows * N.  Two stages: per-block fp64 (n, mean, M2) partials combined pairwise (Chan), then a fold; no floating-point atomics - the
 * same input gives the same bits.  n_rows = 0 leaves an empty record.  Uses the handle's scratch buffer. */
int rmav_obs_moments(rmav_handle h, const float *obs, int layout, int32_t n_rows, int64_t pitch, double *batch_out);
/* Merges n_batches consecutive 33-double records (DEVICE) into the running state, in order, with RunningMeanStd's update rule, then
 * rewrites the tables; empty records are skipped.  n_batches > 1: every rank's record after an all-gather, merged in rank order so that
 * all ranks end with the same bits.  One tiny launch. */
int rmav_obs_norm_merge(rmav_handle h, void *stats, const double *batch, int32_t n_batches);
/* out = the arithmetic above applied to in, elementwise (layouts as rmav_obs_moments; out == in allowed; n_rows = 0: no-op). */
int rmav_obs_normalize(rmav_handle h, const void *stats, const float *in, float *out, int layout, int32_t n_rows, int64_t pitch);
/* rmav_rollout_policy (handle without a time limit: boot_out and trunc_out must be NULL) or rmav_rollout_policy_boot (handle with one:
 * boot_out required) with EVERY evaluation of the policy and of the value net - value_out[n_steps] and the bootstrap value of a truncated
 * episode's terminal state included - fed the normalised observation.  obs_out still holds the RAW state; everything else is laid out as
 * there.  precision: RMAV_POLICY_FP32_MFMA, RMAV_POLICY_F16_MFMA or RMAV_POLICY_F16_SHARED (the other two have no normalised kernel, for
 * the reason above: RMAV_ERR_INVALID).  The statistics are FROZEN for the launch - a fused launch has no grid-wide meeting point between
 * its steps - where baselines updates them every env-step: absorb the rollout afterwards (rmav_obs_moments + rmav_obs_norm_merge on
 * obs_out).  With identity statistics every output has the bits of rmav_rollout_policy / rmav_rollout_policy_boot. */
int rmav_rollout_policy_norm(rmav_handle h, int32_t n_steps, const float *weights, const void *stats, float *actions_out, float *obs_out,
                             float *rew_out, uint8_t *done_out, float *logp_out, float *value_out, float *boot_out, uint8_t *trunc_out,
                             int precision);

/* ---- the action rule of rmav_rollout_policy / _boot / _norm: clipping to the action space, deterministic evaluation -----------------
 * What the in-kernel actors do between the policy's mean head and the dynamics.  stable-baselines' PPO2 runner steps the env with
 * clip(action, Box.low, Box.high) but stores the unclipped action and ITS log-probability for the learner; predict(deterministic=True)
 * takes the mean.  Handle state, host only (no launch, no synchronisation), default (0, -inf, +inf):
 *   deterministic  0 | 1                 noise = deterministic ? 0.0f : 1.0f
 *   clip_lo <= clip_hi, neither NaN       -inf / +inf = no bound on that side; anything else is RMAV_ERR_INVALID
 * THE arithmetic, in fp32, uncontracted, in this order (z = the launch's unit Gaussian draw of (seed, env, step), as without a rule):
 *     std_eff[c] = exp(logstd[c]) * noise                       once per launch
 *     a[c]       = fma(std_eff[c], z[c], mean[c])               -> actions_out: the STORED action is never clipped
 *     logp       = fma(-0.5, noise * sum_c z[c]^2, logp0)       logp0 = -sum(logstd) - nA/2 ln(2 pi); deterministic: logp = logp0
 *     u[c]       = min(max(a[c], clip_lo), clip_hi)             -> the dynamics; obs, reward, done, the episode statistics and the
 *                                                                  boot / trunc outputs all follow from u
 * A non-finite a[c] is not specified.  IDENTITY: with (0, -inf, +inf) every output has the bits it has without a rule for finite
 * actions (std * 1.0f, 1.0f * q and min / max against the infinities are exact), and such a handle launches exactly the kernels it
 * launched before.  Any other rule routes the call as a parameter range does: it runs the normalised kernel of its actor (with
 * identity tables when the call brought no statistics, and the handle's own scratch boot_out when the handle has a time limit and the
 * call asked for no bootstrap term), so RMAV_POLICY_FP32, RMAV_POLICY_BF16_MFMA and RMAV_REINMAV return RMAV_ERR_INVALID.
 * The rule affects these three entry points only: rmav_step, rmav_rollout (caller, random and controller actions) never read it - the
 * caller owns those actions.  The values are kernel arguments: a captured graph keeps the rule it was captured with, as it keeps the
 * time limit. */
int rmav_set_policy_action_rule(rmav_handle h, int32_t deterministic, float clip_lo, float clip_hi);
int rmav_get_policy_action_rule(rmav_handle h, int32_t *deterministic, float *clip_lo, float *clip_hi);

/* ---- return normalisation:the reward half of baselines' VecNormalize(ret=True) in front of GAE -------------------------------------
 * baselines (third-party behaviour restated from memory), per env-step and per env:
 *     R = R * gamma + rew                    R: one float per env, 0 after reset(); gamma = 0.99
 *     ret_rms.update(R)                      ONE scalar RunningMeanStd (mean 0, var 1, count 1e-4; Chan's merge) over all envs
 *     rew = clip(rew / sqrt(ret_rms.var + eps), +-cliprew)         cliprew = 10; the mean is NOT subtracted
 *     R[done] = 0
 * --reward_scale acts inside each env, in front of the wrapper: R accumulates reward_scale * r.  All five env kinds.
 *
 * The statistics live in ONE caller-owned DEVICE buffer of rmav_ret_norm_bytes() bytes, 16-byte aligned (not handle state, as the
 * observation statistics above).  Every call below is a launch on the handle's stream: nothing synchronises.  Fields (byte offset):
 *     0  double count          returns seen (starts at count0)
 *     8  double mean           running mean of R (kept for RunningMeanStd's merge; the normalisation does not use it)
 *    16  double m2             running sum of squared deviations: var = m2 / count
 *    24  double eps            the epsilon under the square root
 *    32  float  clip           the clip (+inf = none), 3 pad words
 *    48  float  rstd_f         \  the table the kernels read, rewritten by every merge:
 *    52  float  clip_f         /  rstd_f = (float)(1 / sqrt(var + eps)) (computed in fp64, rounded once); 2 pad words
 * THE arithmetic, wherever a reward is normalised (rmav_ret_normalize, rmav_gae_norm), in fp32, uncontracted, in this order:
 *     z = (reward_scale * r) * rstd_f;   z = min(max(z, -clip), clip)
 * so torch's clamp((rew * scale) * rstd_f, -clip, clip) in fp32 reproduces it bit for bit for finite r, and identity statistics
 * (rstd 1, clip +inf) with reward_scale = 1 leave the bits of r. */
int64_t rmav_ret_norm_bytes(void);
/* mean 0, var 1, count = count0 (baselines: 1e-4), clip > 0 (baselines: 10; +inf allowed), eps >= 0 (baselines: 1e-8); table from that
 * state: rstd_f = (float)(1 / sqrt(1 + eps)) (= 1.0f for eps <= 5e-8). */
int rmav_ret_norm_init(rmav_handle h, void *stats, float clip, double eps, double count0);
/* The forward scan over a stored trajectory: rew [n_steps][N], done u8 [n_steps][N] (what the rollouts write), carry float [N] = R of
 * every env before the first step (in) and after the last one (out; zero it when the envs are reset).  Per step, in fp32:
 *     R = fmaf(gamma, R, reward_scale * r_t);   R enters the moments;   R = 0 where done_t
 * batch_out <- 3 doubles on the device (count = n_steps * N, mean, m2 = sum of squared deviations from the batch mean), accumulated
 * per env in fp64 and combined pairwise (Chan) per block, then folded - no floating-point atomics: the same input gives the same
 * bits.  n_steps = 0 leaves an empty record (count 0) and does not touch carry.  Reads 5 bytes per sample.  Uses the handle's scratch
 * buffer. */
int rmav_ret_moments(rmav_handle h, int32_t n_steps, const float *rew, const uint8_t *done, float reward_scale, float gamma, float *carry,
                     double *batch_out);
/* Merges n_batches consecutive 3-double records (DEVICE) into the running state, in order, with RunningMeanStd's update rule, then
 * rewrites the table; empty records are skipped.  n_batches > 1: every rank's record after an all-gather, merged in rank order so that
 * all ranks end with the same bits.  One tiny launch. */
int rmav_ret_norm_merge(rmav_handle h, void *stats, const double *batch, int32_t n_batches);
/* out[i] = the arithmetic above applied to in[i], i < count (out == in allowed; count = 0: no-op). */
int rmav_ret_normalize(rmav_handle h, const void *stats, const float *in, float *out, int64_t count, float reward_scale);
/* rmav_gae (boot NULL) / rmav_gae_boot (boot [n_steps][N]) with the arithmetic above applied to every reward as it is loaded:
 *   delta_t = z_t + gamma ((1 - done_t) V_{t+1} [+ boot_t]) - V_t,  z_t = clamp((reward_scale r_t) * rstd_f, -clip, clip)
 * rstd_f / clip_f are read from `stats` inside the launch (no host read of the scale), and the normalised rewards are never stored:
 * the launch moves the bytes of rmav_gae / rmav_gae_boot.  Outputs, sums_out included, have the bits of rmav_gae / rmav_gae_boot
 * with reward_scale = 1 on the output of rmav_ret_normalize; identity statistics and reward_scale = 1 give their bits on the raw
 * rewards.  boot non-NULL follows rmav_gae_boot's rules (RMAV_REINMAV: RMAV_ERR_INVALID), boot NULL rmav_gae's. */
int rmav_gae_norm(rmav_handle h, int32_t n_steps, const float *rew, const uint8_t *done, const float *values, const float *boot,
                  const void *stats, float gamma, float lam, float reward_scale, float *adv_out, float *ret_out, double *sums_out);

/* ---- the fused learner: clipped-surrogate loss of ONE minibatch and its gradient, one launch per net plus a fold ----------------------
 * What gym_reinmav_amd.ppo.PPO.loss + backward() compute for an MlpPolicy(value_network = 'copy', hidden = 64) - two 2 x 64 tanh nets and
 * a state-independent logstd - in fp32, with every activation, delta and weight-gradient accumulator in registers and LDS
 * (csrc/rmav_learner.hpp).  The optimiser step, the gradient-norm clip and the data-parallel all-reduce stay with the caller.
 * Per sample j of the minibatch (x = obs, or with obs_stats  x = clamp((obs - mean_f) * rstd_f, +-clip_f), THE arithmetic above; no
 * gradient flows into the statistics):
 *     mean = pi(x), v = vf(x);   z = (act - mean) exp(-logstd);   logp = -1/2 sum z^2 - sum logstd - nA/2 log 2 pi
 *     ratio = exp(logp - logp_old);   a = (adv - adv_norm[0]) * adv_norm[1]
 *     pg = mean_j max(-a ratio, -a clamp(ratio, 1 - clip, 1 + clip))
 *     v_clip = val_old + clamp(v - val_old, +-clip);   vf = 1/2 mean_j max((v - ret)^2, (v_clip - ret)^2)
 *     loss = pg + vf_coef vf - ent_coef sum_c (logstd_c + 1/2 log 2 pi e)
 * Sub-gradients are torch autograd's: max() hands the gradient to the larger argument and halves it on a tie (so inside the clip range,
 * where both arguments are equal, it flows as through the unclipped branch), clamp's gradient is 1 on the closed interval.
 *
 * The flat gradient, rmav_ppo_grad_param_count(kind) floats, in this fixed order, each tensor in torch's row-major shape:
 *     pi.W1 [64][nS] | pi.b1 [64] | pi.W2 [64][64] | pi.b2 [64] | pi.W3 [nA][64] | pi.b3 [nA] |
 *     vf.W1 [64][nS] | vf.b1 [64] | vf.W2 [64][64] | vf.b2 [64] | vf.W3 [1][64]  | vf.b3 [1]  | logstd [nA]
 * (-1 for a bad kind.)  All five kinds. */
typedef struct rmav_ppo_grad_spec {
    float clip;      /* finite, >= 0 (PPO2: 0.2): the ratio clip AND the value clip, as in baselines' ppo2 */
    float vf_coef;   /* finite (0.5) */
    float ent_coef;  /* finite (0) */
    int32_t _reserved; /* 0 */
} rmav_ppo_grad_spec;
int64_t rmav_ppo_grad_param_count(int kind);
/* Bytes of the caller-owned DEVICE workspace of a call with this batch size (per-workgroup partial gradients; 16-byte aligned; its
 * contents need no initialisation and mean nothing between calls).  -1 for a bad kind or batch < 1. */
int64_t rmav_ppo_grad_workspace_bytes(int kind, int64_t batch);
/* Three launches on the handle's stream (the policy net, the value net, the fold of the per-workgroup partials); nothing allocates,
 * nothing synchronises, the handle's scratch buffer is not used.
 *   batch       samples of the minibatch, in [1, 2^31)
 *   idx         int64 [batch] on the DEVICE, or NULL: sample j is column idx[j] of every input array below (NULL: column j).  The
 *               contents cannot be checked without a synchronisation - THE CALLER'S CONTRACT: 0 <= idx[j] < the pitch of every array
 *               (obs_pitch, act_pitch, and the lengths of logp_old, val_old, adv, ret)
 *   obs, act    feature-major [nS][obs_pitch], [nA][act_pitch] (pitches in floats; >= batch when idx is NULL); obs is RAW
 *   logp_old, val_old, adv, ret   one float per column
 *   adv_norm    2 floats on the DEVICE: the mean of the minibatch's advantages and 1 / (std + 1e-8)
 *   params      HOST array of the 13 DEVICE pointers of the parameters, in the order above (as rmav_pack_policy takes them)
 *   obs_stats   an observation-statistics buffer (rmav_obs_norm_bytes()), or NULL = x is obs
 *   workspace   rmav_ppo_grad_workspace_bytes(kind, batch) bytes
 *   grad_out    rmav_ppo_grad_param_count(kind) floats <- the gradient of loss
 *   stats_out   4 floats <- loss, pg, vf, max_j ratio
 * DETERMINISM: no floating-point atomics; the launch geometry and the order of every sum depend on (kind, batch) alone, and sample j is
 * processed in position j whether it came through idx or not: the same inputs give the same bits, and a minibatch given by idx gives
 * the bits of the same samples gathered into contiguous arrays and passed with idx = NULL.  Samples beyond batch in the last tile read
 * the last sample's column and contribute exact zeros.
 * RMAV_ERR_INVALID (the message names the argument): batch < 1, a NULL required pointer, a pitch too small, clip / vf_coef / ent_coef
 * not finite, clip < 0. */
int rmav_ppo_grad(rmav_handle h, int64_t batch, const int64_t *idx, const float *obs, int64_t obs_pitch, const float *act, int64_t act_pitch,
                  const float *logp_old, const float *val_old, const float *adv, const float *ret, const float *adv_norm,
                  const float *const *params, const void *obs_stats, const rmav_ppo_grad_spec *spec, void *workspace, float *grad_out,
                  float *stats_out);

/* ---- the fused learner of the shared-trunk policy: the same loss, ONE net launch plus the fold -------------------------------------
 * What PPO.loss + backward() compute for an MlpPolicy(value_network = 'shared', hidden = 64): ONE 2 x 64 tanh trunk whose latent h2
 * feeds the mean head pi.2 and the scalar value head vf.0 (csrc/rmav_learner_shared.hpp).  The loss, the sub-gradient rules, the
 * arithmetic of x, the statistics and the determinism rule are those of the block above, with  mean = W3 h2 + b3,  v = w_v . h2 + b_v.
 * What differs:
 *   one trunk       the observation is read and normalised once, layers 1 and 2 run forward once
 *   the summed delta   the trunk's gradient is that of BOTH heads: delta 2 = (W3^T d_mean + w_v d_v) * (1 - h2^2), the value head's
 *                   delta carrying vf_coef
 *   two launches    the net and the fold of the per-workgroup partials (rmav_ppo_grad: three)
 * The flat gradient, rmav_ppo_grad_shared_param_count(kind) = 64 nS + 64 + 4096 + 64 + 64 nA + nA + 64 + 1 + nA floats, and the HOST
 * array params of 9 DEVICE pointers, in this fixed order, each tensor in torch's row-major shape:
 *     pi.W1 [64][nS] | pi.b1 [64] | pi.W2 [64][64] | pi.b2 [64] | pi.W3 [nA][64] | pi.b3 [nA] | vf.W [1][64] | vf.b [1] | logstd [nA]
 * (-1 for a bad kind.)  All five kinds. */
int64_t rmav_ppo_grad_shared_param_count(int kind);
/* Bytes of the caller-owned DEVICE workspace: workgroups * (rmav_ppo_grad_shared_param_count(kind) + 4) * 4 with one workgroup per
 * 64-sample tile up to 512; the rules of rmav_ppo_grad_workspace_bytes.  -1 for a bad kind or batch < 1. */
int64_t rmav_ppo_grad_shared_workspace_bytes(int kind, int64_t batch);
/* The arguments of rmav_ppo_grad with the same meaning, checks and messages; params holds the 9 pointers above, workspace and grad_out
 * have the sizes the two functions above give.  stats_out: loss, pg, vf, max_j ratio. */
int rmav_ppo_grad_shared(rmav_handle h, int64_t batch, const int64_t *idx, const float *obs, int64_t obs_pitch, const float *act,
                         int64_t act_pitch, const float *logp_old, const float *val_old, const float *adv, const float *ret,
                         const float *adv_norm, const float *const *params, const void *obs_stats, const rmav_ppo_grad_spec *spec,
                         void *workspace, float *grad_out, float *stats_out);

/* ---- the shared-trunk learner on the fp32 matrix cores: the same loss and gradient, every product on v_mfma_f32_32x32x2_f32 ------------
 * rmav_ppo_grad_shared with another net kernel (csrc/rmav_learner_mfma.hpp): the loss, the sub-gradient rules, the arithmetic of x, the
 * statistics, the 9 parameters, the flat gradient (rmav_ppo_grad_shared_param_count(kind) floats in that order) and the two launches
 * (the net, then the same fold) are those of the block above.  The fp32-input matrix instruction is a k-ordered fmaf chain: the result
 * is in the precision class of rmav_ppo_grad_shared and differs from it in the order of summation only.
 *   geometry      a wavefront owns a tile of 32 samples, a workgroup of 4 wavefronts a step of 128; step s belongs to workgroup
 *                 s mod workgroups, workgroups = min(ceil(batch / 128), 256): one workgroup per CU (124.5 KB of LDS)
 *   determinism   no atomics; sample j sits in lane j mod 32 of wavefront (j / 32) mod 4 of step j / 128 with or without idx (the idx
 *                 route gives the bits of the gathered route); a wavefront adds its tiles in order, a workgroup its wavefronts in
 *                 order, the fold the workgroups in order; geometry and order depend on (kind, batch) alone, so the same inputs give
 *                 the same bits.  A lane beyond batch reads the last sample's column and adds exact zeros.
 * Bytes of the caller-owned DEVICE workspace: workgroups * (rmav_ppo_grad_shared_param_count(kind) + 4) * 4 with the workgroups above;
 * the rules of rmav_ppo_grad_workspace_bytes.  -1 for a bad kind or batch < 1. */
int64_t rmav_ppo_grad_shared_mfma_workspace_bytes(int kind, int64_t batch);
/* The arguments of rmav_ppo_grad_shared with the same meaning, checks and messages; workspace has the size the function above gives. */
int rmav_ppo_grad_shared_mfma(rmav_handle h, int64_t batch, const int64_t *idx, const float *obs, int64_t obs_pitch, const float *act,
                              int64_t act_pitch, const float *logp_old, const float *val_old, const float *adv, const float *ret,
                              const float *adv_norm, const float *const *params, const void *obs_stats, const rmav_ppo_grad_spec *spec,
                              void *workspace, float *grad_out, float *stats_out);

/* ---- around the fused learner: the advantage moments it takes, and the optimiser step on its gradient --------------------------------
 * rmav_adv_moments writes the two floats rmav_ppo_grad / rmav_ppo_grad_shared take as adv_norm:
 *     adv_norm_out[0] = mean_j x_j,   adv_norm_out[1] = 1 / (std + 1e-8),   x_j = adv[idx[j]] (idx NULL: adv[j]),  j < batch
 * std is torch's default unbiased estimator (divisor batch - 1); batch = 1 gives (x_0, NaN) as torch.std_mean does - no special case.
 * Two launches on the handle's stream (k_adv_moments, k_adv_moments_fold); nothing allocates, nothing synchronises, the handle's scratch
 * buffer is not used.  Per lane sum (x - K) and sum (x - K)^2 in fp64 with K = x_0 (x - K is exact in fp64), Chan's pairwise combination
 * above that in a fixed order, one moment per workgroup in `workspace`, folded in workgroup order.  The last step is fp32, as the torch
 * expression on fp32 tensors is:
 *     mean = (float)mean64;   std = (float)sqrt(M2 / (batch - 1));   adv_norm_out[1] = 1.0f / (std + 1e-8f)
 * DETERMINISM: no atomics; min(ceil(batch / 256), 128) workgroups of 256 lanes, sample j in lane j mod 256 of workgroup (j / 256) mod
 * workgroups with or without idx, a lane adding its samples in order: the same inputs give the same bits, and the idx route gives the
 * bits of the gathered route.
 *   workspace   rmav_adv_moments_workspace_bytes(batch) = 24 * min(ceil(batch / 256), 128) bytes on the DEVICE, 8-byte aligned; its
 *               contents need no initialisation and mean nothing between calls (-1 for batch < 1)
 *   idx         int64 [batch] on the DEVICE or NULL; THE CALLER'S CONTRACT on its contents is rmav_ppo_grad's: 0 <= idx[j] < the length
 *               of adv
 * RMAV_ERR_INVALID (the message names the argument): batch < 1, adv / workspace / adv_norm_out NULL, a misaligned workspace. */
int64_t rmav_adv_moments_workspace_bytes(int64_t batch);
int rmav_adv_moments(rmav_handle h, int64_t batch, const int64_t *idx, const float *adv, void *workspace, float *adv_norm_out);

/* rmav_ppo_adam: what torch.nn.utils.clip_grad_norm_ + torch.optim.Adam.step() (no amsgrad, no weight decay) do to the parameters, from
 * the flat gradient rmav_ppo_grad / rmav_ppo_grad_shared leave, in ONE launch of one workgroup (k_ppo_adam) on the handle's stream.
 *   shared      0: the 13 tensors and flat order of rmav_ppo_grad;  1: the 9 of rmav_ppo_grad_shared
 *   grad        the flat gradient (rmav_ppo_grad_param_count / rmav_ppo_grad_shared_param_count floats), READ ONLY: it keeps the
 *               unscaled, unclipped gradient (clip_grad_norm_ overwrites p.grad; this call does not)
 *   params      HOST array of the 13 / 9 DEVICE pointers, updated in place
 *   exp_avg, exp_avg_sq   Adam's first and second moments, flat, in the order of grad, updated in place (zeros before step 1)
 *   step        the number of this update, >= 1
 *   stats_out   2 floats on the DEVICE <- norm, coef; or NULL
 * THE arithmetic, in fp32, uncontracted, one line per operation, per element i (sqrt and divide correctly rounded):
 *     g    = grad[i] * grad_scale
 *     norm = (float)sqrt(sum_i (double)g * (double)g)      strided per-thread partials and a fixed-order reduction in fp64, rounded once
 *     ratio = max_grad_norm / (norm + 1e-6f)
 *     coef = ratio >= 1 ? 1 : ratio                          min(1, ratio) that keeps a NaN, as torch.clamp(max = 1) does
 *     gh   = g * coef
 *     d = gh - m;   td = omb1 * d;   m = m + td              omb1 = 1.0f - beta1 (fp32, on the host)        [exp_avg.lerp_(gh, 1 - beta1)]
 *     a = beta2 * v;   b = gh * gh;   c = omb2 * b;   v = a + c      omb2 = 1.0f - beta2                    [exp_avg_sq]
 *     s = sqrtf(v);   q = s / bc2_sqrt;   den = q + eps      bc2_sqrt = (float)sqrt(1 - (double)beta2^step)
 *     r = m / den;   u = step_size * r;   p = p - u          step_size = (float)((double)lr / (1 - (double)beta1^step))
 * The two bias corrections are computed on the host in fp64 from the fp32 fields of the spec and rounded to fp32 once.  Non-finite
 * gradients get no special case: they propagate as in torch's sequence (a NaN anywhere in grad makes norm, coef and with them every
 * parameter NaN; a g^2 beyond fp32 makes v infinite and the element's step 0).
 * DETERMINISM: no atomics, one workgroup, every sum in a fixed order: the same inputs give the same bits.
 * RMAV_ERR_INVALID (the message names the argument): shared not 0 / 1; grad, params, params[k], exp_avg, exp_avg_sq or spec NULL;
 * step < 1; lr or eps not finite or < 0; beta1 or beta2 outside [0, 1); max_grad_norm NaN or <= 0; grad_scale not finite or <= 0;
 * _reserved non-zero. */
typedef struct rmav_ppo_adam_spec {
    float lr, beta1, beta2, eps;      /* torch.optim.Adam's; PPO uses 3e-4, 0.9, 0.999, 1e-5 */
    float max_grad_norm;              /* > 0, or +inf for no clip */
    float grad_scale;                 /* finite, > 0: 1 / world size after a SUM all-reduce; 1 otherwise */
    int32_t _reserved[2];             /* 0 */
} rmav_ppo_adam_spec;
int rmav_ppo_adam(rmav_handle h, int shared, const float *grad, float *const *params, float *exp_avg, float *exp_avg_sq, int64_t step,
                  const rmav_ppo_adam_spec *spec, float *stats_out);

#ifdef __cplusplus
}
#endif
#endif

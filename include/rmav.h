/* rmav.h - C ABI of the MI355X-native batched quadrotor dynamics path (librmav.so).
 *
 * This is the drop-in boundary for reinmav-gym's native environments.  The reference has no FFI
 * (it is pure Python); what a binding replaces is the body of its five native gym.Env classes in
 * gym_reinmav/envs/native/ of the reference repository:
 *
 *   reference interface (file:line)                               entry point here
 *   ---------------------------------------------------------------------------------------------
 *   Quadrotor3D.__init__            quadrotor3d.py:44-74          rmav_create(RMAV_QUAD3D, ...)
 *   Quadrotor3DSlungload.__init__   quadrotor3d_slungload.py:44-80  rmav_create(RMAV_QUAD3D_SL, ...)
 *   Quadrotor2D.__init__            quadrotor2d.py:43-67          rmav_create(RMAV_QUAD2D, ...)
 *   Quadrotor2DSlungload.__init__   quadrotor2d_slungload.py:43-73  rmav_create(RMAV_QUAD2D_SL, ...)
 *   ReinmavEnv.__init__ / .step()   reinmav_env.py:53-84, 99-126  rmav_create(RMAV_REINMAV, ...),
 *                                                                 rmav_rollout(RMAV_ACT_CONTROLLER), rmav_get_time
 *   (hard-coded physics literals in each __init__)                rmav_default_params / rmav_params
 *   .seed(seed)                     quadrotor3d.py:77-79          rmav_seed
 *   .reset()                        quadrotor3d.py:182-185        rmav_reset
 *   .step(action)                   quadrotor3d.py:81-124         rmav_step        (batch of N envs)
 *                                   quadrotor3d_slungload.py:87-167
 *                                   quadrotor2d.py:74-113
 *                                   quadrotor2d_slungload.py:79-154
 *   .control()                      quadrotor3d.py:126-180        rmav_control
 *                                   quadrotor2d.py:115-138
 *   one iteration "action = env.control(); env.step(action)" of the reference's smoke tests
 *                                   test/test_quadrotor2d.py:17-18  rmav_control_step (one launch), or rmav_step_control
 *                                   test/test_quadrotor3d.py:16-17  (step + the NEXT control() in one launch)
 *   .state / .steps_beyond_done     quadrotor3d.py:104,68         rmav_get_state / rmav_set_state,
 *                                                                 rmav_get_sbd / rmav_set_sbd
 *   the test loop "control -> step -> reset on done"              rmav_rollout(RMAV_ACT_CONTROLLER)
 *                                   test/test_quadrotor3d.py:16-22
 *   baselines VecEnv rollouts driven by gym_reinmav/run.py:89,190-211
 *                                                                 rmav_rollout(RMAV_ACT_BUFFER|RANDOM), rmav_rollout_chunked
 *   baselines ppo2 Runner.run(): model.step(obs) + env.step(a)    rmav_rollout_policy (+ rmav_pack_policy)
 *   baselines Monitor episode statistics (info['episode'])        rmav_episode_totals / _buffers
 *   baselines ppo2 Runner.run() advantage pass (GAE lambda)       rmav_gae, rmav_normalize
 *   MPI rank probe / data-parallel workers gym_reinmav/run.py:18-21,177-182
 *                                                                 rmav_comm_* + rmav_allgather_stats (RCCL over xGMI)
 *
 * INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - plain C types only; every function returns an rmav_status (0 = ok, < 0 = error) unless noted;
 *     rmav_last_error() returns a thread-local message for the last failure; nothing throws or
 *     aborts across this boundary.
 *   - a handle owns the device-resident env state (fp32, struct-of-arrays) of N independent envs on
 *     one GPU and one HIP stream; it is NOT thread-safe; distinct handles are independent.
 *   - `mem` says where every caller-supplied pointer of that call lives: RMAV_HOST (the library
 *     stages - calls that move <= 256 KiB go zero-copy through a pinned, device-mapped block owned by the
 *     handle: one launch + one synchronise (single-step calls of <= 64 envs wait on a pinned completion word the kernel
 *     writes instead), which is what the gym-shaped single env uses; bulk calls go
 *     through device scratch - and synchronises before returning) or RMAV_DEVICE (HIP device
 *     pointers, e.g. torch tensor data_ptr(); work is enqueued on the handle's stream and the call
 *     returns without synchronising).
 *   - `layout`: RMAV_SOA = [dim][N] (component-major, the native device layout, coalesced) or
 *     RMAV_AOS = [N][dim] (what gym / a policy network hands over).  Trajectory buffers of
 *     rmav_rollout are time-major: [T][dim][N] (SOA) or [T][N][dim] (AOS).
 *   - there is no CPU implementation behind this ABI: rmav_create fails with RMAV_ERR_NO_DEVICE
 *     when no GPU is visible.
 *
 * RNG streams (Philox4x32-10, key = (seed_lo, seed_hi), counter = (env_lo, env_hi, c2, c3), where
 * env is the GLOBAL env id = env_id_base + local index, so results do not depend on how envs are
 * sharded over GPUs):
 *   reset : c2 = index of this env's reset (0 for the first),  c3 = (1<<24) | j ; block j supplies
 *           state components 4j..4j+3 as  2*u - 1,  u = (x>>8) * 2^-24          (U[-1,1), as
 *           quadrotor3d.py:184 draws every state component).  A handle with a start-state spec (rmav_set_start_state) maps each of
 *           these values into its component's range, s_c = fma(h_c, v_c, m_c): same counters, same words, no stream of its own.
 *   action: block index b = the handle's global step counter t (4-action kinds) or t >> 1 (2-action kinds, which use
 *           draws 2 (t & 1) and 2 (t & 1) + 1 of the block, i.e. one Philox call per two steps);
 *           c2 = low 32 bits of b, c3 = (2<<24) | (bits 32..47 of b) << 8 ; component i = fma(act_hi-act_lo, u_i, act_lo)
 *   policy noise (rmav_rollout_policy): as "action" with tag 3; (r0,r1) and (r2,r3) -> Box-Muller:
 *           u1 = ((r>>8)+1) * 2^-24, u2 = (r'>>8) * 2^-24, z = sqrt(-2 ln u1) * (cos, sin)(2 pi u2)
 *   env constants (rmav_set_env_param_range): ONE block per env and reset, c2 = index of this env's reset (the c2 of the fresh state
 *           of that reset), c3 = (4<<24); word `which` (enum rmav_env_param) gives u = (x>>8) * 2^-24 and
 *           value = fma(hi - lo, u, lo) in fp32
 *   wind (rmav_set_disturbance): ONE block per env and episode, c2 = the reset index of that episode (the env-constants stream's),
 *           c3 = (5<<24); word i gives w_i = fma(wind_hi_i - wind_lo_i, u, wind_lo_i) in fp32
 *   gust (rmav_set_disturbance): block index b = floor(t / gust_hold), t = the handle's global step counter (agent steps, as "action");
 *           c2 = low 32 bits of b, c3 = (6<<24) | (bits 32..47 of b) << 8 ; word i gives q_i = fma(gust_i + gust_i, u, -gust_i)
 *   sensor (rmav_set_sensor_noise): block (b, j), j = c >> 2 in 0 .. 3 for observation component c; b = the handle's global step counter
 *           AFTER the operation that produced the observation; c2 = low 32 bits of b, c3 = (7<<24) | (bits 32..47 of b) << 8 | j;
 *           (r0,r1) and (r2,r3) go through Box-Muller exactly as "noise": u1 = ((r>>8)+1) * 2^-24, u2 = (r'>>8) * 2^-24,
 *           rad = sqrtf(-2 logf(u1)), sincospif(2 u2), z = rad * (cos, sin); that gives z[4j .. 4j+3]
 */
#ifndef RMAV_H
#define RMAV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RMAV_VERSION 101 /* 0.1.1: rmav_params.g_vec */

typedef struct rmav_env_s *rmav_handle;

enum rmav_kind {
    RMAV_QUAD2D = 0,
    RMAV_QUAD2D_SL = 1,
    RMAV_QUAD3D = 2,
    RMAV_QUAD3D_SL = 3,
    /* ReinmavEnv (reinmav_env.py:51-352, id 'reinmav-v0'): 13-state rigid body [x y z dx dy dz qw qx qy qz p q r]
     * with thrust + body torques -> motor mixing/clamp -> linear and angular acceleration, 50-or-51 Euler
     * sub-steps of 1/5000 s per step, reward 90 and done = 1 on every step, reset() a no-op.  The reference's
     * step() takes no action: that behaviour is RMAV_ACT_CONTROLLER (built-in PD controller on a min-jerk
     * trajectory, evaluated every sub-step).  With RMAV_ACT_BUFFER / RANDOM / POLICY the 4 action components
     * are (F, Mx, My, Mz) held over the step (an extension).  Each env carries its own clock (rmav_get_time). */
    RMAV_REINMAV = 4
};

enum rmav_status {
    RMAV_OK = 0,
    RMAV_ERR_INVALID = -1,   /* bad argument */
    RMAV_ERR_NO_DEVICE = -2, /* no usable GPU */
    RMAV_ERR_HIP = -3,       /* a HIP runtime call failed (message has the HIP error string) */
    RMAV_ERR_ALLOC = -4,     /* device / host allocation failed */
    RMAV_ERR_TIMEOUT = -5    /* a bounded wait expired (rmav_allgather_stats_wait, an armed exchange whose launch never completed) */
};

enum rmav_mem { RMAV_HOST = 0, RMAV_DEVICE = 1 };
enum rmav_layout { RMAV_SOA = 0, RMAV_AOS = 1 };
enum rmav_action_mode {
    RMAV_ACT_BUFFER = 0,    /* actions read from a caller buffer */
    RMAV_ACT_RANDOM = 1,    /* uniform in [act_lo, act_hi) from the counter RNG, generated in-kernel */
    RMAV_ACT_CONTROLLER = 2, /* the reference's geometric controller, evaluated in-kernel */
    RMAV_ACT_POLICY = 3,     /* Gaussian MLP policy evaluated in-kernel (rmav_rollout_policy only: rmav_ppo.h) */
    RMAV_ACT_POLICY_BF16 = 4 /* the same policy on the matrix cores */
};
enum rmav_integrator { RMAV_INT_EULER = 0, RMAV_INT_RK4 = 1 };

/* rmav_create flags */
#define RMAV_F_AUTO_RESET 1u     /* VecEnv semantics: a done env is reset inside step; the returned
                                    obs is the post-reset obs (baselines DummyVecEnv.step_wait) */
#define RMAV_F_TRACK_EPISODES 2u /* keep per-env episode return/length (baselines Monitor) */

/* Physics and controller constants; defaults are the literals in each reference __init__
 * (rmav_default_params).  Doubles, so that e.g. dt is the same 0.01 the reference uses. */
typedef struct rmav_params {
    double mass;          /* quadrotor3d.py:45 */
    double load_mass;     /* quadrotor3d_slungload.py:46 */
    double dt;            /* quadrotor3d.py:46 */
    double g;             /* RMAV_REINMAV: the scalar self.gravity (reinmav_env.py:58).  Quadrotor kinds: not read (see g_vec);
                             rmav_default_params fills 9.8 = |g_vec| for information */
    double tether_length; /* quadrotor3d_slungload.py:58 / quadrotor2d_slungload.py:53 */
    double pos_limit;     /* episode ends when |pos| > pos_limit (which body: see DESIGN.md) */
    double vel_limit;     /* ... or |vel| > vel_limit */
    double thrust_scale;  /* quadrotor2d.py:75 (10 for quad2d, 1 otherwise) */
    int32_t clamp_thrust; /* quadrotor2d.py:76-77 (1 for quad2d) */
    int32_t integrator;   /* RMAV_REINMAV only: RMAV_INT_EULER (0, the reference: reinmav_env.py:90-98) or
                             RMAV_INT_RK4 (1: classical Runge-Kutta over the same sub-step grid, command held over
                             each sub-step; an option the reference does not have) */
    double ref_pos[3];    /* controller set-point  quadrotor3d.py:51 */
    double ref_vel[3];    /* quadrotor3d.py:52 */
    double kp, kv, tau;   /* controller gains  quadrotor3d.py:143-145, quadrotor2d.py:116-118 */
    double act_lo, act_hi; /* action Box bounds (quadrotor3d.py:70 etc.); used by RMAV_ACT_RANDOM only */
    double g_vec[3];      /* quadrotor kinds: the gravity VECTOR self.g, added component-wise by step() and subtracted by the 3-D
                             control() - quadrotor3d.py:47,96-99,162: (0, 0, -9.8); 2-D kinds use [0..1] - quadrotor2d.py:46,88:
                             (0, -9.8) - and their control() keeps the reference's literal (0, 9.8) (quadrotor2d.py:130) */
} rmav_params;

typedef struct rmav_ep_totals {
    uint64_t episodes;   /* finished episodes since creation / last clear */
    double return_sum;   /* sum of their returns */
    uint64_t length_sum; /* sum of their lengths */
} rmav_ep_totals;

/* ---- library-level ------------------------------------------------------------------------- */
int rmav_version(void);              /* returns RMAV_VERSION */
const char *rmav_last_error(void);   /* thread-local, never NULL */
int rmav_device_count(void);         /* number of visible GPUs, 0 if none (never negative) */
int rmav_state_dim(int kind);        /* 5, 9, 10, 16, 13; -1 for a bad kind */
int rmav_action_dim(int kind);       /* 2, 2, 4, 4, 4 */
int rmav_algorithmic_bytes(int kind); /* bytes per env-step of SURVEY.md 8(d): 53, 85, 101, 149, 125 */
/* reading_2d selects how the unparsable quadrotor2d.py:95-98 is read: 'B' -> |p|>3 or |v|>2
 * (default when 0 is passed), 'A' -> |p|>3 or |v|>10.  Ignored for other kinds. */
int rmav_default_params(int kind, int reading_2d, rmav_params *out);

/* ---- lifetime ------------------------------------------------------------------------------ */
/* Creates n_envs envs of `kind` on GPU `device`; env i has global id env_id_base + i.  All envs are
 * reset once (reset index 0), like the reference constructors (quadrotor3d.py:73-74).
 * params may be NULL (defaults).  hip_stream may be NULL (the handle creates its own non-blocking
 * stream) or a hipStream_t the caller owns (e.g. torch.cuda.current_stream().cuda_stream; pass
 * hipStreamLegacy == (void*)1 to name the legacy default stream, whose handle is 0).
 * n_envs <= 2^25: the size rule stated at rmav_rollout_pitched. */
int rmav_create(rmav_handle *out, int kind, int64_t n_envs, int device, uint64_t seed,
                uint64_t env_id_base, uint32_t flags, const rmav_params *params, void *hip_stream);
int rmav_destroy(rmav_handle h);
/* Re-keys the RNG and rewinds the reset / step counters (gym Env.seed).  Does not touch state. */
int rmav_seed(rmav_handle h, uint64_t seed);
int rmav_get_params(rmav_handle h, rmav_params *out);
int rmav_set_params(rmav_handle h, const rmav_params *in);
/* Rebind the handle to another HIP stream the caller owns (NULL: back to a stream owned by the
 * handle).  Pending work on the old stream is waited for first.  Lets a caller capture rmav_step /
 * rmav_rollout launches (mem = RMAV_DEVICE: no allocation, no synchronisation) into a hipGraph on its
 * capture stream. */
int rmav_set_stream(rmav_handle h, void *hip_stream);
/* Per-env (domain-randomised) physical constants.  The reference hard-codes one value per class
 * (quadrotor3d_slungload.py:45-59); RL users randomise them per env.  values: N floats (one per env)
 * or NULL to go back to the shared value of rmav_params.  Quadrotor kinds only. */
enum rmav_env_param { RMAV_PARAM_MASS = 0, RMAV_PARAM_LOAD_MASS = 1, RMAV_PARAM_TETHER_LENGTH = 2 };
int rmav_set_env_param(rmav_handle h, int which, const float *values, int mem);
/* N floats: the value every env runs with NOW - its element of the per-env array, or the shared value of rmav_params (rounded to
 * fp32) where the parameter has no array.  Quadrotor kinds only. */
int rmav_get_env_param(rmav_handle h, int which, float *out, int mem);

/* ---- per-episode domain randomisation (env constants redrawn at every reset, inside the step kernels) -----------------------
 * rmav_set_env_param gives every env its own constants, frozen for life.  Domain randomisation as RL users mean it draws new ones for
 * every episode; auto-reset runs inside the kernels (a fused launch carries an env through several episodes), so the redraw lives
 * there too.  Callers detect the feature by these symbols (RMAV_VERSION is unchanged).
 *   - A per-handle range [lo, hi] per parameter; none is the default: a handle that never sets one behaves exactly as without this
 *     feature and launches the kernels it launched before.
 *   - While parameter `which` has a range, the value of env i during an episode is a pure function of (seed, global env id, the reset
 *     index of that episode, which): the "env constants" stream of the RNG table above.  The reset index of an episode is the one its
 *     fresh state was drawn with (0 for the reset of rmav_create; the running episode's = rmav_get_reset_counts - 1, modulo 2^32).
 *     Global env ids make the values independent of sharding.
 *   - The values are env state, held in the per-env arrays of rmav_set_env_param, and are redrawn exactly when the env's state is: at
 *     rmav_reset and at every in-kernel auto-reset, by termination or by time-limit truncation.  rmav_set_env_param_range itself
 *     draws parameter `which` for every env's running episode (and allocates the array if there is none).  rmav_seed, rmav_set_state,
 *     rmav_set_reset_counts and rmav_set_step_count do not touch them.  Without RMAV_F_AUTO_RESET only rmav_reset redraws.
 *   - The step that ends an episode uses the old episode's constants; everything evaluated on the post-reset state - the next step,
 *     the trailing control() of rmav_step_control - the new ones.  What the kernels derive from the constants (1/mass,
 *     1/(mass + load_mass), mass * tether_length) is re-derived in fp64 from the new values, as at the start of a launch.
 *   - rmav_set_env_param(values) on a ranged parameter overwrites the values in force until each env's next reset; the range stays.
 *     rmav_set_env_param(NULL) clears both the range and the array.  A checkpoint is the ranges plus rmav_get_env_param: restore the
 *     ranges first, then the values.
 *   - lo == hi == v gives fma(0, u, v) = v: such a handle produces, in every launch, the bits of a handle given N copies of v through
 *     rmav_set_env_param.
 *   - Launches of a ranged handle run kernels of their own: fused rollouts use the one-wavefront kernels
 *     (RMAV_TUNE_SPLIT / RMAV_TUNE_SLICE / RMAV_TUNE_STEP_LAZY / RMAV_TUNE_STEP_STORE do not apply; a chunk-major call is one launch
 *     per chunk; results never depend on that), rmav_rollout_policy / _boot / _norm support RMAV_POLICY_FP32_MFMA, RMAV_POLICY_F16_MFMA
 *     and RMAV_POLICY_F16_SHARED (the others return RMAV_ERR_INVALID).
 * lo and hi finite with 0 < lo <= hi, anything else is RMAV_ERR_INVALID; quadrotor kinds only (RMAV_REINMAV: RMAV_ERR_INVALID).  A
 * parameter the kind does not read is accepted as rmav_set_env_param accepts it.
 * rmav_get_env_param_range: *enabled = 1 and the range, or 0 (and lo = hi = 0) when the parameter has none; any pointer may be NULL. */
int rmav_set_env_param_range(rmav_handle h, int which, float lo, float hi);
int rmav_get_env_param_range(rmav_handle h, int which, float *lo, float *hi, int32_t *enabled);
/* Explicit, per-handle overrides of the launch rules (DESIGN.md section 4 states the automatic rules and what was measured).
 * -1 = automatic, the default of every key.  Results never depend on them: every variant writes the same bits
 * (tests/test_gpu_parity.py::test_kernel_selection_variants_give_the_same_bits, ::test_single_step_variants_give_the_same_bits). */
/* A handle with an episode time limit (rmav_set_time_limit) ignores the split and slice keys: its fused rollouts always run one
 * wavefront per 64 envs (the two-wavefront kernels have no time-limited variant). */
/* A handle with a disturbance (rmav_set_disturbance) ignores RMAV_TUNE_STORE_POLICY as well: to bound the build its fused rollouts exist
 * for ONE store policy (write-back).  Results never depend on the store policy. */
enum rmav_tuning_key {
    RMAV_TUNE_SPLIT = 0,        /* fused rollouts: 0 = one wavefront per 64 envs, 1 = (integrator, memory) wavefront pairs */
    RMAV_TUNE_SLICE = 1,        /* batches beyond the pair kernel's capacity: 0 = one launch, 1 = one launch per balanced slice */
    RMAV_TUNE_STORE_POLICY = 2, /* trajectory stores: 0 write-back, 1 write-through, 2 non-temporal, 3 LDS-transposed batch-major obs */
    RMAV_TUNE_SPLIT_GROUP = 3,  /* (integrator, memory) pairs per workgroup, 1 .. 8 */
    RMAV_TUNE_BLOCK = 4,        /* workgroup size of the one-wavefront kernels: 64 | 128 | 256 */
    RMAV_TUNE_STEP_LAZY = 5,    /* rmav_step: 1 = the env's termination record is loaded only in lanes whose episode ends */
    RMAV_TUNE_STEP_STORE = 6,   /* rmav_step's per-env stores: 0 write-back, 1 write-through, 2 non-temporal */
    RMAV_TUNE_POLICY_PAIR = 7,  /* RMAV_POLICY_BF16_MFMA: 0 = one wavefront per 64 envs instead of the (actor, critic) pair */
    RMAV_TUNE_PAIR_GROUP = 8,   /* (actor, critic) pairs per workgroup of the matrix-core actors, 1 .. 4 */
    RMAV_TUNE_COUNT = 9
};
int rmav_set_tuning(rmav_handle h, int key, int value);
int rmav_get_tuning(rmav_handle h, int key, int *value_out);
int64_t rmav_num_envs(rmav_handle h); /* < 0 on a bad handle */
int rmav_sync(rmav_handle h);         /* waits for everything enqueued on the handle's stream */

/* ---- the hot path -------------------------------------------------------------------------- */
/* Reset every env (fresh U[-1,1) state); steps_beyond_done is NOT cleared (the reference's reset
 * does not).  obs_out (nS*N floats) may be NULL. */
int rmav_reset(rmav_handle h, float *obs_out, int mem, int layout);

/* One step of all N envs.  actions: nA*N floats.  Outputs (each may be NULL): obs_out nS*N floats,
 * rew_out N floats, done_out N bytes (0/1). */
int rmav_step(rmav_handle h, const float *actions, float *obs_out, float *rew_out,
              uint8_t *done_out, int mem, int layout);

/* Geometric controller: actions_out (nA*N floats) <- control(state). */
int rmav_control(rmav_handle h, float *actions_out, int mem, int layout);

/* One iteration of the reference's test loop (test/test_quadrotor3d.py:16-17: action = env.control();
 * env.step(action)) in ONE launch: actions_out (nullable) receives the controller's action, the other outputs
 * are those of rmav_step.  Same results as rmav_control followed by rmav_step. */
int rmav_control_step(rmav_handle h, float *actions_out, float *obs_out, float *rew_out, uint8_t *done_out,
                      int mem, int layout);
/* rmav_step, and the launch ends by evaluating control() on the state it leaves behind: next_actions_out
 * (nA*N floats, required) = what rmav_control would return if called next.  Lets a gym-shaped caller that
 * alternates control() / step(action) pay one launch + one synchronise per iteration (the class caches the
 * action).  Quadrotor kinds only. */
int rmav_step_control(rmav_handle h, const float *actions, float *obs_out, float *rew_out, uint8_t *done_out,
                      float *next_actions_out, int mem, int layout);

/* n_steps steps of all N envs.  fused != 0: one kernel launch with the state held in registers
 * across the steps; fused == 0: n_steps launches of the single-step kernel (same results).
 * actions_in: [n_steps][nA][N] for RMAV_ACT_BUFFER, otherwise ignored (may be NULL).
 * Optional trajectory outputs: actions_out [n_steps][nA][N], obs_out [n_steps][nS][N] (obs after
 * each step, post auto-reset), rew_out [n_steps][N], done_out [n_steps][N]. */
int rmav_rollout(rmav_handle h, int32_t n_steps, int action_mode, const float *actions_in,
                 float *actions_out, float *obs_out, float *rew_out, uint8_t *done_out, int mem,
                 int layout, int fused);

/* rmav_rollout with a column pitch: device pointers, feature-major arrays whose feature columns are `pitch` elements apart -
 * actions_in / actions_out [n_steps][nA][pitch], obs_out [n_steps][nS][pitch], rew_out / done_out [n_steps][pitch]; env i is
 * element i of every column, elements [N, pitch) are never written.  Same results as rmav_rollout.  Keeps the fast store path
 * for batch sizes that are not a multiple of 16.  rmav_trajectory_pitch() = N rounded up to a multiple
 * of 64; any pitch in [N, 2^25] is accepted, a larger one is RMAV_ERR_INVALID (and so is a chunk_envs > N beyond it, which
 * rmav_rollout_chunked turns into a pitch).
 * The one size rule of the trajectory arrays, which also bounds n_envs (rmav_create: n_envs <= 2^25): ONE STEP of the widest
 * array - nS <= 16 columns of 4 * pitch bytes - stays below 2^31 bytes, because the kernels add the offset of a column inside a
 * step in 32 bits.  The number of steps is not bounded by it: an array may exceed 4 GiB (steps are reached with 64-bit pointers,
 * or 32-bit step offsets only while the whole array stays below 4 GiB). */
int64_t rmav_trajectory_pitch(rmav_handle h);
int rmav_rollout_pitched(rmav_handle h, int32_t n_steps, int action_mode, const float *actions_in, float *actions_out,
                         float *obs_out, float *rew_out, uint8_t *done_out, int64_t pitch, int fused);

/* rmav_rollout (fused) with CHUNK-MAJOR trajectory arrays: the env range is cut into chunks of chunk_envs (a multiple of 64; the
 * last one may be shorter) and chunk c's trajectory is a dense array of its own,
 *   actions_in / actions_out [n_chunks][n_steps][nA][chunk_envs], obs_out [n_chunks][n_steps][nS][chunk_envs],
 *   rew_out / done_out [n_chunks][n_steps][chunk_envs]   (env i = chunk i / chunk_envs, column i % chunk_envs; device pointers).
 * Same values as rmav_rollout; one launch per chunk, each writing one dense region - the layout this GPU stores fastest for
 * big quadrotor3d batches (131 072 envs: 0.65 -> 0.78 of the HBM roofline).  rmav_chunk_envs() is the
 * recommended chunk: 65 536 for quadrotor3d beyond 65 536 envs, otherwise N rounded up to a multiple of 64 (one chunk = the
 * plain layout, with that column pitch when N % 64 != 0).  A learner that flattens (step, env) samples - PPO2 does - consumes
 * the chunks as they are.  chunk_envs < N needs n_steps >= 2 and chunk_envs <= the pair kernel's capacity (131 072; 65 536
 * for controller-driven slung-load); RMAV_ACT_BUFFER does not echo the caller's actions (actions_out must be NULL). */
int64_t rmav_chunk_envs(rmav_handle h);
int rmav_rollout_chunked(rmav_handle h, int32_t n_steps, int action_mode, const float *actions_in, float *actions_out,
                         float *obs_out, float *rew_out, uint8_t *done_out, int64_t chunk_envs);

/* ---- state access (also the env checkpoint) ------------------------------------------------ */
int rmav_get_state(rmav_handle h, float *out, int mem, int layout);      /* nS*N floats */
int rmav_set_state(rmav_handle h, const float *in, int mem, int layout);
int rmav_get_sbd(rmav_handle h, int32_t *out, int mem); /* steps_beyond_done per env, -1 = None */
int rmav_set_sbd(rmav_handle h, const int32_t *in, int mem);
int rmav_get_reset_counts(rmav_handle h, uint32_t *out, int mem); /* resets drawn so far per env */
int rmav_set_reset_counts(rmav_handle h, const uint32_t *in, int mem);
int rmav_get_time(rmav_handle h, double *out, int mem);  /* RMAV_REINMAV: per-env clock t (reinmav_env.py:72) */
int rmav_set_time(rmav_handle h, const double *in, int mem);
int rmav_get_step_count(rmav_handle h, uint64_t *out); /* global step counter t */
int rmav_set_step_count(rmav_handle h, uint64_t t);

/* ---- episode statistics (needs RMAV_F_TRACK_EPISODES) -------------------------------------- */
int rmav_episode_totals(rmav_handle h, rmav_ep_totals *out, int clear); /* synchronises */
/* Per-env return / length of the most recently finished episode (0 / 0 if none yet) and of the
 * running episode.  Any pointer may be NULL.  This is the payload of the per-rollout all-gather. */
int rmav_episode_buffers(rmav_handle h, float *last_return, int32_t *last_length,
                         float *cur_return, int32_t *cur_length, int mem);

/* ---- episode time limit (gym's TimeLimit / gym.make(id, max_episode_steps=H), inside the step kernels) ---------------------
 * The reference registers its ids without max_episode_steps (gym_reinmav/__init__.py:3-26): its episodes end only when |pos| or |vel|
 * leaves its box, so a hovering policy's never do.  Auto-reset and the episode statistics run inside the kernels, so the limit lives
 * there too.  Callers detect the feature by these symbols (RMAV_VERSION is unchanged).
 *   - A per-handle limit H (episode length in steps); H = 0 means no limit and is the default: a handle that never sets one behaves
 *     exactly as without this feature.
 *   - An env's running length L counts the steps since its episode began: at creation, at rmav_reset, or after its previous episode
 *     ended.  A step after which L == H and the dynamics did not terminate is TRUNCATED: done = 1 (the done byte stays 0 or 1), the
 *     reward is the step's ordinary -dist, steps_beyond_done is untouched (truncation is not termination), and the episode ends as on
 *     termination - with RMAV_F_TRACK_EPISODES last_return, last_length = H and the totals are updated; with RMAV_F_AUTO_RESET a fresh
 *     state is drawn by the same Philox counter rule and the reset counter advances.
 *   - Termination wins: a step that terminates and reaches H is a termination (reference reward and steps_beyond_done, truncated
 *     flag 0).
 *   - Without RMAV_F_AUTO_RESET a truncation still ends the episode (statistics recorded, the length restarts from 0) but the state
 *     is not reset: the next truncation comes H steps later.  gym's TimeLimit differs here - it reports done on every step after
 *     the limit (stepping past done is undefined behaviour in gym).
 *   - rmav_seed and rmav_set_step_count keep running lengths; rmav_set_state does not restart an episode.
 *   - A handle created without RMAV_F_TRACK_EPISODES keeps no episode starts until it has a limit: rmav_set_time_limit (with H > 0)
 *     starts every env's count at the call, and so does rmav_reset while a limit is set.  Tracking handles keep their exact running
 *     lengths: an env already at or past H when the limit is set is truncated at its next step (L >= H counts as reaching it).
 *   - Launches of a time-limited handle run kernels of their own: fused rollouts use the one-wavefront kernels
 *     (RMAV_TUNE_SPLIT / RMAV_TUNE_SLICE do not apply; a chunk-major call is one launch per chunk), rmav_rollout_policy supports
 *     RMAV_POLICY_FP32_MFMA, RMAV_POLICY_F16_MFMA and RMAV_POLICY_F16_SHARED (the others return RMAV_ERR_INVALID).
 * max_episode_steps in [0, 2^30]; quadrotor kinds only (RMAV_REINMAV ends an episode on every step: RMAV_ERR_INVALID for H > 0). */
int rmav_set_time_limit(rmav_handle h, int32_t max_episode_steps);
int rmav_get_time_limit(rmav_handle h, int32_t *out);
/* N bytes: 1 if the env's most recently finished episode was truncated by the limit, 0 if it terminated or none has finished since
 * the handle first had a limit (written at every episode end of a time-limited handle, tracked or not). */
int rmav_episode_truncated(rmav_handle h, uint8_t *out, int mem);

/* ---- frame skip: hold each action for k dynamics steps ---------------------------------------------------------------------------
 * With k > 1 one AGENT step of an env is up to k ordinary steps of its dynamics (each the same step, reward and steps_beyond_done
 * machine as without a skip) under one action, evaluated once and held; the first termination ends the agent step:
 *     u = the action (for policy rollouts, after the action rule's clip); evaluated ONCE and held
 *     for j = 0 .. k-1:
 *         (s, dist, term) = step(s, u)
 *         r_j = -dist;  if term: r_j = (sbd < 0) ? 1 : 0;  sbd = (sbd < 0) ? 0 : sbd + 1
 *         R = (j == 0) ? r_0 : R + r_j          -- fp32 add, uncontracted, in this order (R = r_0, not 0 + r_0: a -0.0f keeps its sign)
 *         if term: break
 *     obs = s, reward = R, done = term
 * Everything above the dynamics counts agent steps:
 *   - the step counter t (rmav_get_step_count) advances by 1 per agent step; the random-action and policy-noise streams draw once per
 *     agent step; last_length, length_sum, running lengths and the time limit H are in agent steps;
 *   - truncation is tested once, after the loop (termination wins); the running return adds R;
 *   - the auto-reset, and the redraw of a ranged handle's constants, happen once, after the agent step: the old episode's constants
 *     hold for all of its sub-steps.  Without RMAV_F_AUTO_RESET a finished env executes one sub-step per agent step (it terminates at
 *     once; sbd advances by 1);
 *   - rmav_step_final reports the state after the last executed sub-step; rmav_rollout_policy_boot / _norm leave V of that state in
 *     boot_out where the agent step was truncated; value_out[t] / logp_out[t] belong to the agent step: the actor runs once per agent step;
 *   - RMAV_ACT_CONTROLLER and rmav_control_step evaluate control() once per agent step and hold it (zero-order hold);
 *     rmav_step_control returns RMAV_ERR_INVALID on such a handle (call rmav_control and rmav_step).
 * Launches of such a handle run kernels of their own: fused rollouts use the one-wavefront kernels, as for a
 * ranged handle (the split, slice, step-lazy and step-store tuning keys do not apply; a chunk-major call is one launch per chunk;
 * fused = 0 gives the bits of fused = 1; results never depend on the store policy); rmav_rollout_policy / _boot / _norm accept
 * RMAV_POLICY_FP32_MFMA, RMAV_POLICY_F16_MFMA and RMAV_POLICY_F16_SHARED (the others return RMAV_ERR_INVALID).
 * The setting is host state only: no launch, no synchronisation.  k is a kernel argument, so a captured graph keeps the value it was
 * captured with.  A handle with k = 1 - also one set back to 1 - launches exactly the kernels it launched before.  Quadrotor kinds
 * only (RMAV_REINMAV already sub-steps: RMAV_ERR_INVALID for k > 1).  Callers detect the feature by the symbols; RMAV_VERSION is
 * unchanged. */
int rmav_set_frame_skip(rmav_handle h, int32_t k);   /* k in [1, 1024]; 1 = none, the default */
int rmav_get_frame_skip(rmav_handle h, int32_t *out);

/* ---- tracking reward: goal, costs, alive bonus --------------------------------------------------------------------------------------
 * With a spec set the reward of every ordinary dynamics step of a quadrotor handle is, in place of the reference's -|pos| / first-
 * termination literal,
 *     e_i = P_i - goal_i
 *     d = root(fma(e0,e0, fma(e1,e1, e2*e2)))        (2-D kinds: root(fma(e0,e0, e1*e1)); the root() of the step norms)
 *     v = the same expression over V
 *     c = the same fma chain, without the root, over (u_c - act_ref_c), c = 0 .. nA-1 (the last component is the plain product)
 *     r_live = fma(-w_act, c, fma(-w_vel, v, fma(-w_pos, d, alive)))
 *     r = terminated ? terminal : r_live
 * in fp32 on the STORED post-step state, uncontracted except where fma is written.  P / V are the position / velocity of the tracked
 * body - the one whose distance the reference rewards: quadrotor2d s[0:2] / s[3:5]; quadrotor2d-slungload (the quadrotor) s[0:2] /
 * s[3:5]; quadrotor3d s[0:3] / s[7:10]; quadrotor3d-slungload (the load) s[10:13] / s[13:16].  u is the action handed to the dynamics:
 * for policy rollouts after the action rule's clip (the stored action stays unclipped), for the 2-D kinds before thrust_scale, for
 * rmav_control_step and RMAV_ACT_CONTROLLER the controller's action.
 *   - steps_beyond_done advances exactly as without a spec (it is state); `terminal` does not depend on it.  The state, done, the
 *     truncated flags, the reset stream and the constants of a ranged handle never depend on the spec.
 *   - everything that consumes the step's reward consumes this r: a truncated step has not terminated and gets r_live; the running
 *     return, last_return and the episode totals add r; under frame skip r_j is this r per sub-step and R sums as the frame-skip
 *     contract states (c is computed once per agent step: the action is held).  rmav_gae*, rmav_ret_*, rmav_normalize and the
 *     statistics exchange read stored rewards and need no change.
 *   - with goal = 0, alive = 0, w_pos = 1, w_vel = w_act = 0 every non-terminating step has the bits of the reference's reward.
 * Launches of such a handle run kernels of their own, the frame-skip kernels' restrictions apply: fused rollouts
 * use the one-wavefront kernels (the split, slice, step-lazy and step-store tuning keys do not apply; a chunk-major call is one launch
 * per chunk; fused = 0 gives the bits of fused = 1; results never depend on the store policy); rmav_step_control is k_step's launch
 * followed by rmav_control's (with a frame skip k > 1 it stays RMAV_ERR_INVALID); rmav_rollout_policy / _boot / _norm accept
 * RMAV_POLICY_FP32_MFMA, RMAV_POLICY_F16_MFMA and RMAV_POLICY_F16_SHARED (the others return RMAV_ERR_INVALID).
 * Every value must be finite (RMAV_ERR_INVALID otherwise); RMAV_REINMAV takes no spec (RMAV_ERR_INVALID for a non-NULL one).  NULL
 * switches back to the reference's reward: such a handle, like one that never set a spec, launches exactly the kernels it launched before.
 * Ordering: rmav_set_reward is ordered on the handle's stream - launches enqueued after it see the new spec - and neither
 * synchronises nor allocates (the device copy is part of the handle since rmav_create).  The step and one-wavefront rollout kernels take the spec by value: a captured graph keeps the values it was captured
 * with.  The policy rollouts read the handle's device copy, which rmav_set_reward rewrites with a small launch on the stream: a
 * captured graph reads, at replay, whatever the copy holds then (a set captured into the graph is replayed with it).
 * rmav_get_reward: the last spec set (zeros before the first), and whether it is in force; either pointer may be NULL.
 * Callers detect the feature by the symbols; RMAV_VERSION is unchanged. */
typedef struct rmav_reward_spec {
    float goal[3];      /* 2-D kinds read [0..1] */
    float alive;        /* added on every non-terminating step */
    float w_pos, w_vel, w_act;
    float act_ref[4];   /* 2-action kinds read [0..1] */
    float terminal;     /* the reward of a terminating step */
} rmav_reward_spec;
int rmav_set_reward(rmav_handle h, const rmav_reward_spec *spec);   /* NULL: back to the reference's reward */
int rmav_get_reward(rmav_handle h, rmav_reward_spec *out, int32_t *enabled);   /* either pointer may be NULL */

/* ---- wind and gust disturbances ---------------------------------------------------------------------------------------------------
 * With a spec set every env of a quadrotor handle is pushed by an external acceleration d, added to rmav_params.g_vec per env and per
 * agent step inside the step kernels (streams "wind" and "gust" of the RNG table above):
 *     w_i = fma(wind_hi_i - wind_lo_i, u(W_i), wind_lo_i)     per episode; the span is one fp32 subtraction
 *     q_i = fma(gust_i + gust_i, u(G_i), -gust_i)             per block of gust_hold agent steps of the handle's step counter
 *     d_i = w_i + q_i                                          fp32, uncontracted, in this order
 * and every use of g_vec_i in the dynamics reads g_vec_i + (R)d_i, R being the kind's arithmetic type (fp32 for the plain kinds, fp64 for
 * the slung-load kinds, both bodies).  control() in all its forms - rmav_control, rmav_control_step, RMAV_ACT_CONTROLLER, the trailing
 * control() of rmav_step_control - keeps the undisturbed g_vec: the controller does not know the wind.
 *   - d is a pure function of (seed, global env id, the running episode's reset index, the step counter t, the spec): shard-invariant,
 *     and a checkpoint is the spec alone.  rmav_seed, rmav_set_reset_counts and rmav_set_step_count move d exactly as they move the
 *     streams they already move.  Under frame skip one d holds for all sub-steps of an agent step.
 *   - the wind changes exactly when the reset index does: at rmav_reset and at every in-kernel auto-reset, by termination or truncation;
 *     the step that ends an episode uses the old wind.
 *   - nothing else depends on the spec: reward formulae, done thresholds, the reset, action, noise and constants streams, observations
 *     (the disturbance is not observed).
 *   - an all-zero spec gives d = +0, and g_vec + 0 has the bits of g_vec: such a handle stores the bits of one without a spec.
 *   - rmav_disturbance_now: d of every env's NEXT step, [3][N] floats (row 2 is 0 for the 2-D kinds); RMAV_ERR_INVALID without a spec.
 * Launches of such a handle run kernels of their own, as those of a handle with a tracking reward: fused rollouts use
 * the one-wavefront kernels (the split, slice, step-lazy and step-store tuning keys do not apply; a chunk-major call is one launch per
 * chunk; fused = 0 gives the bits of fused = 1).  The disturbed fused rollouts are built for ONE store policy: RMAV_TUNE_STORE_POLICY does not
 * apply either, and results never depend on the store policy.  rmav_step_control is the step kernel's launch followed by rmav_control's
 * (with a frame skip k > 1 it stays RMAV_ERR_INVALID).  rmav_rollout_policy / _boot / _norm run the three actors a frame skip runs
 * (RMAV_POLICY_FP32_MFMA, RMAV_POLICY_F16_MFMA, RMAV_POLICY_F16_SHARED); the other precisions return RMAV_ERR_INVALID.
 * Validation: every value finite, wind_lo <= wind_hi, gust >= 0, gust_hold in [1, 1048576]; otherwise RMAV_ERR_INVALID.  RMAV_REINMAV takes
 * no spec (RMAV_ERR_INVALID for a non-NULL one).  NULL switches the disturbance off: such a handle, like one that never set a spec, launches
 * exactly the kernels it launched before.
 * Ordering and capture as rmav_set_reward: the step kernels and the one-wavefront rollouts take the spec by value; the policy kernels read a
 * device copy in the handle's arena, which rmav_set_disturbance rewrites in stream order with one small launch.  Launches enqueued after a
 * set see the new spec, a captured graph keeps the values (and the step counter) it was captured with, and a set neither allocates nor
 * synchronises.
 * rmav_get_disturbance: the last spec set (zeros before the first), and whether it is in force; either pointer may be NULL.
 * Callers detect the feature by the symbols; RMAV_VERSION is unchanged. */
typedef struct rmav_disturbance_spec {
    float wind_lo[3], wind_hi[3]; /* per-episode constant acceleration, component i ~ U[lo_i, hi_i], m/s^2; 2-D kinds read [0..1] */
    float gust[3];                /* gust amplitude per axis, >= 0: component i ~ U[-gust_i, gust_i) */
    int32_t gust_hold;            /* agent steps one gust value is held, 1 .. 1048576 */
} rmav_disturbance_spec;          /* 40 bytes */
int rmav_set_disturbance(rmav_handle h, const rmav_disturbance_spec *spec);   /* NULL: none (the default) */
int rmav_get_disturbance(rmav_handle h, rmav_disturbance_spec *out, int32_t *enabled);   /* either pointer may be NULL */
int rmav_disturbance_now(rmav_handle h, float *out, int mem);   /* [3][N] floats: d of every env's NEXT step; row 2 is 0 for 2-D kinds */

/* ---- sensor noise: Gaussian observation noise drawn inside the kernels --------------------------------------------------------------
 * With a spec set every OBSERVATION a quadrotor handle emits for an env is, per component c, in fp32 (stream "sensor" of the RNG table
 * above):
 *     o_c = fma(sigma_c, z_c, s_c)
 * s being the true state the observation reports and z standard normal.  b, the block's step counter, is the handle's step counter (agent
 * steps) AFTER the operation that produced the observation: a step that moves t -> t+1 emits observations with b = t+1, rmav_reset and
 * rmav_observe use b = t.  An observation is therefore a pure function of (seed, global env id, state, step counter, spec): shard-invariant,
 * stateless, and a checkpoint is the spec alone.  ONE rule ties every route together: what an operation emits for an env has the bits of
 * rmav_observe called right after it.
 *   - noisy: obs_out of rmav_reset / rmav_step / rmav_control_step / rmav_step_control / rmav_step_final and of rmav_rollout / _pitched /
 *     _chunked in all three action modes, fused and unfused; final_obs_out of rmav_step_final (s = the pre-reset state, under the SAME z as
 *     the post-reset observation of that step).
 *   - not noisy: the dynamics, done, rewards (the tracking reward reads the true state), episode statistics, every other stream,
 *     rmav_get_state, and control() in all its forms (the reference controller reads the state).  A handle with a spec and caller, random
 *     or controller actions leaves every non-observation output and its state bit-identical to a twin without one.
 *   - sigma_c = 0 gives o_c == s_c bit for bit, except that a -0.0 may come out as +0.0 (fma(0, z, -0.0) is +0.0 when 0 * z is +0.0).  An
 *     all-zero spec stores the values of a handle without one.
 *   - rmav_observe: the observation of every env's current state at b = t, nS*N floats, both mem values and both layouts.  On a handle
 *     without a spec it has the bits of rmav_get_state.
 * Launches of such a handle run kernels of their own, cut from the disturbed ones, whose launch rules they share: the
 * one-wavefront fused rollouts with ONE store policy (the split, slice, step-lazy, step-store and store-policy tuning keys do not apply; a
 * chunk-major call is one launch per chunk; fused = 0 gives the bits of fused = 1); a handle without a disturbance passes the all-zero
 * disturbance, whose d = +0 leaves g_vec's bits.  rmav_step_control is the step kernel's launch followed by rmav_control's.
 * rmav_rollout_policy / _boot / _norm run the three actors a disturbance runs (RMAV_POLICY_FP32_MFMA, RMAV_POLICY_F16_MFMA,
 * RMAV_POLICY_F16_SHARED): the input of every policy- and value-net evaluation - value_out[n_steps] and the bootstrap V(s_final) included,
 * in front of the normaliser when there is one - and the stored obs_out are the noisy observation (what the actor reads at step k of a
 * launch that started at t0 is rmav_observe at b = t0 + k, the row the previous step or launch stored); the dynamics run from the true
 * state.  The other precisions return RMAV_ERR_INVALID with a message that names the feature.
 * Validation: every sigma_c finite and >= 0, sigma_c == 0 for c >= nS; RMAV_REINMAV takes no spec; anything else is RMAV_ERR_INVALID and
 * the spec in force stays.  NULL switches the feature off: such a handle, like one that never set a spec, launches exactly the kernels it
 * launched before.
 * Ordering and capture as rmav_set_reward: the step kernels, the one-wavefront rollouts and rmav_observe's kernel take the spec by value; the
 * policy kernels read a device copy in the handle's arena, which rmav_set_sensor_noise rewrites in stream order with one small launch.
 * Launches enqueued after a set see the new spec, a captured graph keeps the values (and the step counter) it was captured with, and a
 * set neither allocates nor synchronises.
 * rmav_get_sensor_noise: the last spec set (zeros before the first), and whether it is in force; either pointer may be NULL.
 * Callers detect the feature by the symbols; RMAV_VERSION is unchanged. */
typedef struct rmav_sensor_noise_spec {
    float sigma[16];              /* standard deviation per observation component; only components < nS are used, the others must be 0 */
} rmav_sensor_noise_spec;         /* 64 bytes */
int rmav_set_sensor_noise(rmav_handle h, const rmav_sensor_noise_spec *spec);   /* NULL: none (the default) */
int rmav_get_sensor_noise(rmav_handle h, rmav_sensor_noise_spec *out, int32_t *enabled);   /* either pointer may be NULL */
int rmav_observe(rmav_handle h, float *obs_out, int mem, int layout);   /* nS*N floats: the observation of the current state at b = t */

/* ---- actuator lag: a first-order motor model between the commanded action and the dynamics -----------------------------------------
 * With a spec set every env of a quadrotor handle carries an actuator state m[nA] in fp32, and the dynamics read m, not the commanded
 * action u.  Per ordinary dynamics step (every sub-step of a frame skip), per component c:
 *     m_c = fma(alpha_c, u_c, beta_c * m_c)      fp32; the product beta_c * m_c is rounded on its own, then one fma
 *     (s, dist, term) = step(s, m)
 * alpha_c = 1 - exp(-dt / tau_c) and beta_c = exp(-dt / tau_c): the host computes both in fp64 from the spec's tau_c (seconds) and the
 * rmav_params.dt in force when the launch is enqueued, rounds each to fp32 once and passes them to the kernels as values;
 * rmav_set_params with a new dt re-derives them for later launches.  tau_c = 0 gives alpha = 1, beta = 0 and m_c = fma(1, u_c, 0 * m_c)
 * = u_c: a handle whose every tau is 0 stores the bits of a handle without a spec (a -0.0 action may act as +0.0, as sigma = 0 of the
 * sensor noise).  No random stream is involved: the RNG table above is unchanged.
 *   - u is the action handed to the dynamics without the feature: the caller's or the random action, the controller's in all its forms
 *     (RMAV_ACT_CONTROLLER, rmav_control_step), and for the policy rollouts the action after the action rule's clip.  For the 2-D kinds the
 *     filter acts on the raw action; thrust_scale and clamp_thrust stay inside the step and act on m.
 *   - nothing else reads m: stored actions, logp and the tracking reward's action cost c (still once per agent step) read u; rmav_control
 *     returns the command; m is not observed (rmav_state_dim and the observation rows are unchanged).
 *   - episodes: m_c = init_c for every env at the moment the feature is switched on, at rmav_reset, and at every in-kernel auto-reset by
 *     termination or truncation.  The step that ends an episode runs with the old m - inside a frame skip m stops advancing with the
 *     sub-step that terminates - and the first step of the next episode filters from init.  Without RMAV_F_AUTO_RESET only rmav_reset
 *     re-initialises.  A set on a handle whose spec is in force changes tau and init and keeps the running m.
 *   - state: m lives in a [nA][N] device array of the handle, like the per-env constants: loaded at the head of every launch, held in
 *     registers through a fused rollout and stored at its end; the single-step kernels update it in place.  A checkpoint is the spec plus
 *     rmav_get_actuator_state / rmav_set_actuator_state (nA*N floats, both mem values, both layouts); rmav_seed, rmav_set_state,
 *     rmav_set_reset_counts and rmav_set_step_count do not touch it.  Because m is in memory and alpha / beta are launch values, a
 *     captured graph advances m correctly at replay and keeps the alpha / beta it was captured with.
 * Launches of such a handle run kernels of their own, cut from the noisy ones, whose launch rules they share: the
 * one-wavefront fused rollouts with ONE store policy (fused = 0 gives the bits of fused = 1; a chunk-major call is one launch per chunk); a
 * handle without sensor noise skips the noise draw, one without a disturbance passes the all-zero one.  rmav_step_control is the step
 * kernel's launch followed by rmav_control's (refused with a frame skip above 1, as ever).  rmav_rollout_policy / _boot / _norm run the
 * three actors the sensor noise runs (RMAV_POLICY_FP32_MFMA, RMAV_POLICY_F16_MFMA, RMAV_POLICY_F16_SHARED); the other precisions return
 * RMAV_ERR_INVALID with a message that names the feature.
 * Validation: every tau_c finite and >= 0, every init_c finite, components >= nA zero; RMAV_REINMAV takes no spec; anything else is
 * RMAV_ERR_INVALID and the spec in force stays.  NULL switches the feature off and frees nothing observable: such a handle, like one that
 * never set a spec, launches exactly the kernels it launched before.
 * Ordering and capture as rmav_set_sensor_noise: the step kernels and the one-wavefront rollouts take alpha / beta / init by value; the
 * policy kernels read a device copy in the handle's arena, which rmav_set_actuator (and rmav_set_params) rewrites in stream order with one
 * small launch.  The first rmav_set_actuator on a handle allocates the [nA][N] array; every set that switches the feature on fills it
 * with init in stream order; later sets neither allocate nor synchronise.
 * rmav_get_actuator: the last spec set (zeros before the first), and whether it is in force; either pointer may be NULL.
 * Callers detect the feature by the symbols; RMAV_VERSION is unchanged. */
typedef struct rmav_actuator_spec {
    float tau[4];                 /* time constant per action component, seconds; 0 = no lag; 2-action kinds read [0..1], the others must be 0 */
    float init[4];                /* m at the start of every episode */
} rmav_actuator_spec;             /* 32 bytes */
int rmav_set_actuator(rmav_handle h, const rmav_actuator_spec *spec);   /* NULL: none (the default) */
int rmav_get_actuator(rmav_handle h, rmav_actuator_spec *out, int32_t *enabled);   /* either pointer may be NULL */
int rmav_get_actuator_state(rmav_handle h, float *out, int mem, int layout);   /* nA*N floats; RMAV_ERR_INVALID without a spec */
int rmav_set_actuator_state(rmav_handle h, const float *in, int mem, int layout);   /* RMAV_ERR_INVALID without a spec */

/* ---- start-state ranges: the per-component distribution of every fresh state --------------------------------------------------------
 * The reference's reset() draws EACH state component as U[-1, 1): a random attitude and up to 1 m/s on every axis.  With a spec set every
 * fresh state a quadrotor handle draws is, per component c, in fp32:
 *     v_c = the value the "reset" stream of the RNG table gives today (same counters, same words; v_c = fma(2^-23, x >> 8, -1))
 *     s_c = fma(h_c, v_c, m_c),   h_c = (hi_c - lo_c) / 2,   m_c = (hi_c + lo_c) / 2
 * The host computes h_c and m_c in fp64 from the spec's fp32 values, rounds each to fp32 once and passes them to the kernels as values.
 * No random stream is added.  A start state is a pure function of (seed, global env id, reset index, spec): shard-invariant, and a
 * checkpoint is the spec alone.  lo_c == hi_c pins component c to that value; the map is the fma of the ROUNDED h and m, not a clamp, so where
 * the midpoint is not representable a state can leave [lo_c, hi_c] by that rounding (half an ulp of the larger bound).  The identity spec (lo = -1, hi = 1 below nS) gives h = 1,
 * m = 0 and fma(1, v, 0) = v: such a handle stores, in every route, the bits of a handle without a spec.
 *   - applies everywhere a fresh state is drawn: at rmav_reset, at every in-kernel auto-reset by termination or by time-limit truncation,
 *     in the spare state a fused launch draws up front (n_steps >= 8) and in the on-demand draw of a second termination inside one launch.
 *   - applies nowhere else: the dynamics, rewards, done, steps_beyond_done, reset counts and every other stream (action, policy noise, env
 *     constants, wind, gust, sensor) are unchanged functions of their inputs; rmav_step_final's final_obs_out is the pre-reset state, as
 *     ever; rmav_set_state, rmav_seed, rmav_set_reset_counts and rmav_set_step_count do not consult the spec.  With sensor noise the
 *     observation a reset emits is the noisy observation of the mapped state.
 *   - rmav_set_start_state is host state plus the device copy below: it draws NOTHING and does not touch the running episodes, which were
 *     drawn under whatever was in force when they began (rmav_create has drawn reset 0 with the reference's rule: call rmav_reset behind the
 *     set to start every env under the spec, at reset index 1).
 * Launches of such a handle run kernels of their own, cut from the lagged ones, whose launch rules they share: the
 * one-wavefront fused rollouts with ONE store policy (fused = 0 gives the bits of fused = 1; a chunk-major call is one launch per chunk);
 * rmav_reset runs k_reset_ss.  A handle without actuator lag passes a wave-uniform flag that GATES the filter: the kernels then neither
 * load nor store a filter state and hand the command itself to the dynamics - a -0.0 action keeps its sign, no handle-owned m exists, and
 * rmav_get_actuator_state stays refused.  One without sensor noise skips the draw, one without a disturbance passes the all-zero one.
 * rmav_rollout_policy / _boot / _norm run the three actors the actuator lag runs (RMAV_POLICY_FP32_MFMA, RMAV_POLICY_F16_MFMA,
 * RMAV_POLICY_F16_SHARED); the other precisions return RMAV_ERR_INVALID with a message that names the feature.
 * Validation: every value finite, lo_c <= hi_c, components >= nS zero; RMAV_REINMAV takes no spec (its reset() is a no-op); anything else
 * is RMAV_ERR_INVALID and the spec in force stays.  NULL switches the feature off: such a handle, like one that never set a spec, launches
 * exactly the kernels it launched before.
 * Ordering and capture as rmav_set_reward: the step kernels, the one-wavefront rollouts and k_reset_ss take h / m by value; the policy
 * kernels read a device copy in the handle's arena, which rmav_set_start_state rewrites in stream order with one small launch.  It neither
 * allocates nor synchronises.
 * rmav_get_start_state: the last spec set (zeros before the first), and whether it is in force; either pointer may be NULL.
 * Callers detect the feature by the symbols; RMAV_VERSION is unchanged. */
typedef struct rmav_start_state_spec {
    float lo[16], hi[16];         /* per state component; components >= nS must be 0 */
} rmav_start_state_spec;          /* 128 bytes */
int rmav_set_start_state(rmav_handle h, const rmav_start_state_spec *spec);   /* NULL: the reference's U[-1,1) (the default) */
int rmav_get_start_state(rmav_handle h, rmav_start_state_spec *out, int32_t *enabled);   /* either pointer may be NULL */

/* ---- termination rules: a per-axis position box, a tilt limit and a finiteness test ----------------------------------------------------
 * The reference's native envs end an episode on |pos| > pos_limit || |vel| > vel_limit: a sphere round the origin.  Its MuJoCo hovering task
 * (gym_reinmav/envs/mujoco/mujoco_quad_hovering.py:55-60) ends on a per-axis box and a finiteness test instead - isfinite(ob).all() and
 * ob[2] > 0.3 and |ob[0]| < 2 and |ob[1]| < 2 - and its two MuJoCo base envs on not isfinite(ob).all().  With a spec set the termination flag of
 * EVERY ordinary dynamics step of a quadrotor handle - every sub-step of a frame skip - is
 *     term = term_ref || rule(s)
 * term_ref what the step computes without a spec, s the stored post-step fp32 state.  The rule is fp32, nothing contracted but the fmas written:
 *     nonfinite = any c < nS: !(|s_c| < inf)
 *     outside   = any body B, any axis i < dim: !(B_i >= pos_lo_i) || !(B_i <= pos_hi_i)
 *                 bodies: the quadrotor s[0:dim]; for the slung-load kinds also the load (s[5:7] / s[10:13]).  Walls and floor apply to both.
 *     tilted    = 2-D kinds:  |s[2]| > max_tilt                        (the angle is never wrapped)
 *                 3-D kinds:  fma(w,w, fma(z,z, -fma(x,x, y*y))) < c * fma(w,w, fma(x,x, fma(y,y, z*z)))
 *                             (w,x,y,z) = s[3:7];  c = (float)cos((double)max_tilt), computed on the host and rounded once;
 *                             max_tilt = +inf passes c = -inf, which never fires
 *     rule      = nonfinite || outside || tilted
 * The 3-D tilt test is the world-z component of the body's z axis against cos(max_tilt), both sides multiplied by |q|^2: no division, no
 * reciprocal square root.
 *   - nothing downstream changes: the reward machine (the reference literal or the tracking reward's `terminal`), steps_beyond_done, the
 *     frame-skip break, "termination wins over truncation" and trunc = 0, the actuator re-initialisation, the redraw of ranged constants and
 *     wind, the auto-reset and the start-state map, the episode statistics and rmav_step_final's final_obs_out (the pre-reset state) see ONE
 *     term, as before.
 *   - nothing else depends on the spec: dist, the dynamics, every RNG stream and control() are unaffected.  The feature adds no stream and no
 *     per-env state: a checkpoint is the spec alone.
 *   - the rule is evaluated on states a step produces: rmav_reset, rmav_set_state and a fresh state are not tested.  A set takes effect with
 *     the next step.
 *   - identity: a spec with all bounds infinite and max_tilt = +inf differs from no spec only in `nonfinite`; on finite trajectories such a
 *     handle stores, in every route, the bits of a handle without one.
 * Launches of such a handle run kernels of their own, cut from those of a start-state spec, whose launch rules they
 * share: the one-wavefront fused rollouts with ONE store policy (fused = 0 gives the bits of fused = 1; a chunk-major call is one launch per
 * chunk).  A handle without a start-state spec passes the identity coefficients (h = 1, m = 0: the plain bits), one without actuator lag the
 * flag that gates the filter, one without sensor noise skips the draw, one without a disturbance passes the all-zero one.  rmav_reset runs
 * what it ran before.  rmav_rollout_policy / _boot / _norm run the three actors the start-state spec runs (RMAV_POLICY_FP32_MFMA,
 * RMAV_POLICY_F16_MFMA, RMAV_POLICY_F16_SHARED); the other precisions return RMAV_ERR_INVALID with a message that names the feature.
 * Validation: no NaN anywhere, pos_lo_i <= pos_hi_i, max_tilt in [0, pi] (pi as fp32 rounds it) or +inf, _reserved 0; RMAV_REINMAV takes no
 * spec; anything else is RMAV_ERR_INVALID and the spec in force stays.  NULL switches the feature off: such a handle, like one that never
 * set a spec, launches exactly the kernels it launched before.
 * Ordering and capture as rmav_set_start_state: the step kernels and the one-wavefront rollouts take the thresholds by value; the policy
 * kernels read a device copy in the handle's arena, which rmav_set_termination rewrites in stream order with one small launch
 * (k_set_termination).  It neither allocates nor synchronises.
 * rmav_get_termination: the last spec set (zeros before the first), and whether it is in force; either pointer may be NULL.
 * Callers detect the feature by the symbols; RMAV_VERSION is unchanged. */
typedef struct rmav_termination_spec {
    float pos_lo[3], pos_hi[3];  /* per-axis box, metres; -inf / +inf = no bound on that side; 2-D kinds read [0..1] */
    float max_tilt;              /* radians in [0, pi], or +inf = none */
    int32_t _reserved;           /* must be 0 */
} rmav_termination_spec;         /* 32 bytes */
int rmav_set_termination(rmav_handle h, const rmav_termination_spec *spec);   /* NULL: the reference's rule alone (the default) */
int rmav_get_termination(rmav_handle h, rmav_termination_spec *out, int32_t *enabled);   /* either pointer may be NULL */

/* ---- what the auto-reset destroys: terminal observations and truncated flags ----------------------------------------------------
 * With RMAV_F_AUTO_RESET every observation a caller sees for a finished env is the fresh post-reset state.  A learner that
 * bootstraps a truncated episode (target r + gamma V(s_final): a truncated episode is not a failure) needs the state the dynamics
 * left BEFORE the reset - gym VecEnvs' info['terminal_observation'].  Callers detect the feature by this symbol (RMAV_VERSION is
 * unchanged); a caller that never calls it runs exactly the kernels it ran before.
 *
 * rmav_step, plus:
 *   final_obs_out  nS*N floats in `layout`; written ONLY for envs whose episode ended with this step (done = 1): the state after the
 *                  dynamics, before the reset.  Other envs' elements are left untouched (with RMAV_HOST too).  Terminated episodes
 *                  report their terminal state as well as truncated ones.
 *   trunc_out      N bytes, written for every env: 1 if the time limit ended the episode with this step, else 0.
 * Either may be NULL.  Works on every quadrotor handle: without RMAV_F_AUTO_RESET final_obs equals the obs of the finished envs;
 * without a time limit trunc_out is all zero.  RMAV_HOST and RMAV_DEVICE, both layouts.  obs, rew, done, the state, the episode
 * records and statistics are bit-identical to rmav_step's.  RMAV_REINMAV (takes no limit, never resets): RMAV_ERR_INVALID. */
int rmav_step_final(rmav_handle h, const float *actions, float *obs_out, float *rew_out, uint8_t *done_out,
                    float *final_obs_out, uint8_t *trunc_out, int mem, int layout);

#ifdef __cplusplus
}
#endif

/* The two extensions of the path, each in its own header (included here, so that `#include "rmav.h"` declares everything):
 *   rmav_ppo.h   SURVEY 8(f1): the PPO2 rollout loop with the policy inside the kernel, GAE, advantage normalisation
 *   rmav_comm.h  SURVEY 8(e): the path's one collective - the all-gather of per-env episode statistics over RCCL / xGMI */
#include "rmav_ppo.h"
#include "rmav_comm.h"

#endif /* RMAV_H */

// rmav_pair_dynamics.inc - one env-step of the stepping wavefront once its action is known: the dynamics, the reward /
// steps_beyond_done machine and the head of the time limit, in the step loop of both pair bodies.
//   expects:  K, NA, the constexpr bools TL, NORM and FS, the kernel arguments ar (ActRuleArgs), - FS - fs (FrameSkipArgs) and - TL - tl (TimeLimitArgs); act[NA] (the
//             action the policy drew), p, li, el
//             - RMAV_PAIR_DS - pl, p_shared, ds_w, ds_q: pl.gv is rewritten to g_vec + d in front of the agent step
//   defines:  dist, r (the step's reward), done (terminated or - TL - truncated)
//   modifies: s (the state after the step), tenv (REINMAV), sb; stores one byte of tl.last_trunc where an episode ends (TL)
//   leaves OPEN: the block of its last statement, `if constexpr (TL) {`, with `const bool trunc` (this lane's episode ran into the limit
//             in this step) declared in it.  The includer follows the include with its BOOT part, which needs trunc and differs between
//             the two bodies, and closes the block.  (Declaring trunc in front of the block instead, so that the fragment could close
//             it, changed the register numbering of two kernels WITHOUT a time limit: profiles/r15/body_fragments.md.)
//   barriers: none (between X(k) / B(k - 1) and the barrier that ends step k)
        float dist = 0.0f, r;
        bool done;
        if constexpr (K == REINMAV) {
            float fm0[4];
            Env<K>::step(s, act, false, tenv, p, fm0);
            done = true;   // reinmav_env.py:110
            r = 90.0f;     // reinmav_env.py:111-116
        } else {
#if RMAV_PAIR_DS   // the disturbance of this agent step (one d for all of its sub-steps): the lane's gravity is g_vec + (w + q)
            disturb_apply(pl, p_shared, ds_w, ds_q);
#endif
            if constexpr (FS) {
                // frame skip (FrameSkipArgs, see k_rollout_fs): the clipped action is held for up to fs.k sub-steps, the reward machine runs
                // behind each; closed HERE, in front of the time limit - between the same two barriers as the single step
                float ca[NA];
#pragma unroll
                for (int c = 0; c < NA; ++c) ca[c] = NORM ? act_clip(ar, act[c]) : act[c];
                [[maybe_unused]] float c_rw = 0.0f;   // RW: the action cost of the agent step - the action is held, so once
                if constexpr (RW) c_rw = reward_act_cost<K>(ca, rw);
                bool live = true;
                done = false;
                r = 0.0f;
                int32_t j = 0;
                do {
                    if (live) {
                        bool term;
#if RMAV_PAIR_AL   // actuator lag: the filter advances in front of every dynamics sub-step, which reads m; c_rw and the stored action keep the command
                        actuator_step<NA>(alc, am, ca);
#if RMAV_PAIR_SS   // (a start spec without actuator lag: the command itself - a select, as in rmav_rollout_body.inc)
#pragma unroll
                        for (int c = 0; c < NA; ++c) am[c] = al_live ? am[c] : ca[c];
#endif
                        Env<K>::step(s, am, p, dist, term);
#else
                        Env<K>::step(s, ca, p, dist, term);
#endif
#if RMAV_PAIR_TC   // the termination rules (tc: TermArgs; rmav_term.hpp): one flag for everything downstream
                        term = term || term_rule<K>(s, tc);
#endif
                        float rj = -dist;
                        if constexpr (RW) {   // the tracking reward (RewardArgs) in the literal's place; steps_beyond_done advances as ever
                            rj = reward_rw<K>(s, c_rw, rw, term);
                            if (term) sb = (sb < 0) ? 0 : sb + 1;
                        } else if (term) {
                            rj = (sb < 0) ? 1.0f : 0.0f;
                            sb = (sb < 0) ? 0 : sb + 1;
                        }
                        r = (j == 0) ? rj : r + rj;
                        done = term;
                        live = !term;
                    }
                    ++j;
                } while (j < fs.k && __ballot(live) != 0);
            } else {
            if constexpr (NORM) {   // the action rule: the dynamics take the clipped action, the stored one stays what the policy drew
                float ca[NA];
#pragma unroll
                for (int c = 0; c < NA; ++c) ca[c] = act_clip(ar, act[c]);
                Env<K>::step(s, ca, p, dist, done);
            } else {
                Env<K>::step(s, act, p, dist, done);
            }
            r = -dist;     // reward / steps_beyond_done machine  (quadrotor3d.py:112-122 and siblings)
            if (done) {
                r = (sb < 0) ? 1.0f : 0.0f;
                sb = (sb < 0) ? 0 : sb + 1;
            }
            }
        }
        // time limit (see k_rollout): after the reward / steps_beyond_done machine, before the episode hand-off
        if constexpr (TL) {
            const bool trunc = !done && el + 1 >= tl.max_steps;
            done = done || trunc;
            if (done) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(trunc ? 1 : 0), make_rsrc(tl.last_trunc), li, 0, 0);

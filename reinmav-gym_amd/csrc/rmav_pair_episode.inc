// rmav_pair_episode.inc - the end of one env-step of the stepping wavefront: episode bookkeeping, auto-reset (with the redraw of a
// ranged handle's constants) and the hand-over of the step's outputs to the helper wavefront, in the step loop of both pair bodies.
// A field added to the reset goes HERE (and its spare, if it has one, into rmav_pair_env_load.inc): both kernels are served.
//   expects:  K, NS, NA, PT (PairTile), the constexpr bools TL and BOOT, the preprocessor flag RMAV_PAIR_DR (see rmav_pair_env_load.inc),
//             the kernel arguments a, pc_shared and - RMAV_PAIR_DR - dr; otile (this lane's word of the pair's output tile), k, r, done
//             (after the time limit), act[NA], env_id, li, off, valid, track, auto_reset
//   defines:  row (the output row of step k: half k & 1 of the tile)
//   modifies: er, el, fin_n, fin_len, fin_ret (an episode that ends also stores a.last_ret and the record's last_len); s, spare,
//             have_spare, rc and - RMAV_PAIR_DR - spare_pe, pl, the handle's per-env arrays a.pe (a reset); the row: state AFTER the
//             reset, reward, action and - unless BOOT, whose includer has written it with the truncation mark - the DONE word
//             - RMAV_PAIR_DS - ds_w (a reset draws the new episode's wind), ds_ph, ds_b, ds_q (the next step's place in the gust sequence)
//   barriers: in front of the barrier that ends step k (B(k) / Y(k)), which publishes the row; the includer places it
        if (track) {
            er += r;
            el += 1;
            if (done) {
                buf_st(make_rsrc(a.last_ret), off, 0, er);
                rec_st_last_len(make_rsrc(a.rec), li, el);
                if (valid) {
                    fin_n += 1;
                    fin_len += (unsigned int)el;
                    fin_ret += er;
                }
                er = 0.0f;
                el = 0;
            }
        } else if (TL) {
            el += 1;
            if (done) el = 0;
        }
        if (K != REINMAV && auto_reset) {
            if (__ballot(done && !have_spare) != 0) {
                if (!have_spare) {   // every lane that has used its spare up (see k_rollout)
                    reset_state<K>(a.seed, env_id, rc, spare);
#if RMAV_PAIR_SS   // a START state: the draw under the handle's ranges
                    start_apply<NS>(ssc, spare);
#endif
#if RMAV_PAIR_DR
                    range_draw(dr, a.seed, env_id, rc, spare_pe);
#endif
                    have_spare = true;
                }
            }
            if (done) {
#pragma unroll
                for (int c = 0; c < NS; ++c) s[c] = spare[c];
#if RMAV_PAIR_DR
                range_apply(dr, a.pe, pc_shared, li, off, spare_pe, pl);   // the new episode's constants, re-derived and stored
#endif
#if RMAV_PAIR_DS
                wind_draw(ds.spec(), a.seed, env_id, rc, ds_w);   // the new episode's wind (the step that ended the old one has used the old)
#endif
#if RMAV_PAIR_AL   // the new episode's actuator state (the step that ended the old one ran with the old m)
#pragma unroll
                for (int c = 0; c < NA; ++c) am[c] = al_init[c];
#endif
                have_spare = false;
                rc += 1;
            }
        }
#if RMAV_PAIR_DS   // the next agent step's place in the gust sequence; a new block draws its gust (wave-uniform: kernel arguments only)
        if (++ds_ph >= ds.spec().hold) {
            ds_ph = 0;
            ++ds_b;
            if (k + 1 < T) gust_draw(ds.spec(), a.seed, env_id, ds_b, ds_q);
        }
#endif
        float *row = otile + (k & 1) * PT::O_HALF;
#if RMAV_PAIR_AL   // the *_al wrappers: the noisy row as below, or - a handle without sensor noise (al_sn = 0, wave-uniform) - the state itself
        actuator_obs_row<NS>(al_sn, sn, a.seed, env_id, a.t0 + (uint64_t)k + 1u, s, row);
#elif RMAV_PAIR_SN   // the *_sn wrappers (kernel argument sn: SensorArgs): the row holds the OBSERVATION of the state after the step and its reset,
                   // under the z of the step counter after the step - computed once, by the lane that owns the env; both nets of step k + 1
                   // and the trajectory store read it from the row.  s stays the true state.
        sensor_store_row<NS>(sn, a.seed, env_id, a.t0 + (uint64_t)k + 1u, s, row);
#else
#pragma unroll
        for (int c = 0; c < NS; ++c) row[c * 64] = s[c];
#endif
        row[PT::REW] = r;
        if constexpr (!BOOT) row[PT::DONE] = done ? 1.0f : 0.0f;
#pragma unroll
        for (int c = 0; c < NA; ++c) row[PT::ACT + c * 64] = act[c];

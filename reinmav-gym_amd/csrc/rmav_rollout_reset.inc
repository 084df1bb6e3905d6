// rmav_rollout_reset.inc - the auto-reset of rmav_rollout_body.inc: draw a spare reset state if a finishing lane has none, copy it,
// re-derive a ranged handle's constants.  Included twice, behind each of the two forms of the episode bookkeeping (SKIP_QUIET and
// predicated: see the comment above them) - the same statements, so a field added to the reset goes here once.
//   expects:  K, NS, the constexpr bools SPARE_LDS, DR and DS, the kernel arguments a, pc_shared and - DR - dr, - DS - ds; done (after the time
//             limit), auto_reset, env_id, li, off; the spare state in spare[] or - SPARE_LDS - behind lds_spare (this lane's words only)
//   defines:  nothing that outlives it
//   modifies: s, have_spare, rc, the spare state and - DR - spare_pe, pl, pcl, the handle's per-env arrays a.pe, - DS - spare_w, ds_w
//   barriers: none (the LDS spare is read back by the lane that wrote it)
                if (K != REINMAV && auto_reset) {
                    const bool rst = done;
                    if (__ballot(rst && !have_spare) != 0) {
                        if (!have_spare) {
                            float sp[NS];
                            reset_state<K>(a.seed, env_id, rc, sp);
#if RMAV_ROLLOUT_SS   // a START state: the draw under the handle's ranges
                            start_apply<NS>(ssc, sp);
#endif
#pragma unroll
                            for (int c = 0; c < NS; ++c) {
                                if constexpr (SPARE_LDS) lds_spare[c * 64] = sp[c];
                                else spare[c] = sp[c];
                            }
                            if constexpr (DR) range_draw(dr, a.seed, env_id, rc, spare_pe);
                            if constexpr (DS) wind_draw(ds.spec(), a.seed, env_id, rc, spare_w);
                            have_spare = true;
                        }
                    }
                    if (rst) {
#pragma unroll
                        for (int c = 0; c < NS; ++c) {
                            if constexpr (SPARE_LDS) s[c] = lds_spare[c * 64];
                            else s[c] = spare[c];
                        }
                        if constexpr (DR) range_apply(dr, a.pe, pc_shared, li, off, spare_pe, pl, pcl);   // the new episode's constants, re-derived and stored
                        if constexpr (DS) {   // the new episode's wind (the step that ended the old one has used the old)
#pragma unroll
                            for (int i = 0; i < disturb_dim<K>(); ++i) ds_w[i] = spare_w[i];
                        }
#if RMAV_ROLLOUT_AL   // the new episode's actuator state (the step that ended the old one ran with the old m)
#pragma unroll
                        for (int c = 0; c < Dims<K>::NA; ++c) am[c] = al_init[c];
#endif
                        have_spare = false;
                        rc += 1;
                    }
                }

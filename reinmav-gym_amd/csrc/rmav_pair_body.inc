// rmav_pair_body.inc - the body of k_rollout_pair / k_rollout_pair_tl (rmav_policy_pair.hpp), included into both kernels: textually, for the
// reason rmav_rollout_body.inc gives.  In scope: template parameters K, FMT, the constexpr bools TL, BOOT (k_rollout_pair_boot: the launch also
// leaves the bootstrap term of its truncated steps) and NORM (k_rollout_pair_nrm: both nets take normalised observations; the tables sit
// between the weights and the tiles) and the kernel arguments a, p_shared, pc_shared, tl, bt, nm, ar (ActRuleArgs: the NORM kernels apply the
// handle's action rule).
    constexpr int NS = Dims<K>::NS, NA = Dims<K>::NA;
    using L = MfmaLayout;
    using PT = PairTile<NS, NA>;
    using frag = typename PairOps<FMT>::frag;
    const uint32_t G = blockDim.x >> 7;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool critic = wave >= G;
    const uint32_t pair = critic ? wave - G : wave, lane = threadIdx.x & 63u;
    const uint32_t gi = (blockIdx.x * G + pair) * 64u + lane;
    const int64_t n = a.n;
    const bool valid = gi < (uint64_t)n;
    const uint32_t li = valid ? gi : (uint32_t)n - 1u;
    const uint32_t col = (uint32_t)n * 4u, off = li * 4u;
    const int32_t T = a.n_steps;
    const bool track = (a.flags & F_TRACK) != 0, auto_reset = (a.flags & F_AUTO_RESET) != 0;
    [[maybe_unused]] const float *ntab = lds_w + L::TOTAL;
    float *tile = lds_w + L::TOTAL + (NORM ? kNormWords : 0) + pair * (BOOT ? PairBootTile<NS, NA>::WORDS : PT::WORDS);   // this pair's hand-over tiles
    float *ztile = tile + lane, *otile = tile + PT::Z_WORDS + lane;

    if (a.xsend && blockIdx.x == 0 && threadIdx.x == 0)   // armed statistics exchange: this launch has begun (see k_rollout)
        __hip_atomic_store(a.xstarted, a.xseq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    {   // stage the weights of both nets (every thread helps), then derive the bias tables the activations need
        const float4 *src = reinterpret_cast<const float4 *>(a.policy_w);
        float4 *dst = reinterpret_cast<float4 *>(lds_w);
        for (int q = threadIdx.x; q < L::TOTAL / 4; q += blockDim.x) dst[q] = src[q];
        if constexpr (NORM) stage_norm(lds_w + L::TOTAL, nm.tab);
        __syncthreads();
        if constexpr (FMT == FMT_F16) fold_biases_f16();
        else scale_biases_for_tanh();
        __syncthreads();
    }

    const rsrc_t r_state = make_rsrc(a.state);
    float s[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) s[c] = buf_ld(r_state, off, (uint32_t)c * col);
    const uint64_t env_id = a.env_base + (uint64_t)li;

    if (critic) {
        // ---- critic: noise one step ahead, value net, every trajectory store ---------------------------------------
        float sl = 0.0f;
#pragma unroll
        for (int c = 0; c < NA; ++c) sl += lds_w[L::LOGSTD + c];
        const float logp0 = -sl - 0.5f * (float)NA * 1.8378770664093453f;   // - sum(logstd) - NA/2 ln(2 pi)
        float *logp_out = a.logp_out, *val_out = a.val_out;
        auto draw = [&](int32_t k) {   // z of step k -> its tile half; log-probability of the action it will make
            float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (!NORM || ar.noise != 0.0f) gaussian4(a.seed, env_id, a.t0 + (uint64_t)k, z);   // (wave-uniform: a deterministic launch draws nothing)
            float *zt = ztile + (k & 1) * PT::Z_HALF;
            float q = 0.0f;
#pragma unroll
            for (int c = 0; c < 4; ++c) zt[c * 64] = z[c];
#pragma unroll
            for (int c = 0; c < NA; ++c) q = rfma(z[c], z[c], q);
            if constexpr (NORM) q *= ar.noise;   // the action rule (deterministic: the log-density of the mean)
            buf_st(make_rsrc(logp_out), off, 0, rfma(-0.5f, q, logp0));
            logp_out += n;
        };
        draw(0);
        __syncthreads();                                              // B: Z(0) is in the tile
        float *act_out = a.act_out, *obs_out = a.obs_out, *rew_out = a.rew_out;
        uint8_t *done_out = a.done_out;
        for (int32_t k = 0; k <= T; ++k) {
            if (k > 0) {   // outputs of step k - 1: LDS -> trajectory; the obs is the state whose value is due now
                const float *row = otile + ((k - 1) & 1) * PT::O_HALF;
#pragma unroll
                for (int c = 0; c < NS; ++c) s[c] = row[c * 64];
                const float rw = row[PT::REW], dn = row[PT::DONE];
                float av[NA];
#pragma unroll
                for (int c = 0; c < NA; ++c) av[c] = row[PT::ACT + c * 64];
                // a missing output gets a descriptor with num_records = 0: the hardware range check drops its stores (no branch)
                const rsrc_t rA = act_out ? make_rsrc(act_out) : make_rsrc_bounded(a.state, 0u);
                const rsrc_t rO = obs_out ? make_rsrc(obs_out) : make_rsrc_bounded(a.state, 0u);
                const rsrc_t rR = rew_out ? make_rsrc(rew_out) : make_rsrc_bounded(a.state, 0u);
                const rsrc_t rD = done_out ? make_rsrc(done_out) : make_rsrc_bounded(a.state, 0u);
#pragma unroll
                for (int c = 0; c < NA; ++c) buf_st(rA, off, (uint32_t)c * col, av[c]);
#pragma unroll
                for (int c = 0; c < NS; ++c) buf_st(rO, off, (uint32_t)c * col, s[c]);
                buf_st(rR, off, 0, rw);
                __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(dn != 0.0f ? 1 : 0), rD, li, 0, 0);
                if (act_out) act_out += (int64_t)NA * n;
                if (obs_out) obs_out += (int64_t)NS * n;
                if (rew_out) rew_out += n;
                if (done_out) done_out += n;
            }
            float x[16];
            if constexpr (NORM) {
                norm_state16<NS>(ntab, s, x);
            } else {
#pragma unroll
                for (int c = 0; c < 16; ++c) x[c] = (c < NS) ? s[c] : 0.0f;
            }
            frag b0, b1;
            state_frags<FMT>(x, b0, b1);
            float t0[4], t1[4];
            mlp_pair<FMT>(b0, b1, (uint32_t)L::NET, t0, t1);
            const float vp = xor32(t1[0]);
            buf_st(make_rsrc(val_out), off, 0, (lane >> 5) ? vp : t0[0]);
            val_out += n;
            // k_rollout_pair_boot: the actor marks a truncated step with 2.0f in the DONE word and leaves the state its reset replaced in
            // the terminal area of the row (PairBootTile); the same value net on it is the step's bootstrap term.  Under B(k - 1), the
            // barrier this wavefront has already passed: a step without a truncation costs one LDS read, one ballot and two stores.
            if constexpr (BOOT) {
                if (k > 0) {
                    using PB = PairBootTile<NS, NA>;
                    const bool tr = otile[((k - 1) & 1) * PT::O_HALF + PT::DONE] == 2.0f;
                    float bv = 0.0f;
                    if (__ballot(tr) != 0) {   // wave-uniform
                        const float *fin = tile + PB::FIN + ((k - 1) & 1) * PB::FIN_HALF + lane;
                        float xf[16];
                        if constexpr (NORM) {
                            float sf[NS];
#pragma unroll
                            for (int c = 0; c < NS; ++c) sf[c] = fin[c * 64];
                            norm_state16<NS>(ntab, sf, xf);
                        } else {
#pragma unroll
                            for (int c = 0; c < 16; ++c) xf[c] = (c < NS) ? fin[c * 64] : 0.0f;
                        }
                        frag f0, f1;
                        state_frags<FMT>(xf, f0, f1);
                        float u0[4], u1[4];
                        mlp_pair<FMT>(f0, f1, (uint32_t)L::NET, u0, u1);
                        const float up = xor32(u1[0]);
                        if (tr) bv = (lane >> 5) ? up : u0[0];
                    }
                    buf_st(make_rsrc(bt.boot_out + (int64_t)(k - 1) * n), off, 0, bv);
                    const rsrc_t rT = bt.trunc_out ? make_rsrc(bt.trunc_out + (int64_t)(k - 1) * n) : make_rsrc_bounded(a.state, 0u);
                    __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(tr ? 1 : 0), rT, li, 0, 0);
                }
            }
            if (k + 1 < T) draw(k + 1);
            if (k < T) __syncthreads();                               // B(k): O(k) handed over, Z(k + 1) in the tile
        }
        return;
    }

    // ---- actor: policy net, action, dynamics, bookkeeping --------------------------------------------------------------
    unsigned int fin_n = 0, fin_len = 0;
    float fin_ret = 0.0f;
    float er = 0.0f;
    int32_t el = 0;
    int32_t sb;   // the env's record (EnvRec): steps_beyond_done, reset counter and - when tracking - the episode's start in ONE access
    uint32_t rc;
    if (track) {
        er = buf_ld(make_rsrc(a.ep_ret), off, 0);
        const u32x3_t q = rec_ld3(make_rsrc(a.rec), li);
        sb = (int32_t)q.x;
        rc = q.y;
        el = (int32_t)(ep_clock0(a) - q.z);
    } else if (TL) {   // (the running length is counted whether or not the handle tracks episodes)
        const u32x3_t q = rec_ld3(make_rsrc(a.rec), li);
        sb = (int32_t)q.x;
        rc = q.y;
        el = (int32_t)(ep_clock0(a) - q.z);
    } else {
        const u32x2_t q = rec_ld2(make_rsrc(a.rec), li);
        sb = (int32_t)q.x;
        rc = q.y;
    }
    typename Env<K>::P pl = p_shared;
    if constexpr (K != REINMAV) {
        if (a.pe[0] || a.pe[1] || a.pe[2]) {
            const double m = a.pe[0] ? (double)a.pe[0][li] : (double)pc_shared.mass;
            const double ml = a.pe[1] ? (double)a.pe[1][li] : (double)pc_shared.load_mass;
            const double Lt = a.pe[2] ? (double)a.pe[2][li] : (double)pc_shared.L;
            override_params(pl, m, ml, Lt);
        }
    }
    const typename Env<K>::P &p = pl;
    double tenv = 0.0;
    if constexpr (K == REINMAV) tenv = a.env_time[li];
    // spare reset state, drawn once per launch (see k_rollout)
    float spare[NS];
    bool have_spare = false;
#if RMAV_PAIR_DR   // the *_dr kernels: the constants of the episode the spare state starts (the ranged parameters' elements)
    float spare_pe[3] = {0.0f, 0.0f, 0.0f};
#endif
    if (K != REINMAV && auto_reset && T >= 8) {
        reset_state<K>(a.seed, env_id, rc, spare);
#if RMAV_PAIR_DR
        range_draw(dr, a.seed, env_id, rc, spare_pe);
#endif
        have_spare = true;
    }
    float pol_std[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NA; ++c) pol_std[c] = NORM ? expf(lds_w[L::LOGSTD + c]) * ar.noise : expf(lds_w[L::LOGSTD + c]);   // the action rule: std_eff
    __syncthreads();                                                  // B: Z(0) is in the tile
    for (int32_t k = 0; k < T; ++k) {
        float z[NA];
        {
            const float *zt = ztile + (k & 1) * PT::Z_HALF;
#pragma unroll
            for (int c = 0; c < NA; ++c) z[c] = zt[c * 64];
        }
        float x[16];
        if constexpr (NORM) {
            norm_state16<NS>(ntab, s, x);
        } else {
#pragma unroll
            for (int c = 0; c < 16; ++c) x[c] = (c < NS) ? s[c] : 0.0f;
        }
        frag b0, b1;
        state_frags<FMT>(x, b0, b1);
        float t0[4], t1[4], act[NA];
        mlp_pair<FMT>(b0, b1, 0u, t0, t1);
#pragma unroll
        for (int c = 0; c < NA; ++c) {
            const float from_partner = xor32(t1[c]);
            act[c] = rfma(pol_std[c], z[c], (lane >> 5) ? from_partner : t0[c]);
        }
        float dist = 0.0f, r;
        bool done;
        if constexpr (K == REINMAV) {
            float fm0[4];
            Env<K>::step(s, act, false, tenv, p, fm0);
            done = true;   // reinmav_env.py:110
            r = 90.0f;     // reinmav_env.py:111-116
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
        // time limit (see k_rollout): after the reward / steps_beyond_done machine, before the episode hand-off
        if constexpr (TL) {
            const bool trunc = !done && el + 1 >= tl.max_steps;
            done = done || trunc;
            if (done) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(trunc ? 1 : 0), make_rsrc(tl.last_trunc), li, 0, 0);
            // k_rollout_pair_boot: the critic owns the value net, this wavefront the state - hand the pre-reset state over in the row's
            // terminal area (only on a step with a truncated lane) and say which lanes in the DONE word
            if constexpr (BOOT) {
                using PB = PairBootTile<NS, NA>;
                if (__ballot(trunc) != 0) {   // wave-uniform
                    float *fin = tile + PB::FIN + (k & 1) * PB::FIN_HALF + lane;
#pragma unroll
                    for (int c = 0; c < NS; ++c) fin[c * 64] = s[c];
                }
                otile[(k & 1) * PT::O_HALF + PT::DONE] = trunc ? 2.0f : (done ? 1.0f : 0.0f);
            }
        }
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
                have_spare = false;
                rc += 1;
            }
        }
        float *row = otile + (k & 1) * PT::O_HALF;
#pragma unroll
        for (int c = 0; c < NS; ++c) row[c * 64] = s[c];
        row[PT::REW] = r;
        if constexpr (!BOOT) row[PT::DONE] = done ? 1.0f : 0.0f;
#pragma unroll
        for (int c = 0; c < NA; ++c) row[PT::ACT + c * 64] = act[c];
        __syncthreads();                                              // B(k)
    }
#pragma unroll
    for (int c = 0; c < NS; ++c) buf_st(r_state, off, (uint32_t)c * col, s[c]);
    if constexpr (K == REINMAV) a.env_time[li] = tenv;
    if (track) {
        buf_st(make_rsrc(a.ep_ret), off, 0, er);
        rec_st3(make_rsrc(a.rec), li, u32x3_t{(uint32_t)sb, rc, ep_clock0(a) + (uint32_t)a.n_steps - (uint32_t)el});
    } else if (TL) {
        rec_st3(make_rsrc(a.rec), li, u32x3_t{(uint32_t)sb, rc, ep_clock0(a) + (uint32_t)a.n_steps - (uint32_t)el});
    } else {
        rec_st2(make_rsrc(a.rec), li, u32x2_t{(uint32_t)sb, rc});
    }
    if (track && __ballot(fin_n != 0) != 0) {   // episode totals: this wavefront's slot (see k_rollout)
        Totals *slot = a.totals + (gi >> 6);
        const unsigned int wn = wave_sum_x(fin_n);
        const unsigned int wl = wave_sum_x(fin_len);
        const float wr = wave_sum_x(fin_ret);
        if (lane == 0) {
            atomicAdd(&slot->episodes, (unsigned long long)wn);
            atomicAdd(&slot->length_sum, (unsigned long long)wl);
            atomicAdd(&slot->return_sum, (double)wr);
        }
    }
    if (a.xsend) {   // snapshot for the armed statistics exchange, then this wavefront's arrival word (see k_rollout)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (valid) {
            const float lr = a.last_ret[li];
            const int32_t ll = a.rec[li].last_len;
            __hip_atomic_store(a.xsend + li, __builtin_bit_cast(int32_t, lr), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.xsend + a.xcmax + li, ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0 && valid) __hip_atomic_store(a.xarrive + (gi >> 6), a.xseq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }

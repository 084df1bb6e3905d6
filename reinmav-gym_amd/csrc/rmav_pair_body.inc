// rmav_pair_body.inc - the body of k_rollout_pair / k_rollout_pair_tl (rmav_policy_pair.hpp), included into both kernels: textually, for the
// reason rmav_rollout_body.inc gives.  In scope: template parameters K, FMT, the constexpr bools TL, BOOT (k_rollout_pair_boot: the launch also
// leaves the bootstrap term of its truncated steps) and NORM (k_rollout_pair_nrm: both nets take normalised observations; the tables sit
// between the weights and the tiles) and the kernel arguments a, p_shared, pc_shared, tl, bt, nm, ar (ActRuleArgs: the NORM kernels apply the
// handle's action rule).
//
// The statements this body has in common with rmav_pair_shared_body.inc are nested fragments both include, one file each (rmav_pair_index.inc,
// _draw, _env_load, _dynamics, _episode, _epilogue): each opens with the names it expects, defines and modifies and the barrier it sits
// next to.  What differs between the two kernels - how the nets are evaluated, the hand-over of the means, the BOOT parts - is here.
    constexpr int NS = Dims<K>::NS, NA = Dims<K>::NA;
    using L = MfmaLayout;
    using PT = PairTile<NS, NA>;
    using frag = typename PairOps<FMT>::frag;
#include "rmav_pair_index.inc"   // G, wave, helper (the critic), pair, lane, h, gi, n, valid, li, col, off, T, track, auto_reset
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
    const float *logstd = lds_w + L::LOGSTD;
    const uint64_t env_id = a.env_base + (uint64_t)li;

    if (helper) {
        // ---- critic: noise one step ahead, value net, every trajectory store ---------------------------------------
#include "rmav_pair_draw.inc"   // logp0, logp_out, val_out, draw(k)
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
#if RMAV_PAIR_SN   // the observation of the launch's first state: the row the actor wavefront has left in half 1 in front of barrier B
            else {
                const float *row = otile + PT::O_HALF;
#pragma unroll
                for (int c = 0; c < NS; ++c) s[c] = row[c * 64];
            }
#endif
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
            buf_st(make_rsrc(val_out), off, 0, h ? vp : t0[0]);
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
                        if (tr) bv = h ? up : u0[0];
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
#include "rmav_pair_env_load.inc"   // fin_*, er, el, sb, rc, pl / p, tenv, spare, have_spare, pol_std
#if RMAV_PAIR_AL   // (the *_al wrappers: the noisy row or - al_sn = 0, wave-uniform - the state itself)
    actuator_obs_row<NS>(al_sn, sn, a.seed, env_id, a.t0, s, otile + PT::O_HALF);
#elif RMAV_PAIR_SN   // the observation of the launch's first state (step counter t0), where step "-1" would have left its row: half 1
    sensor_store_row<NS>(sn, a.seed, env_id, a.t0, s, otile + PT::O_HALF);
#endif
    __syncthreads();                                                  // B: Z(0) is in the tile
    for (int32_t k = 0; k < T; ++k) {
        float z[NA];
        {
            const float *zt = ztile + (k & 1) * PT::Z_HALF;
#pragma unroll
            for (int c = 0; c < NA; ++c) z[c] = zt[c * 64];
        }
        float x[16];
#if RMAV_PAIR_SN   // the policy net reads the observation this lane stored as the previous row (its own words of the tile: program order)
        if constexpr (NORM) {
            float o[NS];
            const float *prev = otile + ((k - 1) & 1) * PT::O_HALF;
#pragma unroll
            for (int c = 0; c < NS; ++c) o[c] = prev[c * 64];
            norm_state16<NS>(ntab, o, x);
        } else {
#else
        if constexpr (NORM) {
            norm_state16<NS>(ntab, s, x);
        } else {
#endif
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
            act[c] = rfma(pol_std[c], z[c], h ? from_partner : t0[c]);
        }
#include "rmav_pair_dynamics.inc"   // dist, r, done; LEAVES OPEN `if constexpr (TL) {` with `const bool trunc` in it:
            // k_rollout_pair_boot: the critic owns the value net, this wavefront the state - hand the pre-reset state over in the row's
            // terminal area (only on a step with a truncated lane) and say which lanes in the DONE word
            if constexpr (BOOT) {
                using PB = PairBootTile<NS, NA>;
                if (__ballot(trunc) != 0) {   // wave-uniform
                    float *fin = tile + PB::FIN + (k & 1) * PB::FIN_HALF + lane;
#if RMAV_PAIR_AL
                    actuator_obs_row<NS>(al_sn, sn, a.seed, env_id, a.t0 + (uint64_t)k + 1u, s, fin);
#elif RMAV_PAIR_SN   // the terminal OBSERVATION: the pre-reset state under the z of this step's row
                    sensor_store_row<NS>(sn, a.seed, env_id, a.t0 + (uint64_t)k + 1u, s, fin);
#else
#pragma unroll
                    for (int c = 0; c < NS; ++c) fin[c * 64] = s[c];
#endif
                }
                otile[(k & 1) * PT::O_HALF + PT::DONE] = trunc ? 2.0f : (done ? 1.0f : 0.0f);
            }
        }   // if constexpr (TL), opened in rmav_pair_dynamics.inc
#include "rmav_pair_episode.inc"   // episode bookkeeping, auto-reset, the row of step k
        __syncthreads();                                              // B(k)
    }
#include "rmav_pair_epilogue.inc"   // state and record write-back, episode totals, statistics-exchange snapshot

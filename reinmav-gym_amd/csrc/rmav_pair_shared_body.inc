// rmav_pair_shared_body.inc - the body of k_rollout_pair_shared / k_rollout_pair_shared_tl (rmav_policy_pair.hpp), included into both kernels: textually, for the
// reason rmav_rollout_body.inc gives.  In scope: template parameters K, the constexpr bools TL, BOOT (k_rollout_pair_shared_boot: the launch also leaves
// the bootstrap term of its truncated steps) and NORM (k_rollout_pair_shared_nrm: the net takes normalised observations; the tables sit between the
// weights and the tiles) and the kernel arguments a, p_shared, pc_shared, tl, bt, nm, ar (ActRuleArgs: the NORM kernels apply the
// handle's action rule).
//
// The statements this body has in common with rmav_pair_body.inc are nested fragments both include, one file each (rmav_pair_index.inc,
// _draw, _env_load, _dynamics, _episode, _epilogue): each opens with the names it expects, defines and modifies and the barrier it sits
// next to.  What differs between the two kernels - how the nets are evaluated, the hand-over of the means, the BOOT parts - is here.
    constexpr int NS = Dims<K>::NS, NA = Dims<K>::NA;
    using L = MfmaLayout;
    using PT = PairTile<NS, NA>;
    using ST_ = SharedTile<NS, NA>;
#include "rmav_pair_index.inc"   // G, wave, helper (wavefront B), pair, lane, h, gi, n, valid, li, col, off, T, track, auto_reset
    [[maybe_unused]] const float *ntab = lds_w + kSharedWeights;
    float *tile = lds_w + kSharedWeights + (NORM ? kNormWords : 0) + pair * (BOOT ? SharedBootTile<NS, NA>::WORDS : ST_::WORDS);
    float *ztile = tile + lane, *otile = tile + PT::Z_WORDS + lane, *mtile = tile + ST_::MEAN;

    if (a.xsend && blockIdx.x == 0 && threadIdx.x == 0)
        __hip_atomic_store(a.xstarted, a.xseq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    {   // stage the one net (+ logstd: the buffer's last four words land where LOGSTD of a two-net buffer would not be: keep them apart)
        const float4 *src = reinterpret_cast<const float4 *>(a.policy_w);
        float4 *dst = reinterpret_cast<float4 *>(lds_w);
        for (int q = threadIdx.x; q < kSharedWeights / 4; q += blockDim.x) dst[q] = src[q];
        if constexpr (NORM) stage_norm(lds_w + kSharedWeights, nm.tab);
        __syncthreads();
        for (int q = threadIdx.x; q < 160; q += blockDim.x) {   // fold_biases_f16 for net 0 only
            float *w = lds_w;
            if (q < 64) {
                w[L::B1 + q] *= kTanhScale;
            } else {
                const bool l2 = q < 128;
                const int i = l2 ? q - 64 : q - 128, Tt = l2 ? (i >> 5) : 0, m = i & 31;
                const float *frag0 = w + (l2 ? L::A2 + Tt * 4 * L::FRAG : L::A3);
                float sum = 0.0f;
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int hh = 0; hh < 2; ++hh) {
                        const f16x8_t v = *reinterpret_cast<const f16x8_t *>(frag0 + s * L::FRAG + (m + 32 * hh) * 4);
#pragma unroll
                        for (int j = 0; j < 8; ++j) sum += (float)v[j];
                    }
                float *b = w + (l2 ? L::B2 : L::B3) + i;
                *b = (l2 ? kTanhScale * *b : *b) - 0.5f * sum;
            }
        }
        __syncthreads();
    }
    const float *logstd = lds_w + L::NET;
    const uint64_t env_id = a.env_base + (uint64_t)li;

    if (helper) {
        // ---- B: tile 1 of the net, noise one step ahead, log-prob, every trajectory store ---------------------------------------
#include "rmav_pair_draw.inc"   // logp0, logp_out, val_out, draw(k)
        // the net for envs 32..63 of the pair from the obs tile half `half`: lane (n, h) takes components [8h, 8h + 8) of env 32 + n
        auto eval_tile1 = [&](int half) {
            const float *obs = tile + PT::Z_WORDS + half * PT::O_HALF + 32u + (lane & 31u);
            float x[8];
            [[maybe_unused]] const float *nt = nullptr;
            [[maybe_unused]] float nclip = 0.0f;
            if constexpr (NORM) {
                nt = norm_tab(ntab);
                nclip = nt[32];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float lo = (j < NS) ? obs[j * 64] : 0.0f, hi = (8 + j < NS) ? obs[(8 + j) * 64] : 0.0f;
                if constexpr (NORM) {
                    if (j < NS) lo = norm1(nt, j, lo, nclip);
                    if (8 + j < NS) hi = norm1(nt, 8 + j, hi, nclip);
                }
                x[j] = h ? hi : lo;
            }
            float o4[4];
            mlp_half_f16(pack_frag_f16(x), o4);
            if (!h) {
#pragma unroll
                for (int c = 0; c < 4; ++c) mtile[c * 32 + lane] = o4[c];    // means of envs 32..63 -> A
            } else {
                buf_st(make_rsrc(val_out), off, 0, o4[0]);                    // lane 32 + n IS env 32 + n of the pair
            }
            val_out += n;
        };
        draw(0);
        __syncthreads();                                                  // P: Z(0) and the initial obs are in the tiles
        float *act_out = a.act_out, *obs_out = a.obs_out, *rew_out = a.rew_out;
        uint8_t *done_out = a.done_out;
        auto drain = [&](int half) {
            const float *row = otile + half * PT::O_HALF;
            float o[NS], av[NA];
#pragma unroll
            for (int c = 0; c < NS; ++c) o[c] = row[c * 64];
            const float rw = row[PT::REW], dn = row[PT::DONE];
#pragma unroll
            for (int c = 0; c < NA; ++c) av[c] = row[PT::ACT + c * 64];
            const rsrc_t rA = act_out ? make_rsrc(act_out) : make_rsrc_bounded(a.state, 0u);
            const rsrc_t rO = obs_out ? make_rsrc(obs_out) : make_rsrc_bounded(a.state, 0u);
            const rsrc_t rR = rew_out ? make_rsrc(rew_out) : make_rsrc_bounded(a.state, 0u);
            const rsrc_t rD = done_out ? make_rsrc(done_out) : make_rsrc_bounded(a.state, 0u);
#pragma unroll
            for (int c = 0; c < NA; ++c) buf_st(rA, off, (uint32_t)c * col, av[c]);
#pragma unroll
            for (int c = 0; c < NS; ++c) buf_st(rO, off, (uint32_t)c * col, o[c]);
            buf_st(rR, off, 0, rw);
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(dn != 0.0f ? 1 : 0), rD, li, 0, 0);
            if (act_out) act_out += (int64_t)NA * n;
            if (obs_out) obs_out += (int64_t)NS * n;
            if (rew_out) rew_out += n;
            if (done_out) done_out += n;
        };
        for (int32_t k = 0; k < T; ++k) {
            eval_tile1((k - 1) & 1);                                      // obs before step k
            __syncthreads();                                              // X(k): the means of envs 32..63 are in the tile
            if (k > 0) drain((k - 1) & 1);
            if constexpr (BOOT) {
                if (k > 0) shared_boot_tile1<NS, NA, NORM>(tile, (k - 1) & 1, bt, (int64_t)(k - 1) * n, make_rsrc_bounded(a.state, 0u), off, li, ntab);
            }
            if (k + 1 < T) draw(k + 1);
            __syncthreads();                                              // Y(k): step k's outputs are in the tile
        }
        eval_tile1((T - 1) & 1);                                          // bootstrap values of envs 32..63
        drain((T - 1) & 1);
        if constexpr (BOOT) shared_boot_tile1<NS, NA, NORM>(tile, (T - 1) & 1, bt, (int64_t)(T - 1) * n, make_rsrc_bounded(a.state, 0u), off, li, ntab);
        return;
    }

    // ---- A: tile 0 of the net from its registers, then action, dynamics, bookkeeping for all 64 envs -----------------------------
    const rsrc_t r_state = make_rsrc(a.state);
    float s[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) s[c] = buf_ld(r_state, off, (uint32_t)c * col);
#include "rmav_pair_env_load.inc"   // fin_*, er, el, sb, rc, pl / p, tenv, spare, have_spare, pol_std
    // value of env gi - 32 (tile 0's column lane - 32) leaves through this lane
    const bool vvalid = h && (uint64_t)(gi - 32u) < (uint64_t)n;
    const uint32_t voff = (gi - 32u) * 4u;
    float *val_out = a.val_out;
#if RMAV_PAIR_SN   // the *_sn wrappers: the net reads the OBSERVATION this lane stored as the previous row (its own words of the tile: program
                   // order), not the true state in s; sn_half names that row's half
    int sn_half = 1;
#define RMAV_SOBS(c) (otile[sn_half * PT::O_HALF + (c) * 64])
#else
#define RMAV_SOBS(c) (s[c])
#endif
    auto eval_tile0 = [&](float (&o4)[4]) {   // lane (n, h): components [8h, 8h + 8) of env n - its own for h = 0, lane n's for h = 1
        float x[8];
        [[maybe_unused]] const float *nt = nullptr;
        [[maybe_unused]] float nclip = 0.0f;
        if constexpr (NORM) {
            nt = norm_tab(ntab);
            nclip = nt[32];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float lo = (j < NS) ? RMAV_SOBS(j) : 0.0f;
            float hi = 0.0f;
            if constexpr (NORM) {   // normalised by the lane that owns the env, before the exchange
                if (j < NS) lo = norm1(nt, j, lo, nclip);
                if (8 + j < NS) hi = xor32(norm1(nt, 8 + j, RMAV_SOBS(8 + j), nclip));
            } else {
                if (8 + j < NS) hi = xor32(RMAV_SOBS(8 + j));   // lanes 32..63 receive lane - 32's component 8 + j  (folded: NS is a constant)
            }
            x[j] = h ? hi : lo;
        }
        mlp_half_f16(pack_frag_f16(x), o4);
        if (vvalid) buf_st(make_rsrc(val_out), voff, 0, o4[0]);
        val_out += n;
    };
    {   // the initial obs of the pair's envs, for B's first evaluation: the obs half step "-1" would have written
        float *row = otile + PT::O_HALF;
#if RMAV_PAIR_AL   // (the *_al wrappers: the noisy row or - al_sn = 0, wave-uniform - the state itself)
        actuator_obs_row<NS>(al_sn, sn, a.seed, env_id, a.t0, s, row);
#elif RMAV_PAIR_SN   // ... the observation of the launch's first state, at the step counter t0
        sensor_store_row<NS>(sn, a.seed, env_id, a.t0, s, row);
#else
#pragma unroll
        for (int c = 0; c < NS; ++c) row[c * 64] = s[c];
#endif
    }
    __syncthreads();                                                      // P
    for (int32_t k = 0; k < T; ++k) {
        float o4[4];
#if RMAV_PAIR_SN
        sn_half = (k - 1) & 1;
#endif
        eval_tile0(o4);
        __syncthreads();                                                  // X(k)
        float act[NA];
        {
            const float *zt = ztile + (k & 1) * PT::Z_HALF;
#pragma unroll
            for (int c = 0; c < NA; ++c) {
                const float mean = h ? mtile[c * 32 + (lane & 31u)] : o4[c];
                act[c] = rfma(pol_std[c], zt[c * 64], mean);
            }
        }
#include "rmav_pair_dynamics.inc"   // dist, r, done; LEAVES OPEN `if constexpr (TL) {` with `const bool trunc` in it:
            // k_rollout_pair_shared_boot: on a step with a truncated lane both wavefronts run the net once more on the state the reset
            // below replaces - this one for envs 0..31 from its registers (the value of env n leaves lane 32 + n, as eval_tile0's), B
            // for envs 32..63 from the row's terminal area (SharedBootTile); the DONE word tells B which lanes
            if constexpr (BOOT) {
                using SB = SharedBootTile<NS, NA>;
                float bv = 0.0f;
                const uint64_t tm = __ballot(trunc);
                if (tm != 0) {   // wave-uniform
                    float *fin = tile + SB::FIN + (k & 1) * SB::FIN_HALF + lane;
#if RMAV_PAIR_AL
                    actuator_obs_row<NS>(al_sn, sn, a.seed, env_id, a.t0 + (uint64_t)k + 1u, s, fin);
#define RMAV_SFIN(c) (fin[(c) * 64])
#elif RMAV_PAIR_SN   // the terminal OBSERVATION: the pre-reset state under the z of this step's row; both wavefronts evaluate the net on it
                    sensor_store_row<NS>(sn, a.seed, env_id, a.t0 + (uint64_t)k + 1u, s, fin);
#define RMAV_SFIN(c) (fin[(c) * 64])
#else
#pragma unroll
                    for (int c = 0; c < NS; ++c) fin[c * 64] = s[c];
#define RMAV_SFIN(c) (s[c])
#endif
                    float xf[8], u4[4];
                    [[maybe_unused]] const float *nt = nullptr;
                    [[maybe_unused]] float nclip = 0.0f;
                    if constexpr (NORM) {
                        nt = norm_tab(ntab);
                        nclip = nt[32];
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        float lo = (j < NS) ? RMAV_SFIN(j) : 0.0f;
                        float hi = 0.0f;
                        if constexpr (NORM) {
                            if (j < NS) lo = norm1(nt, j, lo, nclip);
                            if (8 + j < NS) hi = xor32(norm1(nt, 8 + j, RMAV_SFIN(8 + j), nclip));
                        } else {
                            if (8 + j < NS) hi = xor32(RMAV_SFIN(8 + j));
                        }
                        xf[j] = h ? hi : lo;
                    }
                    mlp_half_f16(pack_frag_f16(xf), u4);
                    if (h && ((tm >> (lane & 31u)) & 1ull)) bv = u4[0];
                }
                if (vvalid) buf_st(make_rsrc(bt.boot_out + (int64_t)k * n), voff, 0, bv);
                otile[(k & 1) * PT::O_HALF + PT::DONE] = trunc ? 2.0f : (done ? 1.0f : 0.0f);
            }
        }   // if constexpr (TL), opened in rmav_pair_dynamics.inc
#include "rmav_pair_episode.inc"   // episode bookkeeping, auto-reset, the row of step k
        __syncthreads();                                                  // Y(k)
    }
    {
        float o4[4];
#if RMAV_PAIR_SN
        sn_half = (T - 1) & 1;
#endif
        eval_tile0(o4);                                                   // bootstrap values of envs 0..31
    }
#undef RMAV_SOBS
#undef RMAV_SFIN
#include "rmav_pair_epilogue.inc"   // state and record write-back, episode totals, statistics-exchange snapshot

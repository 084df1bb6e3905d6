// rmav_rollout_body.inc - the body of the fused rollout kernels k_rollout and k_rollout_tl (rmav_kernels.hpp), included into both.
// Textually, not as a shared __device__ function: the optimiser simplifies such a function on its own - with `a` an opaque pointer
// rather than the kernel's constant argument block - before inlining it, and the kernels came out with a different instruction
// stream (tools/isa_compare.py, profiles/r07/time_limit.md).  In scope: template parameters K, MODE, ST, FIXED, the constexpr
// bool TL (the launch has an episode time limit), the constexpr bool FS (k_rollout_fs: each action is held for up to fs.k sub-steps), the constexpr bool BOOT (it also leaves the bootstrap term of truncated steps:
// k_rollout_boot), the constexpr bool NORM (the nets take normalised observations: k_rollout_nrm - the kernels that also apply the
// handle's action rule `ar`, ActRuleArgs) and the kernel arguments a, p_shared, pc_shared, tl, bt, nm, ar.  The same idiom one level
// down: the auto-reset of the step loop is the fragment rmav_rollout_reset.inc, included behind each form of the episode bookkeeping.
    constexpr int NS = Dims<K>::NS, NA = Dims<K>::NA;
    constexpr int AUX = StoreAux<ST>::value;
    // ACT_RANDOM_SPLIT: 128-thread workgroups, both wavefronts address the same 64 envs
    constexpr bool SPLIT = is_split(MODE), DRAWS = split_feeds_actions(MODE);   // DRAWS: the hand-over has an action tile
    [[maybe_unused]] constexpr int CH = SplitTile<NS, NA, DRAWS>::CH;   // env-steps per hand-over (split modes)
    // SPLIT: G pairs per workgroup; threads [0, 64 G) are the integrators, [64 G, 128 G) their memory wavefronts
    const uint32_t split_g = SPLIT ? (blockDim.x >> 7) : 1u;
    // (Alternating the two roles between the halves by workgroup index was measured in round 4 - no difference with one pair per
    // workgroup, slower with several, profiles/r04/two_d_kinds.md: which wavefronts share a SIMD is not what bounds them.)
    const bool upper_half = SPLIT && (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) >= split_g;
    const bool split_helper = upper_half;
    const uint32_t split_local = threadIdx.x - (upper_half ? 64u * split_g : 0u);
    const uint32_t gi = a.slice_first + (SPLIT ? blockIdx.x * (64u * split_g) + split_local : blockIdx.x * blockDim.x + threadIdx.x);
    const uint32_t slice_end = a.slice_count ? a.slice_first + a.slice_count : (uint32_t)a.n;
    // SPLIT: this pair's hand-over tiles
    [[maybe_unused]] float *lds_p = lds_w;
    if constexpr (SPLIT)
        lds_p = lds_w + (uint32_t)__builtin_amdgcn_readfirstlane(split_local >> 6) * SplitTile<NS, NA, DRAWS>::WORDS;
    const int64_t n = a.n;
    // ACT_POLICY_F32M: 32 envs per wavefront, env = column n of the wavefront's tile, simulated by both half-waves
    constexpr bool HALF = (MODE == ACT_POLICY_F32M);
    // The MFMA actor needs all 64 lanes of a wavefront to take part (lane l and lane l ^ 32 exchange state),
    // so in that mode lanes past the end of the batch become clones of env N-1: they compute and store
    // exactly what that env's lane does; only the episode totals must not count them.
    const uint32_t ge = HALF ? ((gi >> 6) << 5) + (gi & 31u) : gi;                      // env this lane works on
    const bool valid = ge < slice_end;
    const uint32_t li = ((is_mfma_policy(MODE) || SPLIT) && !valid) ? slice_end - 1u : ge;   // local env index
    const uint32_t col = (uint32_t)n * 4u;                      // bytes between components of an SoA block
    // trajectory arrays: [T][dim][pitch] feature-major (rmav_rollout_pitched; pitch = N otherwise, and always for batch-major)
    const int64_t tn = a.pitch;
    const uint32_t tcol = (uint32_t)tn * 4u;
    const uint32_t off = li * 4u;                               // this lane's byte offset inside a column
    const bool aos = !FIXED && (a.flags & F_AOS) != 0;
    const bool track = FIXED || (a.flags & F_TRACK) != 0;
    const bool auto_reset = FIXED || (a.flags & F_AUTO_RESET) != 0;

    // (the host rejects n_steps <= 0; the two-wavefront barrier protocol below needs at least one step.  Only there:
    // the same guard in front of the one-wavefront variants made hipcc restructure their step loop and cost them
    // 33-38 VGPRs, i.e. two to three wavefronts per SIMD of occupancy)
    if constexpr (is_split(MODE)) {
        if (a.n_steps <= 0) return;
    }

    // armed statistics exchange: "this launch has begun" - the communicator stream's 2 s bound counts from here.  Not in the
    // controller-driven two-wavefront kernels: their integrators (fp64 controller on the fp64 step, 124 - 128 registers) spill to
    // scratch with one more live value up here, and the same store inside their memory wavefront makes hipcc wrap that wavefront's
    // buffer accesses in waterfall loops (tests/test_resource_usage.py catches both); the host knows (kPublishesStart) and bounds
    // those launches by the waiter's overall limit only.
    if constexpr (publishes_start(MODE)) {
        if (a.xsend && blockIdx.x == 0 && threadIdx.x == 0)
            __hip_atomic_store(a.xstarted, a.xseq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }

    unsigned int fin_n = 0, fin_len = 0;
    float fin_ret = 0.0f;

    // ACT_RANDOM_SPLIT.  At C2 (65 536 envs = one wavefront per SIMD) the single-wavefront kernel is bound twice
    // over: ONE wavefront issues its ~340 instructions per env-step (VALU + SALU + branches, one stream) at ~5
    // cycles each - 0.72 us per env-step with every output switched off, against 0.34 us per wavefront-step when
    // 16 wavefronts share a SIMD - and then stalls on its own burst of 16 stores, while a store-only kernel
    // with the same pattern drains the trajectory at 7 TB/s (tools/micro/write_ceiling.hip: 36 us per 64 steps).
    // So each 64 envs get a second, "memory" wavefront:
    //   helper  (wave 1): draws the actions (Philox - a third of the instruction stream, independent of the
    //                     state) CH env-steps ahead into an LDS tile, and issues EVERY trajectory
    //                     store: actions directly, obs / reward / done from a second LDS tile the integrator
    //                     fills.  It is the only wavefront that ever waits on the memory pipeline.
    //   integrator (wave 0): state in registers, reads actions from LDS, writes its outputs to LDS.
    // Both tiles are double-buffered; one s_barrier per env-step swaps the halves of both.  The memory wavefront runs TWO
    // steps ahead with the actions, so that the integrator can fetch A(k+1) from LDS while it integrates step k (the LDS
    // round trip behind the barrier used to sit on its critical path: ~150 of ~1100 cycles per step):
    //   helper:     fill A(0), A(1) | B0 |               B0x | fill A(2)                | B1 | fill A(3), drain O(0) | B2 | ... | B(nc) | drain O(nc-1)
    //   integrator:                   B0 | read A(0)   | B0x | read A(1), A(0) -> O(0)  | B1 | read A(2), A(1) -> O(1) | B2 | ... | B(nc)
    // (B0x keeps fill A(2) - same half as A(0) - behind the integrator's first read.)
    // Same Philox counters, same arithmetic: same bits as ACT_RANDOM.  Lanes past the end of the batch are clones
    // of env N-1 (as in the MFMA mode) so that every lane of both wavefronts reaches every barrier.
    // ACT_CONTROLLER_SPLIT is the same arrangement without the draws: the integrator evaluates the controller and
    // hands the action over with its other outputs; the helper only drains.
    if constexpr (SPLIT) {
        using ST_ = SplitTile<NS, NA, DRAWS>;
        // The integrator's dependent chain is the critical path: issue priority 1 for it where that measured faster (same box,
        // two repetitions: quadrotor2d at 65 536 envs 36.9 -> 35.4 us, quadrotor3d at 131 072 envs 92.0 -> 90.5; NOT quadrotor3d
        // with one pair per SIMD: 44.4 -> 44.8, so the 3-D kinds get it only from 6 pairs per workgroup up; priority for the MEMORY
        // wavefront instead: 43.2 -> 45.0).
        if (!split_helper && (K == QUAD2D || K == QUAD2D_SL || split_g >= 6u)) __builtin_amdgcn_s_setprio(1);
        if (split_helper) {
            const uint64_t env_id = a.env_base + (uint64_t)li;
            const uint32_t lane = threadIdx.x & 63u;
            const int32_t T = a.n_steps;
            const int32_t nc = (T + CH - 1) / CH;
            // batch-major obs: output dword 64 q + lane of this wavefront is component e % NS of its env e / NS
            const uint32_t wave_first = __builtin_amdgcn_readfirstlane(gi - lane);
            // (the end of the slice again, as a 64-bit value of its own: derived from the kernel-scope `slice_end` - 32-bit, or
            // widened - hipcc stopped treating the trajectory descriptors below as wave-uniform and wrapped every store of
            // this wavefront in a waterfall loop: 243 v_readfirstlane in the quadrotor3d kernel instead of 3.
            // tests/test_resource_usage.py counts them.)
            const int64_t end64 = a.slice_count ? (int64_t)a.slice_first + (int64_t)a.slice_count : n;
            const uint32_t n_here = (uint64_t)wave_first + 64u <= (uint64_t)end64 ? 64u
                                    : ((uint64_t)wave_first < (uint64_t)end64 ? (uint32_t)(end64 - wave_first) : 0u);
            const uint32_t aos_bytes = n_here * (uint32_t)(NS * 4);   // clones past the end of the batch store nothing
            // wave-uniform: the ragged last wavefront drains dword-wise, and so does a batch whose column pitch or done
            // pointer would misalign the 16-byte / packed-byte stores
            [[maybe_unused]] const bool wide = !aos && n_here == 64u && (tn & 3) == 0 &&
                                               (reinterpret_cast<uintptr_t>(a.done_out) & 3u) == 0;
            uint32_t aos_rd[NS];
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                const uint32_t e = 64u * q + lane;
                aos_rd[q] = (e / NS) * ST_::OBS_STRIDE + (e % NS);
            }
            // ACT_BUFFER_SPLIT: this wavefront also writes the last-episode statistics when an env's episode ends (the integrator's
            // only stores inside its step loop - it must not have any, see split_self_fetch): the same running sums from the same
            // rewards in the same order, so the same bits
            [[maybe_unused]] float er_m = 0.0f;
            [[maybe_unused]] int32_t el_m = 0;
            if constexpr (split_self_fetch(MODE)) {
                if (track) {
                    er_m = buf_ld(make_rsrc(a.ep_ret), off, 0);
                    el_m = (int32_t)(ep_clock0(a) - rec_ld_word(make_rsrc(a.rec), li, 2));
                    // wait for the two loads HERE, before the first store is in flight: left to the first use inside the drain loop the
                    // compiler's s_waitcnt vmcnt(0) would sit in the loop and wait for every outstanding trajectory store, every step
                    asm volatile("" : "+v"(er_m), "+v"(el_m));
                }
            }
            static_assert(!(RMAV_WIDE_DRAIN && split_self_fetch(MODE)), "the wide drain does not carry the episode statistics");
            auto episode_end = [&](float rw, float dn) {
                if constexpr (split_self_fetch(MODE)) {
                    if (track) {
                        er_m += rw;
                        el_m += 1;
                        if (dn != 0.0f) {
                            buf_st(make_rsrc(a.last_ret), off, 0, er_m);
                            rec_st_last_len(make_rsrc(a.rec), li, el_m);
                            er_m = 0.0f;
                            el_m = 0;
                        }
                    }
                }
            };
            auto fill = [&](int32_t c) {   // actions of chunk c: draw, hand over, write the action trajectory
                float *buf = lds_p + (c & 1) * ST_::A_HALF + lane;
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    const int32_t k = c * CH + j;
                    if (k < T) {
                        float act[NA];
                        random_action<K>(a.seed, env_id, a.t0 + (uint64_t)k, a.act_lo, a.act_hi, act);
#pragma unroll
                        for (int q = 0; q < NA; ++q) buf[(j * NA + q) * 64] = act[q];
                        if (a.act_out) {
                            float *dst_step = a.act_out + (int64_t)k * NA * tn;
                            if (aos) {
                                float *dst = dst_step + (int64_t)li * NA;
#pragma unroll
                                for (int q = 0; q < NA; ++q) dst[q] = act[q];
                            } else if (RMAV_WIDE_DRAIN && wide) {
                                // the tile the integrator will read is also the transposition buffer (LDS executes one
                                // wavefront's accesses in order)
                                wide_cols<AUX, NA>(buf - lane + j * NA * 64, make_rsrc(dst_step), wave_first * 4u, tcol, lane);
                            } else {
                                const rsrc_t ra = make_rsrc(dst_step);
#pragma unroll
                                for (int q = 0; q < NA; ++q) buf_st_aux<AUX>(ra, off, (uint32_t)q * tcol, act[q]);
                            }
                        }
                    }
                }
            };
            auto drain = [&](int32_t c) {  // obs / reward / done of chunk c: LDS -> trajectory
                const float *buf = lds_p + ST_::A_WORDS + (c & 1) * ST_::O_HALF + lane;
                if (RMAV_WIDE_DRAIN && wide) {
                    const float *tile = buf - lane;
#pragma unroll
                    for (int j = 0; j < CH; ++j) {
                        const int32_t k = c * CH + j;
                        if (k < T) {
                            const float *row = tile + j * ST_::O_ROW;
                            if constexpr (!DRAWS) {
                                if (a.act_out)
                                    wide_cols<AUX, NA>(row + ST_::ACT, make_rsrc(a.act_out + (int64_t)k * NA * tn), wave_first * 4u, tcol, lane);
                            }
                            if (a.obs_out) wide_cols<AUX, NS>(row, make_rsrc(a.obs_out + (int64_t)k * NS * tn), wave_first * 4u, tcol, lane);
                        }
                    }
                    // reward and done of the chunk's CH steps in one instruction each: lanes [16 j, 16 j + 16) take step j
                    const uint32_t sj = lane >> 4, eq = lane & 15u;
                    const int32_t k0 = c * CH;
                    if (sj < (uint32_t)CH && k0 + (int32_t)sj < T) {
                        const float *row = tile + sj * ST_::O_ROW;
                        if (a.rew_out) {
                            const float4 v = *reinterpret_cast<const float4 *>(row + ST_::REW + 4u * eq);
                            buf_st4_aux<AUX>(make_rsrc(a.rew_out + (int64_t)k0 * tn), (wave_first + 4u * eq) * 4u + sj * tcol, 0u, v);
                        }
                        if (a.done_out) {
                            const float4 d = *reinterpret_cast<const float4 *>(row + ST_::DONE + 4u * eq);
                            const uint32_t bytes = (d.x != 0.0f ? 1u : 0u) | (d.y != 0.0f ? 0x100u : 0u) | (d.z != 0.0f ? 0x10000u : 0u) |
                                                   (d.w != 0.0f ? 0x1000000u : 0u);
                            __builtin_amdgcn_raw_buffer_store_b32(bytes, make_rsrc(a.done_out + (int64_t)k0 * tn),
                                                                  wave_first + 4u * eq + sj * (uint32_t)tn, 0u, 0);
                        }
                    }
                    return;
                }
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    const int32_t k = c * CH + j;
                    if (k < T) {
                        const float *row = buf + j * ST_::O_ROW;
                        if constexpr (!DRAWS) {
                            if (a.act_out) {
                                float *dst_step = a.act_out + (int64_t)k * NA * tn;
                                float av[NA];
#pragma unroll
                                for (int q = 0; q < NA; ++q) av[q] = row[ST_::ACT + q * 64];
                                if (aos) {
                                    float *dst = dst_step + (int64_t)li * NA;
#pragma unroll
                                    for (int q = 0; q < NA; ++q) dst[q] = av[q];
                                } else {
                                    const rsrc_t ra = make_rsrc(dst_step);
#pragma unroll
                                    for (int q = 0; q < NA; ++q) buf_st_aux<AUX>(ra, off, (uint32_t)q * tcol, av[q]);
                                }
                            }
                        }
                        if (a.obs_out) {
                            float *dst_step = a.obs_out + (int64_t)k * NS * tn;
                            float o[NS];
                            if (aos) {
                                // batch-major: the integrator wrote [env][c]; read it back in output order, so the
                                // wavefront's 64 x NS floats leave as NS contiguous 256-byte stores.  The buffer
                                // descriptor covers exactly this wavefront's valid rows: clones are range-checked away.
                                const float *tile = row - lane;
                                const rsrc_t ro = make_rsrc_bounded(dst_step + (int64_t)wave_first * NS, aos_bytes);
#pragma unroll
                                for (int q = 0; q < NS; ++q) o[q] = tile[aos_rd[q]];
#pragma unroll
                                // the per-q term rides in the instruction's immediate offset (256 q <= 3840 < 4096), which the
                                // range check covers; an SGPR soffset is NOT range-checked and would let the clone rows
                                // of a ragged last wavefront land past this wavefront's valid rows
                                for (int q = 0; q < NS; ++q) buf_st_aux<AUX>(ro, lane * 4u + 256u * q, 0u, o[q]);
                            } else {
                                const rsrc_t ro = make_rsrc(dst_step);
#pragma unroll
                                for (int q = 0; q < NS; ++q) o[q] = row[q * 64];
#pragma unroll
                                for (int q = 0; q < NS; ++q) buf_st_aux<AUX>(ro, off, (uint32_t)q * tcol, o[q]);
                            }
                        }
                        if (a.rew_out) buf_st_aux<AUX>(make_rsrc(a.rew_out + (int64_t)k * tn), off, 0, row[ST_::REW]);
                        if (a.done_out)
                            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(row[ST_::DONE] != 0.0f ? 1 : 0),
                                                                 make_rsrc(a.done_out + (int64_t)k * tn), li, 0, 0);
                        episode_end(row[ST_::REW], row[ST_::DONE]);
                    }
                }
            };
            // Lean addressing (the common case: feature-major trajectories below 4 GiB per array).  The generic drain above
            // rebuilds a descriptor per array and step from an advancing 64-bit pointer and tests every optional output with a
            // scalar branch: ~45 scalar / branch instructions per env-step on a wavefront whose ~7 cycles per issued instruction
            // ARE the step time (SQ counters, profiles/r02/sq_counters.md: 76 SALU per 64 envs and step for both wavefronts).
            // Here each array has ONE descriptor for the whole launch - a missing output gets num_records = 0, so the hardware
            // range check drops its stores and no branch is needed - the component offsets q * 4N sit in vector registers
            // (computed once), and a step advances one scalar offset per array.
            if ((a.flags & F_LEAN) != 0) {
                static_assert(CH == 1, "one env-step per hand-over");
                constexpr int NQ = NS > NA ? NS : NA;
                uint32_t voff[NQ];
#pragma unroll
                for (int q = 0; q < NQ; ++q) voff[q] = off + (uint32_t)q * tcol;
                const rsrc_t rA = a.act_out ? make_rsrc(a.act_out) : make_rsrc_bounded(a.state, 0u);
                const rsrc_t rO = a.obs_out ? make_rsrc(a.obs_out) : make_rsrc_bounded(a.state, 0u);
                const rsrc_t rR = a.rew_out ? make_rsrc(a.rew_out) : make_rsrc_bounded(a.state, 0u);
                const rsrc_t rD = a.done_out ? make_rsrc(a.done_out) : make_rsrc_bounded(a.state, 0u);
                const uint32_t sA = (uint32_t)NA * tcol, sO = (uint32_t)NS * tcol, sR = tcol, sD = (uint32_t)tn;
                auto drain_l = [&](int32_t k) {   // obs / reward / done (and the controller's action) of step k: LDS -> trajectory
                    const float *row = lds_p + ST_::A_WORDS + (k & 1) * ST_::O_HALF + lane;
                    float o[NS];
#pragma unroll
                    for (int q = 0; q < NS; ++q) o[q] = row[q * 64];
                    const float rw = row[ST_::REW], dn = row[ST_::DONE];
                    if constexpr (!DRAWS) {
                        float av[NA];
#pragma unroll
                        for (int q = 0; q < NA; ++q) av[q] = row[ST_::ACT + q * 64];
#pragma unroll
                        for (int q = 0; q < NA; ++q) buf_st_aux<AUX>(rA, voff[q], (uint32_t)k * sA, av[q]);
                    }
#pragma unroll
                    for (int q = 0; q < NS; ++q) buf_st_aux<AUX>(rO, voff[q], (uint32_t)k * sO, o[q]);
                    buf_st_aux<AUX>(rR, off, (uint32_t)k * sR, rw);
                    __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(dn != 0.0f ? 1 : 0), rD, li, (uint32_t)k * sD, 0);
                    episode_end(rw, dn);
                };
                {
                    [[maybe_unused]] uint32_t blk[4] = {0u, 0u, 0u, 0u};   // 2-action kinds: the Philox block of the current pair of steps
                    [[maybe_unused]] bool blk_valid = false;
                    auto fill_l = [&](int32_t k) {   // actions of step k: draw, hand over, write the action trajectory
                        float *buf = lds_p + (k & 1) * ST_::A_HALF + lane;
                        float act[NA];
                        const uint64_t t = a.t0 + (uint64_t)k;
                        if constexpr (action_pairs<K>()) {
                            if ((t & 1u) == 0 || !blk_valid) {   // wave-uniform: one draw serves steps 2 j and 2 j + 1
                                random_block<K>(a.seed, env_id, t, blk);
                                blk_valid = true;
                            }
                            action_from_block<K>(blk, t, a.act_lo, a.act_hi, act);
                        } else {
                            random_action<K>(a.seed, env_id, t, a.act_lo, a.act_hi, act);
                        }
#pragma unroll
                        for (int q = 0; q < NA; ++q) buf[q * 64] = act[q];
#pragma unroll
                        for (int q = 0; q < NA; ++q) buf_st_aux<AUX>(rA, voff[q], (uint32_t)k * sA, act[q]);
                    };
                    if constexpr (DRAWS) {
                        fill_l(0);
                        if (nc >= 2) fill_l(1);
                    }
                    __syncthreads();                                   // B0
                    if constexpr (DRAWS) __syncthreads();              // B0x
                    if (nc >= 2) {
                        if constexpr (DRAWS) {
                            if (nc >= 3) fill_l(2);
                        }
                        __syncthreads();                               // B1
                    }
                    int32_t c = 2;
                    if constexpr (DRAWS && action_pairs<K>()) {
                        // One Philox block holds the actions of steps 2 j and 2 j + 1.  Written as `draw when t is even` inside
                        // fill_l the compiler hoists the draw out of the branch and every step pays its 20 quarter-rate multiplies
                        // (a third of the vector-pipe time of a 2-D pair): here the parity is in the structure of the loop instead.
                        auto fill_half = [&](int32_t k, const uint32_t (&b)[4], uint32_t odd) {
                            float *buf = lds_p + (k & 1) * ST_::A_HALF + lane;
                            float act[NA];
                            action_from_block<K>(b, (uint64_t)odd, a.act_lo, a.act_hi, act);
#pragma unroll
                            for (int q = 0; q < NA; ++q) buf[q * 64] = act[q];
#pragma unroll
                            for (int q = 0; q < NA; ++q) buf_st_aux<AUX>(rA, voff[q], (uint32_t)k * sA, act[q]);
                        };
                        if (c + 1 < nc && ((a.t0 + (uint64_t)(c + 1)) & 1u) != 0) {   // reach an even step
                            fill_l(c + 1);
                            drain_l(c - 2);
                            __syncthreads();                           // Bc
                            ++c;
                        }
                        for (; c + 2 < nc; c += 2) {
                            uint32_t b2[4];
                            random_block<K>(a.seed, env_id, a.t0 + (uint64_t)(c + 1), b2);
                            fill_half(c + 1, b2, 0u);
                            drain_l(c - 2);
                            __syncthreads();                           // Bc
                            fill_half(c + 2, b2, 1u);
                            drain_l(c - 1);
                            __syncthreads();                           // B(c + 1)
                        }
                        blk_valid = false;
                    }
                    for (; c + 1 < nc; ++c) {                          // steady state: no guards, no optional-output branches
                        if constexpr (DRAWS) fill_l(c + 1);
                        drain_l(c - 2);
                        __syncthreads();                               // Bc
                    }
                    if (nc >= 3) {                                     // c = nc - 1: nothing left to draw
                        drain_l(nc - 3);
                        __syncthreads();                               // B(nc - 1)
                    }
                }
                if (nc >= 2) drain_l(nc - 2);
                __syncthreads();                                   // B(nc)
                drain_l(nc - 1);
                return;
            }
            {
                if constexpr (DRAWS) {
                    fill(0);
                    if (nc >= 2) fill(1);
                }
                __syncthreads();                                   // B0
                if constexpr (DRAWS) __syncthreads();              // B0x
                for (int32_t c = 1; c < nc; ++c) {
                    if constexpr (DRAWS) {
                        if (c + 1 < nc) fill(c + 1);
                    }
                    if (c >= 2) drain(c - 2);
                    __syncthreads();                               // Bc
                }
            }
            if (nc >= 2) drain(nc - 2);
            __syncthreads();                                   // B(nc)
            drain(nc - 1);
            return;
        }
    }

    // ACT_POLICY: stage the policy weights into LDS once per launch (every thread of the block helps)
    if constexpr (is_policy(MODE)) {
        constexpr int NW4 = (MODE == ACT_POLICY ? PolicyLayout<NS>::TOTAL : MODE == ACT_POLICY_F32M ? Mfma32Layout::TOTAL : MfmaLayout::TOTAL) / 4;
        const float4 *src = reinterpret_cast<const float4 *>(a.policy_w);
        float4 *dst = reinterpret_cast<float4 *>(lds_w);
        for (int q = threadIdx.x; q < NW4; q += blockDim.x) dst[q] = src[q];
        if constexpr (NORM) stage_norm(lds_w + Mfma32Layout::TOTAL, nm.tab);   // k_rollout_nrm: the tables, behind the weights
        __syncthreads();
        if constexpr (MODE == ACT_POLICY_BF16) {
            scale_biases_for_tanh();
            __syncthreads();
        }
    }

    if (li < slice_end) {
        const rsrc_t r_state = make_rsrc(a.state);
        float s[NS];
#pragma unroll
        for (int c = 0; c < NS; ++c) s[c] = buf_ld(r_state, off, (uint32_t)c * col);
        float er = 0.0f;
        int32_t el = 0;
        // steps_beyond_done and the reset counter ride in registers for the whole launch: loading them
        // on demand (only lanes that terminate need them) would put one or two dependent HBM round
        // trips into every step of every wavefront that has a finishing lane (~57 % of them at the
        // 1.3 %/step termination rate of random actions).  One access of the env's record (EnvRec) brings both, and the
        // episode's start when tracking.
        const rsrc_t r_rec = make_rsrc(a.rec);
        int32_t sb;
        uint32_t rc;
        constexpr bool REC_WORDS = is_policy(MODE);   // the one-wavefront actors sit at their register limit: word accesses, no tuples
        // (TL: the running length is counted whether or not the handle tracks episodes)
        if (track) er = buf_ld(make_rsrc(a.ep_ret), off, 0);
        if constexpr (REC_WORDS) {
            sb = (int32_t)rec_ld_word(r_rec, li, 0);
            rc = rec_ld_word(r_rec, li, 1);
            if (TL || track) el = (int32_t)(ep_clock0(a) - rec_ld_word(r_rec, li, 2));
        } else if (TL || track) {
            const u32x3_t q = rec_ld3(r_rec, li);
            sb = (int32_t)q.x;
            rc = q.y;
            el = (int32_t)(ep_clock0(a) - q.z);
        } else {
            const u32x2_t q = rec_ld2(r_rec, li);
            sb = (int32_t)q.x;
            rc = q.y;
        }
        // (written back unconditionally at the end of the launch: neither copies of the loaded values - two registers of the
        // step loop - nor per-lane dirty masks - four scalar instructions per step - for 8 B per env and LAUNCH)
        const uint64_t env_id = a.env_base + (uint64_t)li;
        // per-env (domain-randomised) constants override the shared kernel arguments for this lane
        typename Env<K>::P pl = p_shared;
        ParamsT<double> pcl = pc_shared;
        if constexpr (K != REINMAV) {
            if (a.pe[0] || a.pe[1] || a.pe[2]) {
                const double m = a.pe[0] ? (double)a.pe[0][li] : (double)pc_shared.mass;
                const double ml = a.pe[1] ? (double)a.pe[1][li] : (double)pc_shared.load_mass;
                const double L = a.pe[2] ? (double)a.pe[2][li] : (double)pc_shared.L;
                override_params(pl, m, ml, L);
                override_params(pcl, m, ml, L);
            }
        }
        const typename Env<K>::P &p = pl;
        const ParamsT<double> &pc = pcl;
        // DS (k_rollout_ds): the wind of the running episode (reset index rc - 1: rc names the NEXT fresh state) and of the spare reset state,
        // the gust of the running block, and where the step stands in it (wave-uniform).  pl.gv is rewritten in front of every step.
        [[maybe_unused]] float ds_w[DS ? disturb_dim<K>() : 1], ds_q[DS ? disturb_dim<K>() : 1], spare_w[DS ? disturb_dim<K>() : 1];
        [[maybe_unused]] uint64_t ds_b = 0;
        [[maybe_unused]] int32_t ds_ph = 0;
        if constexpr (DS) {
            ds_b = ds.b0;
            ds_ph = ds.phase0;
            wind_draw(ds.spec(), a.seed, env_id, rc - 1u, ds_w);
            gust_draw(ds.spec(), a.seed, env_id, ds_b, ds_q);
#pragma unroll
            for (int i = 0; i < disturb_dim<K>(); ++i) spare_w[i] = 0.0f;
        }
#if RMAV_ROLLOUT_AL   // the *_al wrappers (alc: ActuatorCoef, al_m: the handle's [nA][N] array, al_sn: the handle has sensor noise): the filter state
                      // of this env rides in registers for the whole launch - loaded here, stored with the state behind the step loop
        float am[NA];
#if RMAV_ROLLOUT_SS   // the *_ss wrappers (ssc: StartCoef, ss_al: the handle has actuator lag, wave-uniform): without it no filter state exists
        const bool al_live = ss_al != 0u;
#pragma unroll
        for (int c = 0; c < NA; ++c) am[c] = 0.0f;
#else
        constexpr bool al_live = true;
#endif
#if RMAV_ROLLOUT_SS   // (the actor through the plain pointer, as for its store behind the step loop: with the descriptor under the branch
                      // one quadrotor2d-slungload kernel kept an unused 48-byte stack frame)
        if (al_live && is_policy(MODE)) {
#pragma unroll
            for (int c = 0; c < NA; ++c) am[c] = al_m[(int64_t)c * n + li];
        } else
#endif
        if (al_live) {
            const rsrc_t r_m = make_rsrc(al_m);
#pragma unroll
            for (int c = 0; c < NA; ++c) am[c] = buf_ld(r_m, off, (uint32_t)c * col);
        }
#endif
        double tenv = 0.0;
        if constexpr (K == REINMAV) tenv = a.env_time[li];

        // Spare reset state.  PMC counters (profiles/r01) show the fused kernel is instruction-issue bound
        // at C2: one wavefront per SIMD, ~4 cycles per instruction, SQ_ACTIVE_INST_ANY = 75 % of
        // SQ_WAVE_CYCLES.  Only ~1.3 % of the lanes terminate per step, but 57 % of the wavefronts
        // contain one, and each of those then executes the three Philox calls of reset_state() for the
        // whole wavefront: ~128 of the ~305 VALU instructions of an average step.  The state an env
        // will be reset to depends only on (seed, env id, reset counter), so for multi-step launches it
        // is drawn ONCE up front (all lanes busy, amortised over the launch) and the in-loop reset
        // becomes a predicated register copy.  A second termination of the same env inside one launch
        // falls back to drawing on demand.  Same counters, same bits either way.
        // (spare_in_lds<K, MODE>: one kernel keeps it in LDS instead, so that it does not occupy NS registers in the step loop)
        constexpr bool SPARE_LDS = spare_in_lds<K, MODE>();
        [[maybe_unused]] float spare[SPARE_LDS ? 1 : NS];
        [[maybe_unused]] float *lds_spare = nullptr;
        if constexpr (SPARE_LDS)
            lds_spare = lds_w + split_g * SplitTile<NS, NA, DRAWS>::WORDS +
                        (uint32_t)__builtin_amdgcn_readfirstlane(split_local >> 6) * SplitTile<NS, NA, DRAWS>::SPARE + (threadIdx.x & 63u);
        bool have_spare = false;
        // k_rollout_dr: the constants of the episode the spare state starts (the ranged parameters' elements)
        [[maybe_unused]] float spare_pe[3];
        if constexpr (DR) spare_pe[0] = spare_pe[1] = spare_pe[2] = 0.0f;
        if (K != REINMAV && auto_reset && a.n_steps >= 8) {   // ReinmavEnv.reset() is a no-op (reinmav_env.py:348-351)
            if constexpr (SPARE_LDS) {
                float sp[NS];
                reset_state<K>(a.seed, env_id, rc, sp);
#if RMAV_ROLLOUT_SS
                start_apply<NS>(ssc, sp);
#endif
#pragma unroll
                for (int c = 0; c < NS; ++c) lds_spare[c * 64] = sp[c];   // read back by this lane only: no barrier needed
            } else {
                reset_state<K>(a.seed, env_id, rc, spare);
#if RMAV_ROLLOUT_SS   // the spare is a START state: the draw under the handle's ranges (clone lanes compute the bits of the env they copy)
                start_apply<NS>(ssc, spare);
#endif
            }
            if constexpr (DR) range_draw(dr, a.seed, env_id, rc, spare_pe);   // the spare constants with the spare state
            if constexpr (DS) wind_draw(ds.spec(), a.seed, env_id, rc, spare_w);      // ... and the spare wind
            have_spare = true;
        }

        // ST_AOS_LDS: this wavefront's transposition tile and, per output dword j of the lane, where in the
        // tile the element lives (output element e = 64 j + lane is component e % NS of the wave's env e / NS)
        [[maybe_unused]] float *tile = nullptr;
        [[maybe_unused]] uint32_t tile_rd[NS];
        [[maybe_unused]] bool full_wave = false;
        [[maybe_unused]] uint32_t wave_obs_base = 0;
        if constexpr (ST == ST_AOS_LDS) {
            const uint32_t lane = threadIdx.x & 63u;
            // readfirstlane: tell the compiler these are wave-uniform (SGPR offsets, no waterfall loops)
            const uint32_t wave_first = __builtin_amdgcn_readfirstlane(gi - lane);
            tile = lds_w + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * AosTile<NS>::WORDS;
            full_wave = wave_first + 64u <= slice_end;
            wave_obs_base = wave_first * (uint32_t)(NS * 4);
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                const uint32_t e = 64u * j + lane;
                tile_rd[j] = (e / NS) * AosTile<NS>::STRIDE + (e % NS);
            }
        }

        // uniform cursors into the time-major trajectory buffers, advanced once per step
        const float *act_in = a.act_in;
        float *act_out = (!is_buffer(MODE) && !SPLIT) ? a.act_out : nullptr;   // SPLIT: the memory wavefront writes them
        float *obs_out = a.obs_out;
        float *rew_out = a.rew_out;
        uint8_t *done_out = a.done_out;

        float *logp_out = a.logp_out;
        float *val_out = a.val_out;
        float pol_std[4] = {0.f, 0.f, 0.f, 0.f};
        float pol_logp0 = 0.0f;   // - sum(logstd) - NA/2 * ln(2 pi)
        if constexpr (is_policy(MODE)) {
            float sl = 0.0f;
#pragma unroll
            for (int c = 0; c < NA; ++c) {
                const float ls = lds_w[(MODE == ACT_POLICY ? PolicyLayout<NS>::LOGSTD : MODE == ACT_POLICY_F32M ? Mfma32Layout::LOGSTD : MfmaLayout::LOGSTD) + c];
                pol_std[c] = expf(ls);
                if constexpr (NORM) pol_std[c] *= ar.noise;   // the action rule: std_eff (noise = 1: the same bits)
                sl += ls;
            }
            pol_logp0 = -sl - 0.5f * (float)NA * kLog2Pi;
        }

        // ACT_BUFFER: actions are prefetched one step ahead
        float act_pre[NA];
        auto load_actions = [&](const float *src_step, float (&dst)[NA]) {
            if (aos) {
                const float *src = src_step + (int64_t)li * NA;
#pragma unroll
                for (int c = 0; c < NA; ++c) dst[c] = src[c];
            } else {
                const rsrc_t r = make_rsrc(src_step);
#pragma unroll
                for (int c = 0; c < NA; ++c) dst[c] = buf_ld(r, off, (uint32_t)c * tcol);
            }
        };
        if constexpr (is_buffer(MODE)) load_actions(act_in, act_pre);
        // ACT_BUFFER_SPLIT: the caller's actions in bursts of D steps.  ring_fetch(k0) issues the loads of steps k0 .. k0 + D - 1 into
        // registers; D steps later ring_put() parks them in this lane's column of a private LDS ring (read back by this lane only: no
        // barrier) and the next burst is issued - so every load has D steps (~2 - 5 us) to arrive, and the only vmcnt wait of the
        // loop sees loads alone (this wavefront stores nothing inside the loop).
        [[maybe_unused]] float ring_pre[split_self_fetch(MODE) ? buf_prefetch<NA>() : 1][NA];
        [[maybe_unused]] float *lds_ring = nullptr;
        [[maybe_unused]] auto ring_fetch = [&](int32_t k0) {
            if constexpr (split_self_fetch(MODE)) {
#pragma unroll
                for (int d = 0; d < buf_prefetch<NA>(); ++d)
                    if (k0 + d < a.n_steps) load_actions(a.act_in + (int64_t)(k0 + d) * NA * tn, ring_pre[d]);
            }
        };
        [[maybe_unused]] auto ring_put = [&]() {
            if constexpr (split_self_fetch(MODE)) {
#pragma unroll
                for (int d = 0; d < buf_prefetch<NA>(); ++d)
#pragma unroll
                    for (int c = 0; c < NA; ++c) lds_ring[(d * NA + c) * 64] = ring_pre[d][c];
            }
        };
        if constexpr (split_self_fetch(MODE)) {
            using STB = SplitTile<NS, NA, DRAWS>;
            lds_ring = lds_w + split_g * (STB::WORDS + (spare_in_lds<K, MODE>() ? STB::SPARE : 0)) +
                       (uint32_t)__builtin_amdgcn_readfirstlane(split_local >> 6) * buf_ring_words<NA>() + (threadIdx.x & 63u);
            ring_fetch(0);
            ring_put();
            ring_fetch(buf_prefetch<NA>());
        }
        // two-wavefront modes whose memory wavefront supplies the actions: A(k + 1) is fetched from the hand-over tile while
        // step k is integrated (see the protocol above)
        [[maybe_unused]] float act_nx[NA];
        if constexpr (split_feeds_actions(MODE)) {
            static_assert(CH == 1, "one env-step per hand-over");
            __syncthreads();                                       // B0: A(0) and A(1) are in the tile
            const float *buf = lds_p + (threadIdx.x & 63u);
#pragma unroll
            for (int c = 0; c < NA; ++c) act_nx[c] = buf[c * 64];
            __syncthreads();                                       // B0x (waits for the read above: lgkmcnt(0) precedes s_barrier)
        }

#if RMAV_ROLLOUT_SN   // the *_sn wrappers: sn_o is the observation of s - what the nets read and the stored row holds.  Drawn ONCE per step, behind
                      // the dynamics and the reset of step k for the step counter t0 + k + 1: stored as row k, read by the actor of step k + 1
                      // and, after the last step, by the value net of value_out[n_steps]; the prologue draw at t0 serves step 0.
#define RMAV_OBS sn_o
        float sn_o[NS];
        if constexpr (is_policy(MODE)) {
#if RMAV_ROLLOUT_AL   // (... or, on a handle without sensor noise, the state itself: one wave-uniform branch per site)
            actuator_obs<NS>(al_sn, sn, a.seed, env_id, a.t0, s, sn_o);
#else
            float sn_z[NS];
            sensor_draw<NS>(a.seed, env_id, a.t0, sn_z);
            sensor_apply(sn, sn_z, s, sn_o);
#endif
        }
#else
#define RMAV_OBS s
#endif
        for (int32_t k = 0; k < a.n_steps; ++k) {
            float act[NA];
            if constexpr (is_mfma_policy(MODE)) {
                float x[16], mean[4], val0, z[4];
                if constexpr (NORM) {
                    norm_state16<NS>(lds_w + Mfma32Layout::TOTAL, RMAV_OBS, x);
                } else {
#pragma unroll
                    for (int c = 0; c < 16; ++c) x[c] = (c < NS) ? s[c] : 0.0f;
                }
                if constexpr (MODE == ACT_POLICY_BF16) policy_forward_mfma(x, mean, val0);
                else policy_forward_mfma32<NS>(x, mean, val0);
                gaussian4(a.seed, env_id, a.t0 + (uint64_t)k, z);
                float q = 0.0f;
#pragma unroll
                for (int c = 0; c < NA; ++c) {
                    act[c] = rfma(pol_std[c], z[c], mean[c]);
                    q = rfma(z[c], z[c], q);
                }
                if constexpr (NORM) q *= ar.noise;   // deterministic: the log-density of the mean
                buf_st(make_rsrc(logp_out), off, 0, rfma(-0.5f, q, pol_logp0));
                buf_st(make_rsrc(val_out), off, 0, val0);
                logp_out += n;
                val_out += n;
            } else if constexpr (MODE == ACT_POLICY) {
                using PL = PolicyLayout<NS>;
                XVec<PL::NSP> x;
#pragma unroll
                for (int c = 0; c < PL::NSP; ++c) x.v[c] = (c < NS) ? s[c] : 0.0f;
                const float4 m4 = mlp_forward<NS>(x, 0u);
                const float4 v4 = mlp_forward<NS>(x, (uint32_t)PL::NET);
                const float mean[4] = {m4.x, m4.y, m4.z, m4.w};
                const float val[1] = {v4.x};
                float z[4];
                gaussian4(a.seed, env_id, a.t0 + (uint64_t)k, z);
                float q = 0.0f;
#pragma unroll
                for (int c = 0; c < NA; ++c) {
                    act[c] = rfma(pol_std[c], z[c], mean[c]);
                    q = rfma(z[c], z[c], q);
                }
                buf_st(make_rsrc(logp_out), off, 0, rfma(-0.5f, q, pol_logp0));
                buf_st(make_rsrc(val_out), off, 0, val[0]);
                logp_out += n;
                val_out += n;
            } else if constexpr (is_buffer(MODE)) {
                // the action of step k was fetched while step k-1 was integrated (see the prefetch below): with one
                // wavefront per SIMD an action load issued at the top of its own step exposes a full memory
                // round trip per step (1.40 -> 1.26 us per env-step batch at 65 536 envs)
#pragma unroll
                for (int c = 0; c < NA; ++c) act[c] = act_pre[c];
                act_in += (int64_t)NA * tn;
                if (k + 1 < a.n_steps) load_actions(act_in, act_pre);
            } else if constexpr (MODE == ACT_RANDOM) {
                random_action<K>(a.seed, env_id, a.t0 + (uint64_t)k, a.act_lo, a.act_hi, act);
            } else if constexpr (split_feeds_actions(MODE)) {
#pragma unroll
                for (int c = 0; c < NA; ++c) act[c] = act_nx[c];
                // A(k + 1): written before B(k), its half is not rewritten before B(k + 1).  (Past the last step this reads a
                // stale half and the values are never used.)
                const float *buf = lds_p + ((k + 1) & 1) * SplitTile<NS, NA, true>::A_HALF + (threadIdx.x & 63u);
#pragma unroll
                for (int c = 0; c < NA; ++c) act_nx[c] = buf[c * 64];
            } else if constexpr (MODE == ACT_CONTROLLER_SPLIT) {
                if ((k % CH) == 0) __syncthreads();   // B(k / chunk): the output tile swaps halves
                env_control<K>(s, pc, act);
            } else if constexpr (split_self_fetch(MODE)) {
                if ((k % CH) == 0) __syncthreads();   // B(k / chunk), as the controller-driven integrator
                constexpr int D = buf_prefetch<NA>();
                static_assert((D & (D - 1)) == 0, "burst length: a power of two");
                const int32_t slot = k & (D - 1);
                if (slot == 0 && k > 0) {   // wave-uniform.  Burst boundary: the loads issued D steps ago go into the ring, the next D are issued
                    ring_put();
                    ring_fetch(k + D);
                }
                // (read at the top of its own step: fetching it one step ahead, as the random-action integrator does with its tile,
                // measured the same and costs the slung-load integrators the four registers they do not have)
                const float *rb = lds_ring + slot * (NA * 64);
#pragma unroll
                for (int c = 0; c < NA; ++c) act[c] = rb[c * 64];
            } else if constexpr (K == REINMAV) {
#pragma unroll
                for (int c = 0; c < NA; ++c) act[c] = 0.0f;   // the built-in controller runs inside every sub-step
            } else {
                env_control<K>(s, pc, act);
            }

            float dist = 0.0f;
            bool done;
            float r;
            if constexpr (K == REINMAV) {
                float fm0[4];
                Env<K>::step(s, act, MODE == ACT_CONTROLLER, tenv, p, fm0);
                if (MODE == ACT_CONTROLLER) {
#pragma unroll
                    for (int c = 0; c < NA; ++c) act[c] = fm0[c];   // reported action = command of sub-step 0
                }
                done = true;   // reinmav_env.py:110
                r = 90.0f;     // reinmav_env.py:111-116: 100 - 10, every step
            } else {
                // the disturbance of this agent step (one d for all of its sub-steps): the lane's gravity is g_vec + (w + q)
                if constexpr (DS) disturb_apply(pl, p_shared, ds_w, ds_q);
                if constexpr (FS) {
                    // frame skip (FrameSkipArgs): the action - clipped ONCE, in front of the loop - is held for up to fs.k sub-steps, each
                    // an ordinary step with the reward / steps_beyond_done machine behind it; a lane leaves at its first termination,
                    // the wavefront when no lane is live.  What follows sees (s, r, done) as after one step.
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
#if RMAV_ROLLOUT_AL   // actuator lag: the filter advances in front of every dynamics sub-step, which reads m; c_rw and the stored action keep the command
                            actuator_step<NA>(alc, am, ca);
#if RMAV_ROLLOUT_SS   // (a start spec without actuator lag: the command itself - a select, not a branch around the filter, which cost the
                      // quadrotor3d-slungload buffer kernels six registers and a wave of occupancy)
#pragma unroll
                            for (int c = 0; c < NA; ++c) am[c] = al_live ? am[c] : ca[c];
#endif
                            Env<K>::step(s, am, p, dist, term);
#else
                            Env<K>::step(s, ca, p, dist, term);
#endif
#if RMAV_ROLLOUT_TC   // the termination rules (tc: TermArgs; rmav_term.hpp): one flag for everything downstream
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
                if constexpr (NORM) {   // the action rule: the dynamics take the clipped action, `act` (stored below) stays what the policy drew
                    float ca[NA];
#pragma unroll
                    for (int c = 0; c < NA; ++c) ca[c] = act_clip(ar, act[c]);
                    Env<K>::step(s, ca, p, dist, done);
                } else {
                    Env<K>::step(s, act, p, dist, done);
                }
                // reward / steps_beyond_done machine  (quadrotor3d.py:112-122 and siblings)
                r = -dist;
                if (done) {
                    r = (sb < 0) ? 1.0f : 0.0f;
                    sb = (sb < 0) ? 0 : sb + 1;
                }
                }
            }
            if (act_out) {
                if (aos) {   // 8 / 16 bytes per lane, contiguous across the wavefront: already coalesced
                    float *dst = act_out + (int64_t)li * NA;
#pragma unroll
                    for (int c = 0; c < NA; ++c) {
                        if constexpr (ST == ST_AOS_LDS) __builtin_nontemporal_store(act[c], dst + c);
                        else dst[c] = act[c];
                    }
                } else {
                    const rsrc_t ra = make_rsrc(act_out);
#pragma unroll
                    for (int c = 0; c < NA; ++c) buf_st_aux<AUX>(ra, off, (uint32_t)c * tcol, act[c]);
                }
                act_out += (int64_t)NA * tn;
            }
            // Time limit: after the reference's reward / steps_beyond_done machine (r and sb are the step's own), before the episode
            // hand-off below - a step that reaches the limit without terminating ends the episode as truncated (termination wins).
            // el counts the steps of the running episode before this one.  The truncated flag of a finished episode is stored here.
            // (Declared only inside this block: a dead `trunc` variable in the kernels without a limit perturbed their register
            // allocation.)
            if constexpr (TL) {
                const bool trunc = !done && el + 1 >= tl.max_steps;
                done = done || trunc;
                if (done) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(trunc ? 1 : 0), make_rsrc(tl.last_trunc), li, 0, 0);
                // k_rollout_boot: the bootstrap term of a truncated step = the value net on the state the reset below replaces.  The ballot
                // is wave-uniform and non-zero on about one step in max_steps; only the value net runs (value_forward_mfma32: the
                // call that produces val_out, on the same operands).
                if constexpr (BOOT) {
                    float bv = 0.0f;
                    if (__ballot(trunc) != 0) {
                        float xf[16];
#if RMAV_ROLLOUT_SN   // V of the terminal OBSERVATION: the pre-reset state under the z of this step's row (a second evaluation of the draw, on
                      // about one step in max_steps - instead of NS registers of z held across the reset)
                        if constexpr (NORM) {
                            float sf[NS];
#if RMAV_ROLLOUT_AL
                            actuator_obs<NS>(al_sn, sn, a.seed, env_id, a.t0 + (uint64_t)k + 1u, s, sf);
#else
                            {
                                float sn_z[NS];
                                sensor_draw<NS>(a.seed, env_id, a.t0 + (uint64_t)k + 1u, sn_z);
                                sensor_apply(sn, sn_z, s, sf);
                            }
#endif
                            norm_state16<NS>(lds_w + Mfma32Layout::TOTAL, sf, xf);
                        } else {
#else
                        if constexpr (NORM) {
                            norm_state16<NS>(lds_w + Mfma32Layout::TOTAL, s, xf);
                        } else {
#endif
#pragma unroll
                            for (int c = 0; c < 16; ++c) xf[c] = (c < NS) ? s[c] : 0.0f;
                        }
                        const float vf = value_forward_mfma32<NS>(xf);
                        if (trunc) bv = vf;
                    }
                    buf_st(make_rsrc(bt.boot_out + (int64_t)k * n), off, 0, bv);
                    // (a plain store: a second buffer descriptor here cost the quadrotor2d kernel a stack frame)
                    if (bt.trunc_out) bt.trunc_out[(int64_t)k * n + li] = (uint8_t)(trunc ? 1 : 0);
                }
            }

            // End of an episode (statistics) and auto-reset.  A lane that terminates again in the same launch has no spare reset
            // state left: draw one first, skipped with ONE wave-uniform branch; what remains on the common path is a single predicated
            // copy (the nested form - copy the spare OR draw - cost a dozen exec-mask instructions per step).  The draw costs the
            // wavefront its ~130 instructions whatever the number of lanes in it, so EVERY lane without a spare takes one then (its
            // reset counter already names its next episode): one draw per wavefront serves all the lanes that have used theirs up,
            // instead of one draw per second termination (the 2-D kinds under random actions: an on-demand draw in most steps).
            //
            // Controller-driven and caller-action rollouts (SKIP_QUIET): all of it sits behind ONE more wave-uniform branch, and a
            // step in which no lane of the wavefront finishes (every step of a hovering rollout) skips the ~25 predicated
            // instructions of the episode hand-off and the reset copy: 65 536 envs, controller-driven, same box, quadrotor3d
            // 47.4 -> 45.8 us, quadrotor2d 34.8 -> 31.2, quadrotor3d-slungload 71.5 -> 66.3.  Under random actions most wavefronts
            // have a finishing lane in most steps and the extra branch costs 1-3 %, so there the block stays predicated.  The
            // bookkeeping of the two forms differs on purpose and is written out in each; the reset behind it is the same statements
            // and is ONE fragment, rmav_rollout_reset.inc, included in both places.  (Shared as text rather than as a lambda: the register
            // allocation of the 1024-thread kernels is tight enough to spill with the latter - tests/test_resource_usage.py.)
            constexpr bool SKIP_QUIET = MODE == ACT_CONTROLLER || MODE == ACT_CONTROLLER_SPLIT || is_buffer(MODE) || MODE == ACT_BUFFER_SPLIT;
            if constexpr (SKIP_QUIET) {
                if (track) {
                    er += r;
                    el += 1;
                } else if (TL) {
                    el += 1;
                }
                if (__ballot(done) != 0) {
                    if constexpr (TL) {
                        if (done && !track) el = 0;
                    }
                    if (track && done) {
                        if constexpr (!split_self_fetch(MODE)) {   // (ACT_BUFFER_SPLIT: the memory wavefront writes them)
                            buf_st(make_rsrc(a.last_ret), off, 0, er);
                            rec_st_last_len(make_rsrc(a.rec), li, el);
                        }
                        if (valid && !(HALF && (threadIdx.x & 32u))) {   // (the second copy of an env does not count)
                            fin_n += 1;
                            fin_len += (unsigned int)el;
                            fin_ret += er;
                        }
                        er = 0.0f;
                        el = 0;
                    }
#include "rmav_rollout_reset.inc"
                }
            } else {
                if (track) {
                    er += r;
                    el += 1;
                    if (done) {
                        buf_st(make_rsrc(a.last_ret), off, 0, er);
                        rec_st_last_len(make_rsrc(a.rec), li, el);
                        if (valid && !(HALF && (threadIdx.x & 32u))) {   // (the second copy of an env does not count)
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
#include "rmav_rollout_reset.inc"
            }
            if constexpr (SPLIT) {
                // hand obs / reward / done (and the controller's action) to the memory wavefront; it drains this
                // half two barriers later
                using ST_ = SplitTile<NS, NA, DRAWS>;
                float *row = lds_p + ST_::A_WORDS + ((k / CH) & 1) * ST_::O_HALF + (k % CH) * ST_::O_ROW +
                             (threadIdx.x & 63u);
                {   // (handed over also when no obs trajectory was asked for: a uniform branch here costs every step)
                    if (aos) {   // env-major for the batch-major drain
                        float *mine = row + (threadIdx.x & 63u) * (ST_::OBS_STRIDE - 1);
#pragma unroll
                        for (int c = 0; c < NS; ++c) mine[c] = s[c];
                    } else {
#pragma unroll
                        for (int c = 0; c < NS; ++c) row[c * 64] = s[c];
                    }
                }
                row[ST_::REW] = r;
                row[ST_::DONE] = done ? 1.0f : 0.0f;
                if constexpr (!DRAWS) {
#pragma unroll
                    for (int c = 0; c < NA; ++c) row[ST_::ACT + c * 64] = act[c];
                }
                if constexpr (split_feeds_actions(MODE)) __syncthreads();   // B(k + 1): O(k) handed over, A(k + 2) may be written
#if RMAV_ROLLOUT_SN   // the *_sn wrappers (kernel argument sn: SensorArgs): the observation of the state after this step and its reset, under
                      // the z of the step counter after the step; s itself - the dynamics, the reward, the state stored in place - stays true
            } else if (is_policy(MODE) || obs_out) {   // (an actor reads the observation whether or not the caller stores it)
#if RMAV_ROLLOUT_AL
                actuator_obs<NS>(al_sn, sn, a.seed, env_id, a.t0 + (uint64_t)k + 1u, s, sn_o);
#else
                {
                    float sn_z[NS];
                    sensor_draw<NS>(a.seed, env_id, a.t0 + (uint64_t)k + 1u, sn_z);
                    sensor_apply(sn, sn_z, s, sn_o);
                }
#endif
                if (obs_out) {
                    if (aos) {
                        float *dst = obs_out + (int64_t)li * NS;
#pragma unroll
                        for (int c = 0; c < NS; ++c) dst[c] = sn_o[c];
                    } else {
                        const rsrc_t ro = make_rsrc(obs_out);
#pragma unroll
                        for (int c = 0; c < NS; ++c) buf_st_aux<AUX>(ro, off, (uint32_t)c * tcol, sn_o[c]);
                    }
                    obs_out += (int64_t)NS * tn;
                }
#else
            } else if (obs_out) {
                if (ST == ST_AOS_LDS && full_wave) {
                    // all 64 lanes are here (full_wave is wave-uniform); LDS executes one wavefront's
                    // instructions in order, the fences only pin the compiler's ordering
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    float *row = tile + (threadIdx.x & 63u) * AosTile<NS>::STRIDE;
#pragma unroll
                    for (int c = 0; c < NS; ++c) row[c] = s[c];
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    const rsrc_t ro = make_rsrc(obs_out);
                    const uint32_t voff = (threadIdx.x & 63u) * 4u;
#pragma unroll
                    for (int j = 0; j < NS; ++j) buf_st_aux<AUX>(ro, voff, wave_obs_base + 256u * j, tile[tile_rd[j]]);
                } else if (aos) {
                    float *dst = obs_out + (int64_t)li * NS;
#pragma unroll
                    for (int c = 0; c < NS; ++c) dst[c] = s[c];
                } else {
                    const rsrc_t ro = make_rsrc(obs_out);
#pragma unroll
                    for (int c = 0; c < NS; ++c) buf_st_aux<AUX>(ro, off, (uint32_t)c * tcol, s[c]);
                }
                obs_out += (int64_t)NS * tn;
#endif
            }
            if (!SPLIT && rew_out) {
                buf_st_aux<AUX>(make_rsrc(rew_out), off, 0, r);
                rew_out += tn;
            }
            if (!SPLIT && done_out) {
                __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(done ? 1 : 0), make_rsrc(done_out), li, 0, 0);
                done_out += tn;
            }
            // DS: the next agent step's place in the gust sequence; a new block draws its gust (wave-uniform: kernel arguments only)
            if constexpr (DS) {
                if (++ds_ph >= ds.spec().hold) {
                    ds_ph = 0;
                    ++ds_b;
                    if (k + 1 < a.n_steps) gust_draw(ds.spec(), a.seed, env_id, ds_b, ds_q);
                }
            }
        }
        if constexpr (MODE == ACT_CONTROLLER_SPLIT || split_self_fetch(MODE)) __syncthreads();   // B(nc): the last step's outputs are in LDS

        if constexpr (is_mfma_policy(MODE)) {   // bootstrap value of the state the rollout ends in
            float x[16], mean[4], val0;
            if constexpr (NORM) {
                norm_state16<NS>(lds_w + Mfma32Layout::TOTAL, RMAV_OBS, x);
            } else {
#pragma unroll
                for (int c = 0; c < 16; ++c) x[c] = (c < NS) ? s[c] : 0.0f;
            }
            if constexpr (MODE == ACT_POLICY_BF16) policy_forward_mfma(x, mean, val0);
            else policy_forward_mfma32<NS>(x, mean, val0);
            buf_st(make_rsrc(val_out), off, 0, val0);
        }
        if constexpr (MODE == ACT_POLICY) {   // bootstrap value of the state the rollout ends in
            using PL = PolicyLayout<NS>;
            XVec<PL::NSP> x;
#pragma unroll
            for (int c = 0; c < PL::NSP; ++c) x.v[c] = (c < NS) ? s[c] : 0.0f;
            const float4 v4 = mlp_forward<NS>(x, (uint32_t)PL::NET);
            buf_st(make_rsrc(val_out), off, 0, v4.x);
        }
#pragma unroll
        for (int c = 0; c < NS; ++c) buf_st(r_state, off, (uint32_t)c * col, s[c]);
#if RMAV_ROLLOUT_AL   // the filter state, with the state (vector stores; clone lanes store the bits of the lane they copy, as for the state).  The
                      // actor through the plain pointer: with a third buffer descriptor here one quadrotor2d-slungload kernel kept a 48-byte
                      // stack frame; the others through a descriptor: the 64-bit address costs quadrotor3d-slungload a wave of occupancy
        if (!al_live) {
        } else if constexpr (is_policy(MODE)) {
#pragma unroll
            for (int c = 0; c < NA; ++c) al_m[(int64_t)c * n + li] = am[c];
        } else {
            const rsrc_t r_m = make_rsrc(al_m);
#pragma unroll
            for (int c = 0; c < NA; ++c) buf_st(r_m, off, (uint32_t)c * col, am[c]);
        }
#endif
        if constexpr (MODE == ACT_BUFFER_CTRL && K != REINMAV) {   // control() of the state this launch leaves behind
            float a2[NA];
            env_control<K>(s, pc, a2);
            if (aos) {
                float *dst = a.ctrl_out + (int64_t)li * NA;
#pragma unroll
                for (int c = 0; c < NA; ++c) dst[c] = a2[c];
            } else {
                const rsrc_t rc2 = make_rsrc(a.ctrl_out);
#pragma unroll
                for (int c = 0; c < NA; ++c) buf_st(rc2, off, (uint32_t)c * col, a2[c]);
            }
        }
        if constexpr (K == REINMAV) a.env_time[li] = tenv;
        if (track) buf_st(make_rsrc(a.ep_ret), off, 0, er);
        if constexpr (is_policy(MODE)) {
            rec_st_word(make_rsrc(a.rec), li, 0, (uint32_t)sb);
            rec_st_word(make_rsrc(a.rec), li, 1, rc);
            if (TL || track) rec_st_word(make_rsrc(a.rec), li, 2, ep_clock0(a) + (uint32_t)a.n_steps - (uint32_t)el);
        } else if (TL || track) {
            rec_st3(make_rsrc(a.rec), li, u32x3_t{(uint32_t)sb, rc, ep_clock0(a) + (uint32_t)a.n_steps - (uint32_t)el});
        } else {
            rec_st2(make_rsrc(a.rec), li, u32x2_t{(uint32_t)sb, rc});
        }
    }

    if (track) {
        // Episode totals: each wavefront owns one slot of a [ceil(N/64)] partials array, so the adds never
        // contend (same-address device atomics cost ~12 ns each: ~600 finishing waves per step made the
        // single-step kernel 20 us slower than its memory time).  The adds are result-less atomics:
        // fire-and-forget at the L2, no load -> add -> store round trip at the tail of the kernel.
        // rmav_episode_totals sums the slots.
        Totals *slot = a.totals + (gi >> 6);
        if (a.n_steps == 1) {
            // single-step launches are latency-bound (~4.5 us): three 6-deep shuffle reductions at the tail of
            // the kernel cost ~0.4 us, while on average fewer than one lane per wavefront finishes an episode
            // - let those lanes add to the wave's slot themselves.
            if (fin_n != 0) {
                atomicAdd(&slot->episodes, (unsigned long long)fin_n);
                atomicAdd(&slot->length_sum, (unsigned long long)fin_len);
                atomicAdd(&slot->return_sum, (double)fin_ret);
            }
        } else if (__ballot(fin_n != 0) != 0) {
            // (the matrix-core actors keep ds_bpermute out of their kernels: rmav_policy_mfma.hpp, xor32)
            const unsigned int wn = is_mfma_policy(MODE) ? wave_sum_x(fin_n) : wave_sum(fin_n);
            const unsigned int wl = is_mfma_policy(MODE) ? wave_sum_x(fin_len) : wave_sum(fin_len);
            const float wr = is_mfma_policy(MODE) ? wave_sum_x(fin_ret) : wave_sum(fin_ret);
            if ((threadIdx.x & 63) == 0) {
                atomicAdd(&slot->episodes, (unsigned long long)wn);
                atomicAdd(&slot->length_sum, (unsigned long long)wl);
                atomicAdd(&slot->return_sum, (double)wr);
            }
        }
    }

    if (a.xsend) {   // wave-uniform.  Snapshot for the statistics exchange, then this wavefront's arrival word.
        // The loads see this lane's own stores of the step loop (same address, same lane: program order); the stores are
        // agent-scope (written through to the level the other XCDs' wavefronts and the next kernel read from), and
        // vmcnt(0) = they have been acknowledged there before the arrival word goes out.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (valid && !(HALF && (threadIdx.x & 32u))) {
            const float lr = a.last_ret[li];
            const int32_t ll = a.rec[li].last_len;
            __hip_atomic_store(a.xsend + li, __builtin_bit_cast(int32_t, lr), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.xsend + a.xcmax + li, ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // one word per wavefront that owns envs (its lane 0 owns the first of them): 64 envs each, 32 in the fp32-MFMA mode
        if ((threadIdx.x & 63u) == 0 && valid)
            __hip_atomic_store(a.xarrive + (HALF ? (ge >> 5) : (ge >> 6)), a.xseq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#undef RMAV_OBS

// rmav_pair_epilogue.inc - what the stepping wavefront leaves behind after its last step: the last statements of both pair bodies.
//   expects:  K, NS, the constexpr bool TL, the kernel argument a; r_state (the descriptor of a.state), s, tenv, er, el, sb, rc,
//             fin_n, fin_len, fin_ret, gi, li, lane, col, off, valid, track
//   defines:  nothing that outlives it
//   modifies: global memory only: the state, the env time (REINMAV), the running return and the record (EnvRec: with the episode's
//             start when tracking or TL), this wavefront's slot of the episode totals, and - armed - the statistics-exchange snapshot
//             with this wavefront's arrival word
//   barriers: behind the last barrier of the step loop; none follows (the helper wavefront has returned or is draining the last row)
#pragma unroll
    for (int c = 0; c < NS; ++c) buf_st(r_state, off, (uint32_t)c * col, s[c]);
#if RMAV_PAIR_AL   // the filter state, with the state (vector stores; clone lanes store the bits of the lane they copy, as for the state)
    if (al_live) {
        const rsrc_t r_m = make_rsrc(al_m);
#pragma unroll
        for (int c = 0; c < NA; ++c) buf_st(r_m, off, (uint32_t)c * col, am[c]);
    }
#endif
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

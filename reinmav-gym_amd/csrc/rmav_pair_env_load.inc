// rmav_pair_env_load.inc - what the stepping wavefront (the actor of rmav_pair_body.inc, wavefront A of rmav_pair_shared_body.inc)
// carries through the step loop besides the state: the first statements of its part in both pair bodies.
//   expects:  K, NS, NA, L (MfmaLayout), the constexpr bools TL and NORM, the preprocessor flag RMAV_PAIR_DR (set by the *_dr wrappers
//             around the include of the BODY, rmav_policy_pair.hpp; a nested include sees it), the kernel arguments a, p_shared,
//             pc_shared, ar and - RMAV_PAIR_DR - dr; logstd, env_id, li, off, T, track, auto_reset
//   defines:  the episode totals of this lane fin_n, fin_len, fin_ret; the running episode er (return), el (length); the env's record
//             sb (steps_beyond_done), rc (reset counter); the env's constants pl and the reference p the dynamics take; tenv; the spare
//             reset state spare[NS] with have_spare and - RMAV_PAIR_DR - the constants of the episode it starts, spare_pe[3]; pol_std[4];
//             - RMAV_PAIR_DS (the *_ds wrappers; kernel argument ds: DisturbRef) - the wind ds_w, the gust ds_q, the gust block ds_b and the phase ds_ph
//   modifies: nothing else (loads only: a.ep_ret, a.rec, a.pe, a.env_time)
//   barriers: in front of the barrier that opens the step loop (B / P): it reads logstd, not the tiles
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
#if RMAV_PAIR_SS   // the spare is a START state: the draw under the handle's ranges (clone lanes compute the bits of the env they copy)
        start_apply<NS>(ssc, spare);
#endif
#if RMAV_PAIR_DR
        range_draw(dr, a.seed, env_id, rc, spare_pe);
#endif
        have_spare = true;
    }
#if RMAV_PAIR_DS   // the *_ds kernels: the wind of the running episode (reset index rc - 1: rc names the NEXT fresh state), the gust of the
                   // running block and where the step stands in it (wave-uniform); a reset redraws the wind itself - no spare wind in registers
    float ds_w[disturb_dim<K>()], ds_q[disturb_dim<K>()];
    uint64_t ds_b = ds.b0;
    int32_t ds_ph = ds.phase0;
    wind_draw(ds.spec(), a.seed, env_id, rc - 1u, ds_w);
    gust_draw(ds.spec(), a.seed, env_id, ds_b, ds_q);
#endif
#if RMAV_PAIR_AL   // the *_al kernels (alc: ActuatorCoef, al_m: the handle's [nA][N] array): the filter state of this env, which belongs to the
                   // wavefront that integrates - in registers through the launch, stored by rmav_pair_epilogue.inc
    float am[NA];
#if RMAV_PAIR_SS   // the *_ss kernels (ssc: StartCoef, ss_al: the handle has actuator lag, wave-uniform): without it no filter state exists
    const bool al_live = ss_al != 0u;
#pragma unroll
    for (int c = 0; c < NA; ++c) am[c] = 0.0f;
#else
    constexpr bool al_live = true;
#endif
    if (al_live) {
        const rsrc_t r_m = make_rsrc(al_m);
#pragma unroll
        for (int c = 0; c < NA; ++c) am[c] = buf_ld(r_m, off, (uint32_t)c * col);
    }
#endif
    float pol_std[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NA; ++c) pol_std[c] = NORM ? expf(logstd[c]) * ar.noise : expf(logstd[c]);   // the action rule: std_eff

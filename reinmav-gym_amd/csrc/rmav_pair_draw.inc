// rmav_pair_draw.inc - the noise draw of the helper wavefront (the critic of rmav_pair_body.inc, wavefront B of
// rmav_pair_shared_body.inc): the first statements of its branch in both pair bodies.
//   expects:  NA, PT (PairTile), the constexpr bool NORM, the kernel arguments a (seed, t0, logp_out, val_out) and ar (ActRuleArgs);
//             logstd (the LDS copy of the policy's log-std, after the staging barriers), ztile (this lane's word of the pair's noise
//             tile), env_id, n, off
//   defines:  sl, logp0, the output cursors logp_out and val_out, and the lambda draw(k): z of step k into half k & 1 of the noise
//             tile, the log-probability of the action it will make into logp_out
//   modifies: nothing until draw is called; each call advances logp_out by one step (val_out is the includer's to advance)
//   barriers: none; the includer calls draw(0) in front of the barrier that opens the step loop and draw(k + 1) in front of the one
//             that ends step k
        float sl = 0.0f;
#pragma unroll
        for (int c = 0; c < NA; ++c) sl += logstd[c];
        const float logp0 = -sl - 0.5f * (float)NA * kLog2Pi;   // - sum(logstd) - NA/2 ln(2 pi)
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

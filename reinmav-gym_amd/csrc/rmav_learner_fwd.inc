// rmav_learner_fwd.inc - the head of a tile in learner_net (rmav_learner.hpp) and k_trunk_grad (rmav_learner_shared.hpp): this lane's
// sample, the observation tile with its normalisation, and the two hidden layers forward.
//   expects:  A (idx, obs, obs_pitch, norm_tab, batch), S with the weights staged, t, rb, cb, ns, tile
//   defines:  s (the lane's sample of the tile), j, live (j < batch), jc, col (the sample's column in the caller's arrays; a tail
//             lane's is the last sample's)
//   modifies: S.x (rows >= ns zero), S.h1 and S.h2 (tanh of layers 1 and 2)
//   barriers: three, behind x, h1 and h2; the last is the fragment's last statement
        // ---- the observation tile: x[c][s], rows >= ns zero; a tail lane reads the last sample's column ------------------------------
        const int s = t & 63;
        const int64_t j = tile * kLrnTile + s;
        const bool live = j < A.batch;
        const int64_t jc = live ? j : (int64_t)A.batch - 1;
        const int64_t col = A.idx ? A.idx[jc] : jc;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = (t >> 6) + 4 * q;
            float x = 0.0f;
            if (c < ns) {
                x = A.obs[(int64_t)c * A.obs_pitch + col];
                if (A.norm_tab) {   // THE arithmetic of include/rmav_ppo.h, uncontracted
                    const float lim = A.norm_tab[32];
                    x = (x - A.norm_tab[c]) * A.norm_tab[16 + c];
                    x = fminf(fmaxf(x, -lim), lim);
                }
            }
            S.x[c * kLrnPitch + s] = x;
        }
        __syncthreads();
        // ---- forward ------------------------------------------------------------------------------------------------------------------
        {
            float acc[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[r][q] = S.b1[rb + 16 * r];
            lrn_gemm(S.w1t, S.x, ns, rb, cb, acc);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                *reinterpret_cast<float4 *>(&S.h1[(rb + 16 * r) * kLrnPitch + 4 * cb]) =
                    make_float4(tanhf(acc[r][0]), tanhf(acc[r][1]), tanhf(acc[r][2]), tanhf(acc[r][3]));
        }
        __syncthreads();
        {
            float acc[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[r][q] = S.b2[rb + 16 * r];
            lrn_gemm(S.w2t, S.h1, 64, rb, cb, acc);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                *reinterpret_cast<float4 *>(&S.h2[(rb + 16 * r) * kLrnPitch + 4 * cb]) =
                    make_float4(tanhf(acc[r][0]), tanhf(acc[r][1]), tanhf(acc[r][2]), tanhf(acc[r][3]));
        }
        __syncthreads();

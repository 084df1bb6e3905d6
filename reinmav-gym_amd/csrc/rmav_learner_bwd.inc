// rmav_learner_bwd.inc - the tail of a tile in learner_net (rmav_learner.hpp) and k_trunk_grad (rmav_learner_shared.hpp): dW2,
// delta 1 and dW1, from delta 2 down.
//   expects:  S.h2 = delta 2 (behind the includer's barrier), S.h1 = tanh of layer 1, S.x, S.w2n, t's rb and cb
//   defines:  nothing
//   modifies: S.h1 (delta 1 in place); the thread's accumulators g2[r][c], gb1[r], g1[r]
//   barriers: three, behind dW2, delta 1 and dW1; the last ends the tile and is the fragment's last statement
        // ---- dW2 += d2 . h1^T: thread (rows rb + 16 r of d2) x (rows cb + 16 c of h1), K = the tile's samples -------------------------
        for (int s4 = 0; s4 < kLrnTile; s4 += 4) {
            float4 d[4], h[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) d[r] = lds4(&S.h2[(rb + 16 * r) * kLrnPitch + s4]);
#pragma unroll
            for (int c = 0; c < 4; ++c) h[c] = lds4(&S.h1[(cb + 16 * c) * kLrnPitch + s4]);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    g2[r][c] = fmaf(d[r].x, h[c].x, g2[r][c]);
                    g2[r][c] = fmaf(d[r].y, h[c].y, g2[r][c]);
                    g2[r][c] = fmaf(d[r].z, h[c].z, g2[r][c]);
                    g2[r][c] = fmaf(d[r].w, h[c].w, g2[r][c]);
                }
        }
        __syncthreads();
        // ---- delta 1 = (W2^T d2) * (1 - h1^2), in place -------------------------------------------------------------------------------
        {
            float acc[4][4] = {};
            lrn_gemm(S.w2n, S.h2, 64, rb, cb, acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float4 *hp = reinterpret_cast<float4 *>(&S.h1[(rb + 16 * r) * kLrnPitch + 4 * cb]);
                const float4 h = *hp;
                const float4 dl = make_float4(acc[r][0] * fmaf(-h.x, h.x, 1.0f), acc[r][1] * fmaf(-h.y, h.y, 1.0f),
                                              acc[r][2] * fmaf(-h.z, h.z, 1.0f), acc[r][3] * fmaf(-h.w, h.w, 1.0f));
                *hp = dl;
                gb1[r] += (dl.x + dl.y) + (dl.z + dl.w);
            }
        }
        __syncthreads();
        // ---- dW1 += d1 . x^T: thread (rows rb + 16 r of d1) x (row cb of x; rows >= ns are zero) --------------------------------------
        for (int s4 = 0; s4 < kLrnTile; s4 += 4) {
            const float4 x = lds4(&S.x[cb * kLrnPitch + s4]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float4 d = lds4(&S.h1[(rb + 16 * r) * kLrnPitch + s4]);
                g1[r] = fmaf(d.x, x.x, g1[r]);
                g1[r] = fmaf(d.y, x.y, g1[r]);
                g1[r] = fmaf(d.z, x.z, g1[r]);
                g1[r] = fmaf(d.w, x.w, g1[r]);
            }
        }
        __syncthreads();   // (the next tile overwrites x and h1)

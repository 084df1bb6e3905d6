// rmav_learner_pg.inc - the policy term of sample s and the deltas of the mean rows, on wave 0: learner_net<false>
// (rmav_learner.hpp) and k_trunk_grad (rmav_learner_shared.hpp).
//   expects:  A (act, act_pitch, logp_old, adv, adv_norm, clip), S (logstd, out rows 0 .. na-1), na, s, col, live, inv_b, inside
//             `if (t < 64)` and a scope of the includer's
//   defines:  nothing that outlives the includer's scope
//   modifies: S.d3 rows 0 .. na-1; the lane's accumulators sum_pg, max_ratio, gb3[c], gls[c] (a tail lane adds exact zeros)
//   barriers: none
                float ss = 0.0f, sum_ls = 0.0f, z[4], inv_std[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    z[c] = inv_std[c] = 0.0f;
                    if (c < na) {
                        inv_std[c] = expf(-S.logstd[c]);
                        z[c] = (A.act[(int64_t)c * A.act_pitch + col] - S.out[c * kLrnTile + s]) * inv_std[c];
                        ss = fmaf(z[c], z[c], ss);
                        sum_ls += S.logstd[c];
                    }
                }
                const float logp = -0.5f * ss - sum_ls - 0.5f * (float)na * kLog2Pi;
                const float ratio = expf(logp - A.logp_old[col]);
                const float a = (A.adv[col] - A.adv_norm[0]) * A.adv_norm[1];
                const float lo = 1.0f - A.clip, hi = 1.0f + A.clip;
                const float t1 = -a * ratio, t2 = -a * fminf(fmaxf(ratio, lo), hi);
                const bool inside = ratio >= lo && ratio <= hi;
                // autograd: max() hands the gradient to the larger argument and halves it on a tie; clamp's is 1 on the closed interval
                float g_ratio = 0.0f;
                if (t1 > t2 || (t1 == t2 && inside)) g_ratio = -a;
                else if (t1 == t2) g_ratio = -0.5f * a;
                const float gl = live ? g_ratio * ratio * inv_b : 0.0f;   // d loss / d logp of this sample
                if (live) {
                    sum_pg += fmaxf(t1, t2);
                    max_ratio = fmaxf(max_ratio, ratio);
                }
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c < na) {
                        const float d = gl * z[c] * inv_std[c];   // d logp / d mean_c = z_c / std_c
                        S.d3[c * kLrnTile + s] = d;
                        gb3[c] += d;
                        gls[c] = fmaf(gl, fmaf(z[c], z[c], -1.0f), gls[c]);   // d logp / d logstd_c = z_c^2 - 1
                    }

// rmav_learner_vf.inc - the value term of sample s and the delta of the value row, on wave 0: learner_net<true>
// (rmav_learner.hpp) and k_trunk_grad (rmav_learner_shared.hpp).
//   expects:  A (val_old, ret, clip, vf_coef), S.out, vrow (the value's output row: 0 in the value net, na in the trunk), s, col,
//             live, inv_b, inside `if (t < 64)` and a scope of the includer's
//   defines:  nothing that outlives the includer's scope
//   modifies: S.d3 row vrow; the lane's accumulators sum_vf and gbv (the value bias; a tail lane adds exact zeros)
//   barriers: none
                const float v = S.out[vrow * kLrnTile + s], vo = A.val_old[col], rt = A.ret[col];
                const float dv = v - vo;
                const float vc = vo + fminf(fmaxf(dv, -A.clip), A.clip);
                const float u1 = v - rt, u2 = vc - rt;
                const float e1 = u1 * u1, e2 = u2 * u2;
                const bool inside = dv >= -A.clip && dv <= A.clip;
                float gv;   // d max(e1, e2) / d v
                if (e1 > e2) gv = 2.0f * u1;
                else if (e1 < e2) gv = inside ? 2.0f * u2 : 0.0f;
                else gv = u1 + (inside ? u2 : 0.0f);
                const float d = live ? A.vf_coef * 0.5f * gv * inv_b : 0.0f;
                if (live) sum_vf += fmaxf(e1, e2);
                S.d3[vrow * kLrnTile + s] = d;
                gbv += d;

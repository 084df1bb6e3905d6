// rmav_learner_stage.inc - the staging of the two hidden layers' weights, the first statements of learner_net (rmav_learner.hpp) and
// k_trunk_grad (rmav_learner_shared.hpp).  The head (W3, the biases, logstd, the zeroed d3) differs and stays with the includer.
//   expects:  S (the kernel's Lds), t, ns, and p = the parameter pointers with p[0] = W1 [64][ns] and p[2] = W2 [64][64]
//   defines:  nothing
//   modifies: S.w2t, S.w2n, S.w1t (rows >= ns zero), columns in pos() order
//   barriers: none; the includer's barrier behind its head staging covers these stores
    for (int e = t; e < 64 * 64; e += kLrnThreads) {
        const int j = e >> 6, i = e & 63;   // W2[j][i]
        const float w = p[2][e];
        S.w2t[i * 64 + lrn_pos(j)] = w;
        S.w2n[j * 64 + lrn_pos(i)] = w;
    }
    for (int e = t; e < 16 * 64; e += kLrnThreads) {
        const int i = e >> 6, j = e & 63;   // W1[j][i]
        S.w1t[i * 64 + lrn_pos(j)] = i < ns ? p[0][j * ns + i] : 0.0f;
    }

// TEST-ONLY: the termination rule (csrc/rmav_term.hpp: term_rule<K>, term_tilt), compiled for the host, as a stand-alone program for
// tests/test_termination_host.py.  It runs no kernel and needs no GPU.
//
//   term_host < cases > results
//
// One case per input line, every number but the kind in hexadecimal (fp32 bit patterns):
//   K lo0 lo1 lo2 hi0 hi1 hi2 max_tilt s_0 .. s_{nS-1}     K = 0 .. 3 (quad2d, quad2d_sl, quad3d, quad3d_sl)
//       -> the decision term_rule<K>(s, t), 0 or 1, and the fp32 bits of the seventh threshold term_tilt(K, max_tilt)
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include <hip/hip_runtime.h>

#include "../../reinmav-gym_amd/csrc/rmav_term.hpp"

static uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
static float from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static bool word(float &f) {
    uint32_t u;
    if (scanf("%" SCNx32, &u) != 1) return false;
    f = from_bits(u);
    return true;
}

template <int K> static int one(const rmav::TermArgs &t) {
    float s[rmav::TermDims<K>::NS];
    for (float &x : s)
        if (!word(x)) return 2;
    printf("%d %08x\n", rmav::term_rule<K>(s, t) ? 1 : 0, bits(t.tilt()));
    return 0;
}

int main() {
    int k;
    while (scanf("%d", &k) == 1) {
        rmav::TermArgs t{};
        float mt;
        for (int i = 0; i < 6; ++i)
            if (!word(t.v[i])) return 2;
        if (!word(mt)) return 2;
        t.v[6] = rmav::term_tilt(k, mt);
        int rc = 2;
        switch (k) {
        case 0: rc = one<0>(t); break;
        case 1: rc = one<1>(t); break;
        case 2: rc = one<2>(t); break;
        case 3: rc = one<3>(t); break;
        }
        if (rc) return rc;
    }
    return 0;
}

// TEST-ONLY: the map statement of the start-state ranges and the host's derivation of its coefficients (csrc/rmav_start.hpp: start_map,
// start_coeffs), compiled for the host, as a stand-alone program for tests/test_start_state_host.py.  It runs no kernel and needs no GPU.
//
//   start_host < cases > results
//
// One case per input line, every number in hexadecimal (fp32 bit patterns):
//   f h m v        -> the fp32 bits of s = fma(h, v, m) (start_map)
//   d lo hi        -> the fp32 bits of h and m for the range [lo, hi] (start_coeffs)
//   i h m          -> over ALL 2^24 values the reset stream can give, v = fma(2^-23, x, -1) for x = 0 .. 2^24 - 1: the number of v whose
//                     map fma(h, v, m) does not have the bits of v (h = 1, m = 0: the identity), then the bits of the smallest and the largest v
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>

#include <hip/hip_runtime.h>

#include "../../reinmav-gym_amd/csrc/rmav_start.hpp"

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

int main() {
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'f') {
            uint32_t h, m, v;
            if (scanf("%" SCNx32 " %" SCNx32 " %" SCNx32, &h, &m, &v) != 3) return 2;
            printf("%08x\n", bits(rmav::start_map(from_bits(h), from_bits(v), from_bits(m))));
        } else if (what == 'd') {
            uint32_t lo, hi;
            if (scanf("%" SCNx32 " %" SCNx32, &lo, &hi) != 2) return 2;
            float h, m;
            rmav::start_coeffs(from_bits(lo), from_bits(hi), h, m);
            printf("%08x %08x\n", bits(h), bits(m));
        } else if (what == 'i') {
            uint32_t hb, mb, bad = 0;
            if (scanf("%" SCNx32 " %" SCNx32, &hb, &mb) != 2) return 2;
            const float h = from_bits(hb), m = from_bits(mb);
            float vmin = 2.0f, vmax = -2.0f;
            for (uint32_t x = 0; x < (1u << 24); ++x) {
                const float v = std::fmaf(1.0f / 8388608.0f, (float)x, -1.0f);   // reset_state's statement (csrc/rmav_math.hpp)
                if (bits(rmav::start_map(h, v, m)) != bits(v)) ++bad;
                vmin = v < vmin ? v : vmin;
                vmax = v > vmax ? v : vmax;
            }
            printf("%08x %08x %08x\n", bad, bits(vmin), bits(vmax));
        } else {
            return 2;
        }
    }
    return 0;
}

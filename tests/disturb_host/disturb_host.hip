// TEST-ONLY: the disturbance draw functions of the kernels (csrc/rmav_disturb.hpp: wind_draw, gust_draw, and the fp32 sum d = w + q),
// compiled for the host, as a stand-alone program for tests/test_disturbance_host.py.  It runs no kernel and needs no GPU.
//
//   disturb_host < cases > results
//
// One case per input line, every number in hexadecimal:
//   seed env_id reset_idx t  lo0 lo1 lo2  hi0 hi1 hi2  g0 g1 g2  hold        (seed, env_id, t: 64 bits; the floats: their fp32 bits)
// One result line per case: the fp32 bits of w0 w1 w2 q0 q1 q2 d0 d1 d2.  The span hi - lo and the gust block t / hold are computed here
// as the library's host side computes them (rmav_handle.hpp: disturb_args).
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../reinmav-gym_amd/csrc/rmav_disturb.hpp"

static float f32(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

int main() {
    uint64_t seed, env, t;
    uint32_t rc, v[9], hold;
    while (scanf("%" SCNx64 " %" SCNx64 " %" SCNx32 " %" SCNx64, &seed, &env, &rc, &t) == 4) {
        for (int i = 0; i < 9; ++i)
            if (scanf("%" SCNx32, &v[i]) != 1) return 2;
        if (scanf("%" SCNx32, &hold) != 1 || hold == 0) return 2;
        rmav::DisturbSpec ds{};
        for (int i = 0; i < 3; ++i) {
            ds.lo[i] = f32(v[i]);
            ds.span[i] = f32(v[3 + i]) - f32(v[i]);
            ds.gust[i] = f32(v[6 + i]);
        }
        ds.hold = (int32_t)hold;
        float w[3], q[3];
        rmav::wind_draw(ds, seed, env, rc, w);
        rmav::gust_draw(ds, seed, env, t / (uint64_t)hold, q);
        for (int i = 0; i < 3; ++i) printf("%08x ", bits(w[i]));
        for (int i = 0; i < 3; ++i) printf("%08x ", bits(q[i]));
        for (int i = 0; i < 3; ++i) {
            const float d = w[i] + q[i];
            printf("%08x%c", bits(d), i == 2 ? '\n' : ' ');
        }
    }
    return 0;
}

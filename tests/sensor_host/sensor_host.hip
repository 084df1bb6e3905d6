// TEST-ONLY: the counter / words part of the sensor-noise draw of the kernels (csrc/rmav_sensor.hpp: sensor_words, sensor_uniforms),
// compiled for the host, as a stand-alone program for tests/test_sensor_noise_host.py.  It runs no kernel and needs no GPU.
//
//   sensor_host < cases > results
//
// One case per input line, every number in hexadecimal:
//   c seed env_id b j          -> the four Philox words of block (b, j), then the fp32 bits of u1_0 u2_0 u1_1 u2_1
//   w r0 r1 r2 r3              -> the fp32 bits of u1_0 u2_0 u1_1 u2_1 of these four words (the ends of the 24-bit uniforms)
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../reinmav-gym_amd/csrc/rmav_sensor.hpp"

static uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

static void print_uniforms(const uint32_t (&r)[4]) {
    for (int p = 0; p < 2; ++p) {
        float u1, u2;
        rmav::sensor_uniforms(r, p, u1, u2);
        printf("%08x %08x%c", bits(u1), bits(u2), p == 1 ? '\n' : ' ');
    }
}

int main() {
    char what;
    while (scanf(" %c", &what) == 1) {
        uint32_t r[4];
        if (what == 'c') {
            uint64_t seed, env, b;
            uint32_t j;
            if (scanf("%" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx32, &seed, &env, &b, &j) != 4) return 2;
            rmav::sensor_words(seed, env, b, j, r);
            printf("%08x %08x %08x %08x ", r[0], r[1], r[2], r[3]);
        } else if (what == 'w') {
            if (scanf("%" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32, &r[0], &r[1], &r[2], &r[3]) != 4) return 2;
        } else {
            return 2;
        }
        print_uniforms(r);
    }
    return 0;
}

// TEST-ONLY: the filter statement of the actuator lag and the host's derivation of its coefficients (csrc/rmav_actuator.hpp: actuator_filter,
// actuator_step, actuator_coeffs), compiled for the host, as a stand-alone program for tests/test_actuator_host.py.  It runs no kernel and
// needs no GPU.
//
//   actuator_host < cases > results
//
// One case per input line, every number in hexadecimal:
//   f alpha beta m u           -> the fp32 bits of m' = fma(alpha, u, beta * m) (fp32 bit patterns in, actuator_filter)
//   v alpha beta m u           -> the same through actuator_step<4>, the case in component 2 of a lane
//   d tau dt                   -> the fp32 bits of alpha and beta for the fp32 bit pattern tau and the fp64 bit pattern dt (actuator_coeffs)
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include <hip/hip_runtime.h>

#include "../../reinmav-gym_amd/csrc/rmav_actuator.hpp"

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
        if (what == 'f' || what == 'v') {
            uint32_t a, b, m, u;
            if (scanf("%" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32, &a, &b, &m, &u) != 4) return 2;
            if (what == 'f') {
                printf("%08x\n", bits(rmav::actuator_filter(from_bits(a), from_bits(b), from_bits(m), from_bits(u))));
            } else {
                rmav::ActuatorCoef c{};
                float mm[4] = {1.0f, 2.0f, from_bits(m), 3.0f}, uu[4] = {0.5f, 0.25f, from_bits(u), 0.125f};
                for (int i = 0; i < 4; ++i) c.alpha[i] = 0.5f, c.beta[i] = 0.5f;
                c.alpha[2] = from_bits(a);
                c.beta[2] = from_bits(b);
                rmav::actuator_step<4>(c, mm, uu);
                printf("%08x\n", bits(mm[2]));
            }
        } else if (what == 'd') {
            uint32_t t;
            uint64_t d;
            if (scanf("%" SCNx32 " %" SCNx64, &t, &d) != 2) return 2;
            double dt;
            memcpy(&dt, &d, 8);
            float alpha, beta;
            rmav::actuator_coeffs((double)from_bits(t), dt, alpha, beta);
            printf("%08x %08x\n", bits(alpha), bits(beta));
        } else {
            return 2;
        }
    }
    return 0;
}

// rmav_pack_policy.hpp - policy weights -> the buffer rmav_rollout_policy reads (rmav_pack_policy / _f16; rmav_ppo_abi.hip only:
// the kernels here and in the headers beside it are ordinary external definitions, one translation unit each).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace rmav {

// out word i = flat[lo[i]]  (hi[i] < 0), or the bf16 pair (flat[lo[i]], flat[hi[i]]) in one word (low half first), where `flat`
// is the concatenation of the caller's parameter tensors (<= kPackMaxParams of them) followed by zeros.  The layouts of
// include/rmav.h are fixed permutations + zero padding (+ bf16 rounding) of the parameters, so one gather launch replaces
// the ~8 dependent torch launches (cat, index, convert, cat, copy: ~35 us) a repack used to cost before every rollout.
constexpr int kPackMaxParams = 16;
struct PackSrc {
    const float *p[kPackMaxParams];
    int32_t end[kPackMaxParams];   // exclusive prefix ends of the parameters inside `flat`
    int32_t n;
};
__device__ __forceinline__ float pack_fetch(const PackSrc &src, int32_t j) {
    int32_t begin = 0;
#pragma unroll
    for (int k = 0; k < kPackMaxParams; ++k) {
        if (k < src.n && j >= begin && j < src.end[k]) return src.p[k][j - begin];
        if (k < src.n) begin = src.end[k];
    }
    return 0.0f;   // the appended zero (padding)
}
// F16: the pair words are f16 (round to nearest even) and word i of the MfmaLayout buffer is pre-scaled by `scale2` inside
// the layer-2 fragments, by `scale3` inside the layer-3 fragments (rmav_pack_policy_f16: tanh folded into the next layer).
template <bool F16>
__global__ __launch_bounds__(256) void k_pack_policy(const PackSrc src, const int32_t *__restrict__ lo, const int32_t *__restrict__ hi,
                                                     int64_t n_out, float *__restrict__ out, int32_t net_words, int32_t a2_begin,
                                                     int32_t a3_begin, int32_t a3_end, float scale2, float scale3) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_out) return;
    const float a = pack_fetch(src, lo[i]);
    const int32_t h = hi[i];
    if (h < 0) {
        out[i] = a;
    } else {
        typedef __attribute__((ext_vector_type(2))) float f32x2_t;
        f32x2_t v = {a, pack_fetch(src, h)};
        if constexpr (F16) {
            typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;
            const int32_t o = (int32_t)(i % net_words);
            const float sc = (i < 2 * (int64_t)net_words && o >= a2_begin && o < a3_end) ? (o < a3_begin ? scale2 : scale3) : 1.0f;
            v = v * sc;
            out[i] = __builtin_bit_cast(float, __builtin_convertvector(v, f16x2_t));
        } else {
            typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
            out[i] = __builtin_bit_cast(float, __builtin_convertvector(v, bf16x2_t));   // round to nearest even, as torch's .to(bfloat16)
        }
    }
}

}  // namespace rmav

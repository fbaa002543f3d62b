// quant.h -- element decoders and the accumulation step of quantized rows (bf16 bits, the reference's FP8 E4M3 codes,
// int8 with one inv_multiplier): shared by the brute-force kernels (bf.hip: bf_quant_kernel, the quantized shortlist
// pass) and the tree / hasher re-rank over quantized rows (txh_rows.hip: rerank_quant_kernel).  Device code only.
#pragma once
#include "common.h"

namespace scann {

typedef float f32x2q __attribute__((ext_vector_type(2)));

template <int FMT>
__host__ __device__ constexpr uint32_t quant_bytes() { return FMT == SCANN_HIP_ROWS_BF16 ? 2u : 1u; }

// fp8_to_f32(b, 0) of txh_rows.hip without branches: exponent field e and mantissa m as one 7-bit field em shifted
// into place, biased by 120 = 127 - 7, one binade lower when e == 0 (2^-8 * (1 + m/8)), zero when em == 0.
// The branchy form makes the compiler decode a whole 64-element block into registers before using it.
__device__ __forceinline__ float fp8_e4m3_to_f32(uint32_t b) {
    const uint32_t em = b & 0x7Fu;
    const uint32_t mag = em ? (em << 20) + (em < 8u ? 119u << 23 : 120u << 23) : 0u;
    return __uint_as_float(((b & 0x80u) << 24) | mag);
}

// element `sub` of a 32-bit word of packed row elements
template <int FMT>
__device__ __forceinline__ float quant_decode(uint32_t w, int sub, float inv) {
    if (FMT == SCANN_HIP_ROWS_BF16) return __uint_as_float(sub ? (w & 0xFFFF0000u) : (w << 16));
    const uint32_t b = (w >> (8 * sub)) & 0xFFu;
    if (FMT == SCANN_HIP_ROWS_FP8_E4M3) return fp8_e4m3_to_f32(b);
    return (float)(int)(int8_t)b * inv;
}

template <int FMT>
__device__ __forceinline__ float quant_load1(const uint8_t *row, uint32_t e, float inv) {
    if (FMT == SCANN_HIP_ROWS_BF16)
        return __uint_as_float((uint32_t)reinterpret_cast<const uint16_t *>(row)[e] << 16);
    if (FMT == SCANN_HIP_ROWS_FP8_E4M3) return fp8_e4m3_to_f32(row[e]);
    return (float)(int)(int8_t)row[e] * inv;
}

// one element into an accumulator: INT8 chains fuse (_mm256_fmadd_ps), everything else is add(mul)
template <int MEASURE, bool FUSED>
__device__ __forceinline__ void quant_step(f32x2q &acc, f32x2q q, float x) {
    const f32x2q xv = f32x2q{x, x};
    if (MEASURE == SCANN_HIP_DOT_PRODUCT) {
        if (FUSED) acc = __builtin_elementwise_fma(q, xv, acc);
        else acc = acc + q * xv;
    } else {
        const f32x2q d = q - xv;
        if (FUSED) acc = __builtin_elementwise_fma(d, d, acc);
        else acc = acc + d * d;
    }
}

}  // namespace scann

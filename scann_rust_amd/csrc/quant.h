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

// ---- encoders (the quantize entry points of bf.hip / txh_rows.hip and the row passes of scalarq.hip) ----
// half::bf16::from_f32 (quantization/bfloat16.rs:13-30): NaN keeps its top bits with the quiet bit set;
// otherwise round to nearest even on bit 15 (inf stays inf, the largest finite values round up to inf).
__device__ __forceinline__ uint32_t bf16_from_f32(float value) {
    const uint32_t x = __float_as_uint(value);
    if ((x & 0x7FFFFFFFu) > 0x7F800000u) return ((x >> 16) | 0x40u) & 0xFFFFu;
    return ((x >> 16) + (((x & 0x8000u) && (x & 0x17FFFu)) ? 1u : 0u)) & 0xFFFFu;
}

// The reference's FP8 encoder (quantization/fp8.rs:80-140), bit for bit.
// format 0 = E4M3 (bias 7, 3 mantissa bits, max code 0x7E), 1 = E5M2 (bias 15, 2 bits, max code 0x7C).
// NOT the hardware conversion: the mantissa carry wraps without bumping the exponent, the top exponent
// field only ever encodes the maximum, values under the smallest normal flush to (signed) zero.
__device__ __forceinline__ uint32_t fp8_from_f32(float value, int format) {
    const int mbits = format ? 2 : 3, bias = format ? 15 : 7, emax = format ? 31 : 15;
    const uint32_t maxcode = format ? 0x7Cu : 0x7Eu;
    if (value == 0.0f) return 0u;
    const uint32_t bits = __float_as_uint(value);
    const uint32_t sign = bits >> 31;
    const int exp = (int)((bits >> 23) & 0xFFu);
    const uint32_t mantissa = bits & 0x7FFFFFu;
    if (exp == 0xFF) return (sign << 7) | maxcode;
    const int e8 = exp - 127 + bias;
    if (e8 <= 0) return sign << 7;
    if (e8 >= emax) return (sign << 7) | maxcode;
    const uint32_t m = ((mantissa >> (23 - mbits)) + ((mantissa >> (22 - mbits)) & 1u)) & ((1u << mbits) - 1u);
    return (sign << 7) | ((uint32_t)e8 << mbits) | m;
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

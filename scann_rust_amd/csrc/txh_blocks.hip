// txh_blocks.hip -- building blocks of the AsymmetricHasher path exposed through the C ABI: explicit-table ADC
// distances, the LUT16 u8 batch and its table quantiser, the encoder.  No search calls them.
#include "launch.h"
#include "txh.h"

namespace scann {

// All-pairs ADC distances for explicit f32 LUTs [nq][S][K]: out [nq][n_local].
// hashes/lut.rs:74-82: sum = 0.0; for s ascending: sum += lut[s][code[s]].
__global__ __launch_bounds__(256) void adc_distances_kernel(TxhIndexDev ix,
                                                            const float *__restrict__ luts,
                                                            float *__restrict__ out) {
    extern __shared__ float slut[];   // [S][K]
    const uint32_t q = blockIdx.y, S = ix.S, K = ix.K, nw = ix.nw;
    const uint32_t bits = ix.code_bits, per = 32u / bits, mask = (1u << bits) - 1u;
    for (uint32_t e = threadIdx.x; e < S * K; e += blockDim.x) slut[e] = luts[(size_t)q * S * K + e];
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ix.n_local;
         i += (uint64_t)gridDim.x * blockDim.x) {
        float acc = 0.0f;
        for (uint32_t sub = 0; sub < S; ++sub) {
            const uint32_t w = ix.codes[i * nw + sub / per];
            const uint32_t code = (w >> (bits * (sub % per))) & mask;
            acc = acc + slut[sub * K + (code < K ? code : 0u)];
        }
        out[(size_t)q * ix.n_local + i] = acc;
    }
}

// Lut16SimdTables::compute_distances_batch (hashes/lut16_simd.rs:119-141 over
// simd/dispatch.rs:259-295): u32 sum of u8 table entries, then sum * mult + bias * S.
__global__ __launch_bounds__(256) void lut16_u8_batch_kernel(
    const uint8_t *__restrict__ packed, const uint8_t *__restrict__ lut8, uint32_t S,
    uint64_t n, float bias, float mult, float *__restrict__ out) {
    extern __shared__ uint8_t s_lut8[];  // [S*16]
    for (uint32_t e = threadIdx.x; e < S * 16; e += blockDim.x) s_lut8[e] = lut8[e];
    __syncthreads();
    const uint32_t bpp = (S + 1) / 2;
    const float bias_total = bias * (float)S;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint8_t *row = packed + i * bpp;
        uint32_t sum = 0, sub = 0;
        for (uint32_t b = 0; b < bpp; ++b) {
            const uint32_t byte = row[b];
            if (sub < S) { sum += s_lut8[sub * 16 + (byte & 15u)]; ++sub; }
            if (sub < S) { sum += s_lut8[sub * 16 + (byte >> 4)]; ++sub; }
        }
        const float r = (float)sum * mult;
        out[i] = r + bias_total;
    }
}

// Lut16SimdTables::from_float_tables (hashes/lut16_simd.rs:39-90): global min / max of the S x 16
// entries (f32::min / f32::max: a NaN operand is ignored), range = max - min, scale = 255 / range
// (1 when range < 1e-10), lut8 = round((v - min) * scale) as u8 (round half away from zero; `as u8`
// saturates and maps NaN to 0), bias = min, multiplier = 1 / scale (1 in the degenerate case).
__global__ __launch_bounds__(256) void lut16_quantize_kernel(const float *__restrict__ tables, uint32_t S,
                                                             uint8_t *__restrict__ lut8,
                                                             float *__restrict__ bias_mult) {
    __shared__ float s_min[4], s_max[4];
    const uint32_t tid = threadIdx.x, n = S * 16;
    float mn = 3.40282347e+38f, mx = -3.40282347e+38f;   // f32::MAX / f32::MIN
    for (uint32_t i = tid; i < n; i += 256) {
        const float v = tables[i];
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o));
        mx = fmaxf(mx, __shfl_xor(mx, o));
    }
    if ((tid & 63u) == 0) {
        s_min[tid >> 6] = mn;
        s_max[tid >> 6] = mx;
    }
    __syncthreads();
    mn = fminf(fminf(s_min[0], s_min[1]), fminf(s_min[2], s_min[3]));
    mx = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
    const float range = mx - mn;
    const bool degenerate = range < 1e-10f;
    const float scale = degenerate ? 1.0f : 255.0f / range;
    for (uint32_t i = tid; i < n; i += 256) {
        const float r = roundf((tables[i] - mn) * scale);
        lut8[i] = !(r > 0.0f) ? (uint8_t)0 : (r >= 255.0f ? (uint8_t)255 : (uint8_t)r);
    }
    if (tid == 0) {
        bias_mult[0] = mn;
        bias_mult[1] = degenerate ? 1.0f : 1.0f / scale;
    }
}

// Codebook::encode (hashes/codebook.rs:82-95): per subspace argmin over K with strict '<'.
__global__ __launch_bounds__(256) void encode_kernel(
    const float *__restrict__ codebook, uint32_t S, uint32_t K, uint32_t dsub,
    const float *__restrict__ rows, uint64_t n, uint32_t stride,
    const float *__restrict__ centers, const uint32_t *__restrict__ leaf_of_row,
    uint8_t *__restrict__ out) {
    const uint64_t total = n * S;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = e / S;
        const uint32_t s = (uint32_t)(e - i * S);
        const float *x = rows + i * stride + s * dsub;
        const float *cen = centers ? centers + (size_t)leaf_of_row[i] * (S * dsub) + s * dsub
                                   : nullptr;
        float best = __builtin_inff();
        uint32_t bi = 0;
        for (uint32_t c = 0; c < K; ++c) {
            const float *cb = codebook + ((size_t)s * K + c) * dsub;
            float d = 0.0f;
            for (uint32_t j = 0; j < dsub; ++j) {
                float xv = x[j];
                if (cen) xv = xv - cen[j];
                const float t = xv - cb[j];
                d = d + t * t;
            }
            if (d < best) {
                best = d;
                bi = c;
            }
        }
        out[e] = (uint8_t)bi;
    }
}

int txh_launch_adc_distances(const TxhIndexDev &ix, const float *d_luts, uint32_t nq, float *d_out,
                             hipStream_t st) {
    if (nq == 0 || ix.n_local == 0) return SCANN_HIP_OK;
    const uint32_t gx = (uint32_t)std::min<uint64_t>(ceil_div_u64(ix.n_local, 256), 4096);
    dim3 grid(gx, nq);
    const size_t lds = (size_t)ix.S * ix.K * sizeof(float);
    SCANN_TRY(launch(adc_distances_kernel, grid, dim3(256), lds, st, ix, d_luts, d_out));
    return SCANN_HIP_OK;
}

int launch_lut16_u8_batch(const uint8_t *d_packed, const uint8_t *d_lut8, uint32_t S, uint64_t n,
                          float bias, float mult, float *d_out, hipStream_t st) {
    if (n == 0) return SCANN_HIP_OK;
    const uint32_t gx = (uint32_t)std::min<uint64_t>(ceil_div_u64(n, 256), 8192);
    SCANN_TRY(launch(lut16_u8_batch_kernel, dim3(gx), dim3(256), (size_t)S * 16, st, d_packed, d_lut8,
                     S, n, bias, mult, d_out));
    return SCANN_HIP_OK;
}

int launch_lut16_quantize(const float *d_tables, uint32_t S, uint8_t *d_lut8, float *d_bias_mult,
                          hipStream_t st) {
    if (S == 0) return SCANN_HIP_OK;
    SCANN_TRY(launch(lut16_quantize_kernel, dim3(1), dim3(256), 0, st, d_tables, S, d_lut8, d_bias_mult));
    return SCANN_HIP_OK;
}

int launch_encode(const float *d_codebook, uint32_t S, uint32_t K, uint32_t dsub, const float *d_rows,
                  uint64_t n, uint32_t stride, const float *d_centers, const uint32_t *d_leaf_of_row,
                  uint8_t *d_out, hipStream_t st) {
    if (n == 0) return SCANN_HIP_OK;
    const uint32_t gx = (uint32_t)std::min<uint64_t>(ceil_div_u64(n * S, 256), 16384);
    SCANN_TRY(launch(encode_kernel, dim3(gx), dim3(256), 0, st, d_codebook, S, K, dsub, d_rows, n,
                     stride, d_centers, d_leaf_of_row, d_out));
    return SCANN_HIP_OK;
}

}  // namespace scann

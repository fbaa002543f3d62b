// scalarq.hip -- ScalarQuantizer on the device (scalarq.h): the stats reduction, the f32 -> int8 /
// bf16 / FP8 row passes, and the stateless entry points scann_hip_scalar_quantizer_calibrate,
// scann_hip_scalar_quantize, scann_hip_scalar_dequantize, scann_hip_scalar_quantize_device.
#include "scalarq.h"

#include <algorithm>
#include <cfloat>
#include <cmath>

#include "comm.h"   // ctx_device
#include "launch.h"
#include "quant.h"

namespace scann {

// =====================================================================================
// stats: one streaming pass, f64 partials per fixed chunk, a fixed-order final reduce
// =====================================================================================
struct SqAcc {
    double s = 0.0, s2 = 0.0;
    float mn = FLT_MAX, mx = -FLT_MAX, am = 0.0f;
    uint32_t nf = 0;
    __device__ __forceinline__ void add(float v) {
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
        const float a = fabsf(v);
        am = fmaxf(am, a);
        nf |= !(a < __builtin_inff()) ? 1u : 0u;
        const double d = (double)v;
        s = s + d;
        s2 = s2 + d * d;
    }
};

// the 256 thread accumulators of a workgroup -> thread 0's, as the tree of scalarq.h
__device__ __forceinline__ void sq_block_reduce(SqAcc &a) {
    __shared__ double sh_s[kSqThreads], sh_s2[kSqThreads];
    __shared__ float sh_mn[kSqThreads], sh_mx[kSqThreads], sh_am[kSqThreads];
    __shared__ uint32_t sh_nf[kSqThreads];
    const uint32_t t = threadIdx.x;
    sh_s[t] = a.s; sh_s2[t] = a.s2; sh_mn[t] = a.mn; sh_mx[t] = a.mx; sh_am[t] = a.am; sh_nf[t] = a.nf;
    __syncthreads();
    for (uint32_t off = kSqThreads / 2; off > 0; off >>= 1) {
        if (t < off) {
            sh_s[t] = sh_s[t] + sh_s[t + off];
            sh_s2[t] = sh_s2[t] + sh_s2[t + off];
            sh_mn[t] = fminf(sh_mn[t], sh_mn[t + off]);
            sh_mx[t] = fmaxf(sh_mx[t], sh_mx[t + off]);
            sh_am[t] = fmaxf(sh_am[t], sh_am[t + off]);
            sh_nf[t] |= sh_nf[t + off];
        }
        __syncthreads();
    }
    a.s = sh_s[0]; a.s2 = sh_s2[0]; a.mn = sh_mn[0]; a.mx = sh_mx[0]; a.am = sh_am[0]; a.nf = sh_nf[0];
}

__device__ __forceinline__ void sq_store_partial(SqPartial *dst, const SqAcc &a) {
    SqPartial p;
    p.sum = a.s; p.sum_sq = a.s2; p.mn = a.mn; p.mx = a.mx; p.amax = a.am; p.nonfinite = a.nf;
    *dst = p;
}

// Workgroup c reduces the logical values [c * kSqChunk, (c + 1) * kSqChunk) of the row-major n x dim matrix stored
// at `stride`; total = n * dim.  VEC: dim % 4 == 0, stride % 4 == 0 and a 16-byte aligned base -- a group of four
// logical values is then one aligned 16-byte load that never crosses a row.  step_rows / step_cols: 1024 / dim and
// 1024 % dim, the walk from one of a thread's groups to its next.
template <bool VEC>
__global__ __launch_bounds__(kSqThreads) void sq_stats_kernel(const float *__restrict__ rows, uint64_t total, uint32_t dim,
                                                              uint32_t stride, uint32_t step_rows, uint32_t step_cols,
                                                              SqPartial *__restrict__ partials) {
    constexpr int kGroups = kSqChunk / kSqGroupStep;   // 16 groups of four per thread
    const uint64_t e0 = (uint64_t)blockIdx.x * kSqChunk + 4u * threadIdx.x;
    uint64_t row = e0 / dim;
    uint32_t col = (uint32_t)(e0 % dim);
    SqAcc a;
    if (VEC) {
        float4 v[kGroups];
#pragma unroll
        for (int j = 0; j < kGroups; ++j) {
            const uint64_t e = e0 + (uint64_t)j * kSqGroupStep;
            v[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (e < total) v[j] = *reinterpret_cast<const float4 *>(rows + row * stride + col);
            row += step_rows;
            col += step_cols;
            if (col >= dim) {
                col -= dim;
                ++row;
            }
        }
#pragma unroll
        for (int j = 0; j < kGroups; ++j) {
            if (e0 + (uint64_t)j * kSqGroupStep < total) {   // (total % 4 == 0: a group is whole or absent)
                a.add(v[j].x);
                a.add(v[j].y);
                a.add(v[j].z);
                a.add(v[j].w);
            }
        }
    } else {
        for (int j = 0; j < kGroups; ++j) {
            const uint64_t e = e0 + (uint64_t)j * kSqGroupStep;
            uint64_t r = row;
            uint32_t c = col;
            for (uint32_t i = 0; i < 4; ++i) {
                if (e + i < total) a.add(rows[r * stride + c]);
                if (++c == dim) {
                    c = 0;
                    ++r;
                }
            }
            row += step_rows;
            col += step_cols;
            if (col >= dim) {
                col -= dim;
                ++row;
            }
        }
    }
    sq_block_reduce(a);
    if (threadIdx.x == 0) sq_store_partial(partials + blockIdx.x, a);
}

// One workgroup: thread t folds the partials t, t + 256, ... in order, then the tree.
__global__ __launch_bounds__(kSqThreads) void sq_stats_final_kernel(const SqPartial *__restrict__ partials, uint32_t count,
                                                                    SqPartial *__restrict__ out) {
    SqAcc a;
    for (uint32_t c = threadIdx.x; c < count; c += kSqThreads) {
        const SqPartial p = partials[c];
        a.s = a.s + p.sum;
        a.s2 = a.s2 + p.sum_sq;
        a.mn = fminf(a.mn, p.mn);
        a.mx = fmaxf(a.mx, p.mx);
        a.am = fmaxf(a.am, p.amax);
        a.nf |= p.nonfinite;
    }
    sq_block_reduce(a);
    if (threadIdx.x == 0) sq_store_partial(out, a);
}

int sq_stats_device(const float *d_rows, uint64_t n, uint32_t dim, uint32_t stride, hipStream_t st, SqPartial *out) {
    if (!d_rows || !out || n == 0 || dim == 0 || stride < dim) return fail(SCANN_HIP_INVALID_ARGUMENT, "stats: bad rows");
    const uint64_t total = n * dim;
    const uint64_t chunks = ceil_div_u64(total, kSqChunk);
    if (chunks > 0x7FFFFFFFull) return fail(SCANN_HIP_OUT_OF_RANGE, "stats: more than 2^31 - 1 chunks");
    DevBuf partials, result;
    SCANN_TRY(partials.ensure((size_t)chunks * sizeof(SqPartial)));
    SCANN_TRY(result.ensure(sizeof(SqPartial)));
    const bool vec = (dim & 3u) == 0 && (stride & 3u) == 0 && (reinterpret_cast<uintptr_t>(d_rows) & 15u) == 0;
    const uint32_t step_rows = kSqGroupStep / dim, step_cols = kSqGroupStep % dim;
    if (vec)
        SCANN_TRY(launch(sq_stats_kernel<true>, dim3((uint32_t)chunks), dim3(kSqThreads), 0, st, d_rows, total, dim, stride,
                         step_rows, step_cols, partials.as<SqPartial>()));
    else
        SCANN_TRY(launch(sq_stats_kernel<false>, dim3((uint32_t)chunks), dim3(kSqThreads), 0, st, d_rows, total, dim, stride,
                         step_rows, step_cols, partials.as<SqPartial>()));
    SCANN_TRY(launch(sq_stats_final_kernel, dim3(1), dim3(kSqThreads), 0, st, partials.as<SqPartial>(), (uint32_t)chunks,
                     result.as<SqPartial>()));
    SCANN_HIP_CHECK(hipMemcpyAsync(out, result.p, sizeof(SqPartial), hipMemcpyDeviceToHost, st));
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    return SCANN_HIP_OK;
}

void sq_stats_finish(const SqPartial &r, uint64_t count, float *out4) {
    const double cnt = (double)count;
    const float mean = count > 0 ? (float)(r.sum / cnt) : 0.0f;
    float variance = 0.0f;
    if (count > 1) {
        const double sq = r.sum * r.sum;
        variance = (float)((r.sum_sq - sq / cnt) / (double)(count - 1));
    }
    out4[0] = r.mn;
    out4[1] = r.mx;
    out4[2] = mean;
    out4[3] = sqrtf(variance);
}

// =====================================================================================
// calibrate (scalar.rs:103-130) and the project's signed mode
// =====================================================================================
static int sq_levels(uint32_t bits, int mode, int32_t *levels) {
    if (mode < SCANN_HIP_SQ_STDDEV || mode > SCANN_HIP_SQ_SIGNED)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "scalar quantizer: unknown mode " + std::to_string(mode));
    if (mode == SCANN_HIP_SQ_SIGNED ? bits != 8 : (bits != 4 && bits != 8))
        return fail(SCANN_HIP_INVALID_ARGUMENT, "scalar quantizer: bits must be 4 or 8 (8 in the signed mode)");
    *levels = mode == SCANN_HIP_SQ_SIGNED ? 127 : (1 << bits) - 1;
    return SCANN_HIP_OK;
}

int sq_calibrate(const float *stats4, uint32_t bits, int mode, float a, float b, SqParams *out, int32_t *zero_point) {
    SqParams p{};
    SCANN_TRY(sq_levels(bits, mode, &p.levels));
    const float smin = stats4[0], smax = stats4[1], mean = stats4[2], std_dev = stats4[3];
    if (mode == SCANN_HIP_SQ_SIGNED) {
        if (!std::isfinite(smin) || !std::isfinite(smax) || !std::isfinite(mean))
            return fail(SCANN_HIP_INVALID_ARGUMENT, "scalar quantizer: the signed mode needs finite values");
        const float m = fmaxf(fabsf(smin), fabsf(smax));
        const float s = m > 0.0f ? (float)((double)m / 127.0) : 1.0f;
        p.mn = -m;
        p.mx = m;
        p.scale = s;
        p.inv_scale = 1.0f / s;
        *out = p;
        *zero_point = 0;
        return SCANN_HIP_OK;
    }
    if (mode == SCANN_HIP_SQ_RANGE) {
        p.mn = a;
        p.mx = b;
    } else if (mode == SCANN_HIP_SQ_SYMMETRIC) {
        const float abs_max = fmaxf(fabsf(smin), fabsf(smax));
        p.mn = -abs_max;
        p.mx = abs_max;
    } else {
        const float r = a * std_dev;
        const float lo = mean - r, hi = mean + r;
        p.mn = fmaxf(lo, smin);
        p.mx = fminf(hi, smax);
    }
    if (!(p.mn <= p.mx))   // f32::clamp panics on min > max or a NaN bound
        return fail(SCANN_HIP_INVALID_ARGUMENT, "scalar quantizer: the range is empty or not a number");
    const float range = p.mx - p.mn;
    int32_t zp = 0;
    if (range > 1e-10f) {
        const float levels = (float)p.levels;
        p.scale = range / levels;
        p.inv_scale = levels / range;
        const float z = -p.mn * p.inv_scale;
        zp = sq_f32_as_i32(roundf(z));
    } else {
        p.scale = 1.0f;
        p.inv_scale = 1.0f;
    }
    *out = p;
    *zero_point = zp;
    return SCANN_HIP_OK;
}

int sq_params_checked(uint32_t bits, int mode, const float *params4, SqParams *out) {
    SqParams p{};
    SCANN_TRY(sq_levels(bits, mode, &p.levels));
    if (!params4) return fail(SCANN_HIP_INVALID_ARGUMENT, "scalar quantizer: params is null");
    p.mn = params4[0];
    p.mx = params4[1];
    p.scale = params4[2];
    p.inv_scale = params4[3];
    if (mode == SCANN_HIP_SQ_SIGNED) {
        if (!(p.scale > 0.0f) || !std::isfinite(p.scale))
            return fail(SCANN_HIP_INVALID_ARGUMENT, "scalar quantizer: the signed mode needs a finite scale > 0");
    } else if (!(p.mn <= p.mx) || p.inv_scale != p.inv_scale) {
        return fail(SCANN_HIP_INVALID_ARGUMENT, "scalar quantizer: the range is empty or not a number");
    }
    *out = p;
    return SCANN_HIP_OK;
}

// =====================================================================================
// row passes: f32 rows -> int8 (reference modes / signed), bf16, FP8 E4M3
// =====================================================================================
enum { kSqKindRef = 0, kSqKindSigned = 1, kSqKindBf16 = 2, kSqKindFp8 = 3 };

template <int KIND>
__device__ __forceinline__ uint32_t sq_encode(float v, const SqParams &p) {
    if (KIND == kSqKindRef) return (uint8_t)sq_ref_code(v, p);
    if (KIND == kSqKindSigned) return (uint8_t)sq_signed_code(v, p.scale);
    if (KIND == kSqKindBf16) return bf16_from_f32(v);
    return fp8_from_f32(v, 0) & 0xFFu;
}

// The output is walked as one flat array of n * out_stride elements in units of 16 bytes (16 codes, or 8 bf16
// values); a thread encodes one unit in registers and writes it with one 16-byte store.  Element f is column
// f % out_stride of row f / out_stride: a code where the column is below dim, 0 in the pad columns.  FAST: out_stride
// is a multiple of the unit and the source qualifies for 16-byte loads (dim % 4, stride % 4, aligned base), so a unit
// lies in one row and reads whole float4 groups.  The last unit may be partial and an unaligned output has no 16-byte
// stores: both write element by element, never past element `total`.
template <int KIND, bool FAST>
__global__ __launch_bounds__(256) void sq_quantize_kernel(const float *__restrict__ rows, uint32_t dim, uint32_t stride,
                                                          SqParams p, void *__restrict__ out, uint32_t out_stride,
                                                          uint64_t total, int wide_stores) {
    constexpr uint32_t kEsz = KIND == kSqKindBf16 ? 2u : 1u;
    constexpr uint32_t kUnit = 16u / kEsz;        // elements per 16-byte unit
    constexpr uint32_t kPerWord = 4u / kEsz;
    const uint64_t units = (total + kUnit - 1) / kUnit;
    for (uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x; u < units; u += (uint64_t)gridDim.x * 256) {
        const uint64_t first = u * kUnit;
        uint64_t row = first / out_stride;
        uint32_t col = (uint32_t)(first % out_stride);
        const uint32_t live = (uint32_t)std::min<uint64_t>(kUnit, total - first);
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (FAST) {
            const float *src = rows + row * stride;
#pragma unroll
            for (uint32_t g = 0; g < kUnit / 4; ++g) {
                const uint32_t c = col + 4 * g;
                if (c < dim) {   // (dim % 4 == 0: the four columns are all data or all pad)
                    const float4 v = *reinterpret_cast<const float4 *>(src + c);
                    const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (uint32_t i = 0; i < 4; ++i) {
                        const uint32_t e = 4 * g + i;
                        w[e / kPerWord] |= sq_encode<KIND>(x[i], p) << (8 * kEsz * (e % kPerWord));
                    }
                }
            }
        } else {
#pragma unroll
            for (uint32_t e = 0; e < kUnit; ++e) {
                if (e < live) {
                    if (col < dim) w[e / kPerWord] |= sq_encode<KIND>(rows[row * stride + col], p) << (8 * kEsz * (e % kPerWord));
                    if (++col == out_stride) {
                        col = 0;
                        ++row;
                    }
                }
            }
        }
        if (wide_stores && live == kUnit) {
            reinterpret_cast<uint4 *>(out)[u] = make_uint4(w[0], w[1], w[2], w[3]);
        } else if (kEsz == 2) {
            uint16_t *o = reinterpret_cast<uint16_t *>(out) + first;
            for (uint32_t e = 0; e < live; ++e) o[e] = (uint16_t)(w[e / kPerWord] >> (16 * (e % kPerWord)));
        } else {
            uint8_t *o = reinterpret_cast<uint8_t *>(out) + first;
            for (uint32_t e = 0; e < live; ++e) o[e] = (uint8_t)(w[e / kPerWord] >> (8 * (e % kPerWord)));
        }
    }
}

template <int KIND>
static int launch_sq_kind(const float *d_rows, uint64_t n, uint32_t dim, uint32_t stride, const SqParams &p, void *d_out,
                          uint32_t out_stride, hipStream_t st) {
    constexpr uint32_t kUnit = KIND == kSqKindBf16 ? 8u : 16u;
    const uint64_t total = n * out_stride;
    const uint64_t units = ceil_div_u64(total, kUnit);
    const bool fast = out_stride % kUnit == 0 && (dim & 3u) == 0 && (stride & 3u) == 0 &&
                      (reinterpret_cast<uintptr_t>(d_rows) & 15u) == 0;
    const int wide = (reinterpret_cast<uintptr_t>(d_out) & 15u) == 0 ? 1 : 0;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(ceil_div_u64(units, 256), (uint64_t)num_cus() * 8);
    if (fast)
        return launch((sq_quantize_kernel<KIND, true>), dim3(grid), dim3(256), 0, st, d_rows, dim, stride, p, d_out,
                      out_stride, total, wide);
    return launch((sq_quantize_kernel<KIND, false>), dim3(grid), dim3(256), 0, st, d_rows, dim, stride, p, d_out, out_stride,
                  total, wide);
}

int launch_sq_quantize(const float *d_rows, uint64_t n, uint32_t dim, uint32_t stride, int fmt, int mode, const SqParams &p,
                       void *d_out, uint32_t out_stride, hipStream_t st) {
    if (n == 0) return SCANN_HIP_OK;
    if (!d_rows || !d_out || dim == 0 || stride < dim || out_stride < dim)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "quantize rows: null rows/output or a stride below dim");
    if (fmt == SCANN_HIP_ROWS_BF16) return launch_sq_kind<kSqKindBf16>(d_rows, n, dim, stride, p, d_out, out_stride, st);
    if (fmt == SCANN_HIP_ROWS_FP8_E4M3) return launch_sq_kind<kSqKindFp8>(d_rows, n, dim, stride, p, d_out, out_stride, st);
    if (fmt != SCANN_HIP_ROWS_INT8) return fail(SCANN_HIP_INVALID_ARGUMENT, "unknown row format " + std::to_string(fmt));
    if (mode == SCANN_HIP_SQ_SIGNED) return launch_sq_kind<kSqKindSigned>(d_rows, n, dim, stride, p, d_out, out_stride, st);
    return launch_sq_kind<kSqKindRef>(d_rows, n, dim, stride, p, d_out, out_stride, st);
}

}  // namespace scann

// =====================================================================================
// C ABI: the stateless entry points (the index entry points are in api.hip)
// =====================================================================================
using namespace scann;

extern "C" {

int scann_hip_scalar_quantizer_calibrate(const float *stats4, uint32_t bits, int mode, float a, float b, float *out_params4,
                                         int32_t *out_zero_point) {
    if (!stats4 || !out_params4 || !out_zero_point) return fail(SCANN_HIP_INVALID_ARGUMENT, "null stats/output");
    SqParams p{};
    int32_t zp = 0;
    SCANN_TRY(sq_calibrate(stats4, bits, mode, a, b, &p, &zp));
    out_params4[0] = p.mn;
    out_params4[1] = p.mx;
    out_params4[2] = p.scale;
    out_params4[3] = p.inv_scale;
    *out_zero_point = zp;
    return SCANN_HIP_OK;
}

int scann_hip_scalar_quantize(const float *values, uint64_t n, uint32_t bits, int mode, const float *params4, int8_t *out) {
    SqParams p{};
    SCANN_TRY(sq_params_checked(bits, mode, params4, &p));
    if (n == 0) return SCANN_HIP_OK;
    if (!values || !out) return fail(SCANN_HIP_INVALID_ARGUMENT, "null values/output");
    if (mode == SCANN_HIP_SQ_SIGNED) {
        for (uint64_t i = 0; i < n; ++i)
            if (!std::isfinite(values[i]))
                return fail(SCANN_HIP_INVALID_ARGUMENT, "scalar quantizer: the signed mode needs finite values");
        for (uint64_t i = 0; i < n; ++i) out[i] = sq_signed_code(values[i], p.scale);
    } else {
        for (uint64_t i = 0; i < n; ++i) out[i] = sq_ref_code(values[i], p);
    }
    return SCANN_HIP_OK;
}

int scann_hip_scalar_dequantize(const int8_t *codes, uint64_t n, int mode, const float *params4, float *out) {
    if (mode < SCANN_HIP_SQ_STDDEV || mode > SCANN_HIP_SQ_SIGNED)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "scalar quantizer: unknown mode " + std::to_string(mode));
    if (!params4) return fail(SCANN_HIP_INVALID_ARGUMENT, "scalar quantizer: params is null");
    if (n == 0) return SCANN_HIP_OK;
    if (!codes || !out) return fail(SCANN_HIP_INVALID_ARGUMENT, "null codes/output");
    const float mn = params4[0], scale = params4[2];
    for (uint64_t i = 0; i < n; ++i) {
        if (mode == SCANN_HIP_SQ_SIGNED) {
            out[i] = (float)codes[i] * scale;   // what the searchers read
        } else {
            const float t = (float)(uint8_t)codes[i] * scale;   // scalar.rs:168-172
            out[i] = t + mn;
        }
    }
    return SCANN_HIP_OK;
}

int scann_hip_scalar_quantize_device(scann_hip_ctx *ctx, const float *d_rows, uint64_t n, uint32_t dim, uint32_t stride,
                                     uint32_t bits, int mode, const float *params4, int8_t *d_out, uint32_t out_stride,
                                     void *hip_stream) {
    if (!ctx) return fail(SCANN_HIP_INVALID_ARGUMENT, "ctx is null");
    SqParams p{};
    SCANN_TRY(sq_params_checked(bits, mode, params4, &p));
    if (n == 0) return SCANN_HIP_OK;
    if (!d_rows || !d_out || dim == 0 || stride < dim || out_stride < dim)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "quantize rows: null rows/output or a stride below dim");
    if (n > UINT64_MAX / std::max(stride, out_stride)) return fail(SCANN_HIP_OUT_OF_RANGE, "quantize rows: n * stride overflows");
    SCANN_HIP_CHECK(hipSetDevice(ctx_device(ctx)));
    return launch_sq_quantize(d_rows, n, dim, stride, SCANN_HIP_ROWS_INT8, mode, p, d_out, out_stride,
                              static_cast<hipStream_t>(hip_stream));
}

}  // extern "C"

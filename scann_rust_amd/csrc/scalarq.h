// scalarq.h -- the reference's ScalarQuantizer on the device: QuantizationStats::from_dataset
// (quantization/mod.rs:75-110) as a fixed-order two-launch reduction, calibrate / quantize_value / dequantize_value
// (quantization/scalar.rs:103-172) as one arithmetic shared by the host entry points and the kernels, and the row
// passes f32 -> int8 / bf16 / FP8 E4M3 that scann_hip_index_quantize_rows builds handles from.
#pragma once
#include <limits.h>

#include "common.h"

namespace scann {

// ---- the summation order of the stats pass (part of the contract; tests/scalar_quantizer_model.py restates it) ----
// The n * dim logical values, row-major, are cut into chunks of kSqChunk; chunk c is reduced by one workgroup of
// kSqThreads threads.  Thread t adds, in this order, the values 4 g .. 4 g + 3 of the chunk for g = t, t + 256, ...
// (sum += (double)v; sum_sq += (double)v * (double)v, unfused), then the 256 thread sums are added as a tree
// (s[t] += s[t + off] for off = 128, 64, ..., 1).  The final launch gives thread t the partials t, t + 256, ... in
// order and ends with the same tree.  Nothing depends on the grid, the CU count or the stride.
constexpr uint32_t kSqChunk = 16384;
constexpr uint32_t kSqThreads = 256;
constexpr uint32_t kSqGroupStep = 4 * kSqThreads;   // logical distance between a thread's groups of four

struct SqPartial {   // one chunk's (and, from the final launch, the dataset's) sums; 32 bytes
    double sum, sum_sq;
    float mn, mx, amax;      // fminf / fmaxf folds from f32::MAX / f32::MIN / 0: a NaN operand is ignored
    uint32_t nonfinite;      // 1 when a value is NaN or +-inf
};

struct SqParams {   // a calibrated quantizer: params4 of the C ABI plus the level count
    float mn, mx, scale, inv_scale;
    int32_t levels;
};

// ---- element arithmetic, host and device ------------------------------------------------------------------------
// f32 -> i32 as Rust's `as`: saturating, NaN -> 0
__host__ __device__ inline int32_t sq_f32_as_i32(float t) {
    if (!(t == t)) return 0;
    if (t >= 2147483648.0f) return INT_MAX;
    if (t <= -2147483648.0f) return INT_MIN;
    return (int32_t)t;
}

// ScalarQuantizer::quantize_value (scalar.rs:162-166): clamp (a NaN stays), round half away from zero, `as i32`,
// clamp to [0, levels], `as i8` (128..255 wrap to -128..-1: offset-binary bytes)
__host__ __device__ inline int8_t sq_ref_code(float v, const SqParams &p) {
    float c = v;
    if (c < p.mn) c = p.mn;
    else if (c > p.mx) c = p.mx;
    const float d = c - p.mn;
    const float t = roundf(d * p.inv_scale);
    int32_t q = sq_f32_as_i32(t);
    q = q < 0 ? 0 : (q > p.levels ? p.levels : q);
    return (int8_t)(uint8_t)q;
}

// hip.symmetric_int8: clip(rint(x / s), -127, 127), a correctly rounded division; NaN -> 0
__host__ __device__ inline int8_t sq_signed_code(float v, float s) {
    float t = rintf(v / s);
    if (!(t == t)) return 0;   // (fmaxf / fminf would drop the NaN and keep the bound)
    t = fminf(fmaxf(t, -127.0f), 127.0f);
    return (int8_t)(int)t;
}

// ---- host arithmetic (scalarq.hip) ---------------------------------------------------------------------------------
// mean / std_dev of quantization/mod.rs:96-102 from the reduced sums; out4 = min, max, mean, std_dev
void sq_stats_finish(const SqPartial &r, uint64_t count, float *out4);
// scann_hip_scalar_quantizer_calibrate without the output-pointer checks; writes nothing on failure
int sq_calibrate(const float *stats4, uint32_t bits, int mode, float a, float b, SqParams *out, int32_t *zero_point);
// mode / bits / params of a quantize call -> SqParams (InvalidArgument on a bad one)
int sq_params_checked(uint32_t bits, int mode, const float *params4, SqParams *out);

// ---- launches -------------------------------------------------------------------------------------------------------
// sq_stats_kernel + sq_stats_final_kernel over n rows of dim values at `stride`; synchronises `st` and returns the sums
int sq_stats_device(const float *d_rows, uint64_t n, uint32_t dim, uint32_t stride, hipStream_t st, SqPartial *out);
// f32 rows -> rows of out_stride elements of `fmt` (SCANN_HIP_ROWS_*; INT8: `mode` and `p`), pad columns 0; enqueue only
int launch_sq_quantize(const float *d_rows, uint64_t n, uint32_t dim, uint32_t stride, int fmt, int mode,
                       const SqParams &p, void *d_out, uint32_t out_stride, hipStream_t st);

}  // namespace scann

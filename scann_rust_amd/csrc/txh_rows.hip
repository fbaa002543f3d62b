// txh_rows.hip -- the 8-bit row stores of the exact re-rank's row filter (K8b, described in txh.hip): the int8 and FP8
// store builds, the reference's FP8 codec, and rerank_i8_kernel, which brackets every candidate from its 8-bit row;
// and rerank_quant_kernel (K8q), the re-rank of a handle whose rows the caller stores as bf16, FP8 E4M3 or int8.
#include "launch.h"
#include "quant.h"
#include "txh_stages.h"

namespace scann {

__global__ __launch_bounds__(256) void rows_i8_build_kernel(const float *__restrict__ rows, uint64_t n, uint32_t dim,
                                                            uint32_t stride, int8_t *__restrict__ rows8,
                                                            float2 *__restrict__ meta, float uni_scale) {
    // 8 lanes per row
    const uint64_t r = (uint64_t)blockIdx.x * 32 + (threadIdx.x >> 3);
    const uint32_t l8 = threadIdx.x & 7u;
    const bool act = r < n;
    const float *row = rows + (act ? r : 0) * stride;
    float mx = 0.0f;
    for (uint32_t j = l8; j < dim; j += 8) mx = fmaxf(mx, fabsf(row[j]));
    mx = fmaxf(mx, __shfl_xor(mx, 1, 8));
    mx = fmaxf(mx, __shfl_xor(mx, 2, 8));
    mx = fmaxf(mx, __shfl_xor(mx, 4, 8));
    const bool finite = mx < __builtin_inff();      // (NaN rows: mx stays finite-or-NaN; the error below turns NaN)
    const float sc = uni_scale > 0.0f ? uni_scale : (mx > 0.0f && finite) ? mx / 127.0f : 1.0f;
    float err = 0.0f;
    for (uint32_t j = l8; j < dim; j += 8) {
        const float x = row[j];
        float t = rintf(x / sc);
        t = fminf(fmaxf(t, -127.0f), 127.0f);
        if (act) rows8[r * dim + j] = (int8_t)(t == t ? (int)t : 0);
        const float e = x - sc * (t == t ? t : 0.0f);
        err = err + e * e;
    }
    err += __shfl_xor(err, 1, 8);
    err += __shfl_xor(err, 2, 8);
    err += __shfl_xor(err, 4, 8);
    if (act && l8 == 0) {
        // E rounded up a little (the sum above is f32); a NaN / infinite row gets E = +inf: never filtered out
        float E = sqrtf(err) * 1.0001f + 1e-30f;
        if (!(E == E) || !finite) E = __builtin_inff();
        meta[r] = make_float2(sc, E);
    }
}

// ---- the reference's FP8 codec (quantization/fp8.rs:80-203), bit for bit -----------------------------
// (the encoder fp8_from_f32: quant.h, shared with the f32 -> FP8 row pass of scalarq.hip)
__device__ __forceinline__ float fp8_to_f32(uint32_t b, int format) {
    const int mbits = format ? 2 : 3, bias = format ? 15 : 7;
    const uint32_t sign = (b >> 7) & 1u;
    const int exp = (int)((b >> mbits) & (format ? 0x1Fu : 0xFu));
    const uint32_t mantissa = b & ((1u << mbits) - 1u);
    if (exp == 0 && mantissa == 0) return sign ? -0.0f : 0.0f;
    const int e32 = exp == 0 ? 126 - bias : exp - bias + 127;
    return __uint_as_float((sign << 31) | ((uint32_t)e32 << 23) | (mantissa << (23 - mbits)));
}

// Quantizer::quantize / dequantize over Fp8Quantizer (fp8.rs:247-268)
__global__ __launch_bounds__(256) void fp8_quantize_kernel(const float *__restrict__ values, uint64_t n, float scale,
                                                           int format, uint8_t *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
        out[i] = (uint8_t)fp8_from_f32(values[i] * scale, format);
}

__global__ __launch_bounds__(256) void fp8_dequantize_kernel(const uint8_t *__restrict__ bits, uint64_t n, float scale,
                                                             int format, float *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
        out[i] = fp8_to_f32(bits[i], format) / scale;
}

// one_to_many_fp8_float_{squared_l2, dot_product} (distance_measures/one_to_many_asymmetric.rs:327-377):
// E4M3 rows, one sequential f32 sum per row (no FMA), the dot product negated.
__global__ __launch_bounds__(256) void fp8_one_to_many_kernel(const float *__restrict__ query, uint32_t dim,
                                                              const uint8_t *__restrict__ db, uint64_t stride,
                                                              uint64_t n, int dot, float *__restrict__ out) {
    extern __shared__ float s_q8[];   // [dim]
    for (uint32_t j = threadIdx.x; j < dim; j += 256) s_q8[j] = query[j];
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint8_t *row = db + i * stride;
        float sum = 0.0f;
        if (dot) {
            for (uint32_t j = 0; j < dim; ++j) sum = sum + s_q8[j] * fp8_to_f32(row[j], 0);
            out[i] = -sum;
        } else {
            for (uint32_t j = 0; j < dim; ++j) {
                const float diff = s_q8[j] - fp8_to_f32(row[j], 0);
                sum = sum + diff * diff;
            }
            out[i] = sum;
        }
    }
}

// The FP8 row store of the re-rank filter: the reference's E4M3 codec with Fp8Quantizer::calibrate_scale
// per row (scale = 448 / max|x|, fp8.rs:238-244); the filter decodes with v_cvt_pk_f32_fp8 (gfx950: OCP
// E4M3 -- equal to the reference's decode on every code its encoder emits) as x~ = dec * (1 / scale), and E
// is computed from that same expression.  `mismatch` counts codes the hardware decodes differently
// (never, unless the conversion instruction means another format: the create call then fails).
__global__ __launch_bounds__(256) void rows_fp8_build_kernel(const float *__restrict__ rows, uint64_t n, uint32_t dim,
                                                             uint32_t stride, uint8_t *__restrict__ rows8,
                                                             float2 *__restrict__ meta, uint32_t *__restrict__ mismatch) {
    const uint64_t r = (uint64_t)blockIdx.x * 32 + (threadIdx.x >> 3);
    const uint32_t l8 = threadIdx.x & 7u;
    const bool act = r < n;
    const float *row = rows + (act ? r : 0) * stride;
    float mx = 0.0f;
    for (uint32_t j = l8; j < dim; j += 8) mx = fmaxf(mx, fabsf(row[j]));
    mx = fmaxf(mx, __shfl_xor(mx, 1, 8));
    mx = fmaxf(mx, __shfl_xor(mx, 2, 8));
    mx = fmaxf(mx, __shfl_xor(mx, 4, 8));
    const bool finite = mx < __builtin_inff();
    const float scale = 448.0f / fmaxf(finite ? mx : 1.0f, 1e-10f);
    const float inv = 1.0f / scale;
    float err = 0.0f;
    uint32_t bad = 0;
    for (uint32_t j = l8; j < dim; j += 8) {
        const float x = row[j];
        const uint32_t b = fp8_from_f32(x * scale, 0);
        const float hw = __builtin_amdgcn_cvt_f32_fp8((int)b, 0);
        bad += (__float_as_uint(hw) != __float_as_uint(fp8_to_f32(b, 0))) ? 1u : 0u;
        if (act) rows8[r * dim + j] = (uint8_t)b;
        const float e = x - hw * inv;
        err = err + e * e;
    }
    err += __shfl_xor(err, 1, 8);
    err += __shfl_xor(err, 2, 8);
    err += __shfl_xor(err, 4, 8);
    if (act && bad) atomicAdd(mismatch, bad);
    if (act && l8 == 0) {
        float E = sqrtf(err) * 1.0001f + 1e-30f;
        if (!(E == E) || !finite) E = __builtin_inff();
        meta[r] = make_float2(inv, E);
    }
}

struct I8RerankArgs {
    const int8_t *rows8;      // [n_rows][dim] int8, or the reference's E4M3 codes (FMT = 1)
    const float2 *meta;       // [n_rows] {dequantisation factor, error norm}
    float uni_scale, uni_E;   // UNI form: one dequantisation factor and one error bound for every row (no meta gather)
    const float *queries;
    uint32_t q_stride, m;
    const uint32_t *cand_row, *cand_count;
    uint32_t *lb, *ub;        // [nq][m] ordered(L), ordered(U)
};

constexpr uint32_t kI8PerBlock = 256;   // candidates per block (8 lanes each, 8 rounds): amortises the query staging

// DPP exchanges inside a group of 8 lanes (no LDS crossbar): quad_perm [1,0,3,2], quad_perm [2,3,0,1], and
// row_half_mirror (lane i <-> 7 - i, the other quad of the group)
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppHalfMirror = 0x141;
template <int CTRL> __device__ __forceinline__ int dpp_get(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }
template <int CTRL> __device__ __forceinline__ float dpp_get(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}

// the sum over a group's 8 lanes, the same bits in each of them (every step adds the same two values in both lanes)
__device__ __forceinline__ float sum8(float v) {
    v += dpp_get<kDppXor1>(v);
    v += dpp_get<kDppXor2>(v);
    return v + dpp_get<kDppHalfMirror>(v);
}

// v[r] in every lane of a group -> lane l8 gets the group's sum of v[l8]: three exchange steps, each halving the
// rounds a lane still carries (7 exchanges, against 8 x 3 for a full sum per round plus the moves)
template <typename T> __device__ __forceinline__ T sum8_transposed(const T (&v)[8], uint32_t l8) {
    const bool h4 = l8 & 4u, h2 = l8 & 2u, h1 = l8 & 1u;
    T a[4], b[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = (h4 ? v[i + 4] : v[i]) + dpp_get<kDppHalfMirror>(h4 ? v[i] : v[i + 4]);
#pragma unroll
    for (int i = 0; i < 2; ++i) b[i] = (h2 ? a[i + 2] : a[i]) + dpp_get<kDppXor2>(h2 ? a[i] : a[i + 2]);
    return (h1 ? b[1] : b[0]) + dpp_get<kDppXor1>(h1 ? b[0] : b[1]);
}

// [L, U] around the exact f32 distance from d~ = acc, the row's error norm E and B, a bound on what the arithmetic
// that produced acc lost beyond the (dim + 8) 1.2e-7 |acc| of two dim-term f32 sums (0 for the per-dimension form).
//   | d_f32 - d~ | <= 2 sqrt(d~) E + E^2 (triangle inequality on the real values; d~ itself known to +- B, hence
//   sqrt(max(acc, 0) + B)) + the f32 rounding of the sums + B + slack on the bound itself
template <bool EXPANDED>   // false: acc is a sum of squares (>= 0 or NaN), B = 0
__device__ __forceinline__ void store_bracket(const I8RerankArgs &a, size_t at, uint32_t dim, float acc, float E, float B) {
    const float slack = EXPANDED ? (2.0f * sqrtf(fmaxf(acc, 0.0f) + B) * E + E * E) * 1.0001f +
                                       fabsf(acc) * ((float)(dim + 8) * 1.2e-7f) + B + 1e-30f
                                 : (2.0f * sqrtf(acc) * E + E * E) * 1.0001f + acc * ((float)(dim + 8) * 1.2e-7f) + 1e-30f;
    float L = acc - slack, U = acc + slack;
    // NaN or overflow anywhere (an infinite d~ would make L = inf - inf = NaN, which orders above +inf and
    // drops the candidate): never filtered out, never a bound for others
    if (!(slack < __builtin_inff()) || !(acc < __builtin_inff())) {
        L = -__builtin_inff();
        U = __builtin_inff();
    }
    a.lb[at] = f32_to_ordered(L);
    a.ub[at] = f32_to_ordered(U);
}

// FMT: 0 = int8 rows, 1 = FP8 (E4M3) rows.
// EX (SCANN_HIP_RERANK_EXPAND): 0 = d~ summed per dimension as (q - s x8)^2, one epilogue per round in lane 0 of each
// group.  1, 2, 3 = one epilogue per wave: the 8 rounds leave their sums transposed, lane l8 of a group holding round
// l8's, so that 64 lanes finish 64 candidates at once; int8 rows of the one-scale store by the expanded square
//     d~ = Q2 - 2 s D + s^2 N,   N = sum x8^2 (exact, v_dot4 on the packed bytes),   D = sum q x8 (f32, one convert and
// one FMA per dimension),   Q2 = |q|^2
// with the lane's 16-dim slices of the query in registers for 2: one, 3: two 128-dim passes, 1: read from LDS (any dim);
// FP8 rows keep the per-dimension sum (EX = 1).  int8 rows with a scale per row stay on EX = 0 whatever the knob says:
// they go with rows of unequal magnitude, and on the clustered 10M x 128 set (candidates nearly equidistant,
// |q|^2 >> d) the expanded form's cancellation term B lengthened the shortlists: rerank_short_kernel 130 -> 340 us at
// m = 8192, 800 k -> 670 k QPS (profiles/rerank_expand_10m_perrow_expanded_*).
template <int FMT, bool UNI = false, int EX = 0>
__global__ __launch_bounds__(256) void rerank_i8_kernel(uint32_t dim, I8RerankArgs a) {
    typedef float v2f __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) float s_q[];   // [dim]
    const uint32_t q = blockIdx.y, tid = threadIdx.x;
    const uint32_t nsel = a.cand_count[q];
    const uint32_t c0 = blockIdx.x * kI8PerBlock;
    if (c0 >= nsel) return;   // uniform
    for (uint32_t j = tid; j < dim; j += 256) s_q[j] = a.queries[(size_t)q * a.q_stride + j];
    __syncthreads();
    const uint32_t l8 = tid & 7u;
    constexpr int R = kI8PerBlock / 32;
    uint32_t row[R];
#pragma unroll
    for (int it = 0; it < R; ++it) {   // the rounds' row ids first: their gathers then overlap
        const uint32_t c = c0 + (uint32_t)it * 32u + (tid >> 3);
        row[it] = c < nsel ? a.cand_row[(size_t)q * a.m + c] : 0u;
    }
    if constexpr (EX == 0) {
#pragma unroll
        for (int it = 0; it < R; ++it) {
            const uint32_t c = c0 + (uint32_t)it * 32u + (tid >> 3);
            const bool act = c < nsel;
            const float2 me = UNI ? make_float2(a.uni_scale, a.uni_E) : a.meta[row[it]];
            const int8_t *r8 = a.rows8 + (size_t)row[it] * dim;
            float acc = 0.0f;
            for (uint32_t j0 = l8 * 16u; j0 < dim; j0 += 128u) {   // 16 dims per lane per pass (dim % 16 == 0)
                const uint4 v = *reinterpret_cast<const uint4 *>(r8 + j0);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                if constexpr (FMT == 1) {
#pragma unroll
                    for (int wi = 0; wi < 4; ++wi) {
                        const v2f lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[wi], false);
                        const v2f hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[wi], true);
                        const float xs[4] = {lo.x, lo.y, hi.x, hi.y};
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float d = s_q[j0 + wi * 4 + i] - xs[i] * me.x;
                            acc = fmaf(d, d, acc);
                        }
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const float x = me.x * (float)(int)(int8_t)(w[i >> 2] >> (8 * (i & 3)));
                        const float d = s_q[j0 + i] - x;
                        acc = fmaf(d, d, acc);
                    }
                }
            }
            acc += __shfl_xor(acc, 1, 8);
            acc += __shfl_xor(acc, 2, 8);
            acc += __shfl_xor(acc, 4, 8);
            if (act && l8 == 0) store_bracket<false>(a, (size_t)q * a.m + c, dim, acc, me.y, 0.0f);
        }
    } else {
        // the candidate this lane finishes: round l8 of its group (its meta line is in flight under the rounds)
        const uint32_t ce = c0 + l8 * 32u + (tid >> 3);
        const bool acte = ce < nsel;
        const float2 mee = UNI ? make_float2(a.uni_scale, a.uni_E) : a.meta[acte ? a.cand_row[(size_t)q * a.m + ce] : 0u];
        if constexpr (FMT == 1) {
            float accv[R];
#pragma unroll
            for (int it = 0; it < R; ++it) {
                const float inv = a.meta[row[it]].x;
                const int8_t *r8 = a.rows8 + (size_t)row[it] * dim;
                float acc = 0.0f;
                for (uint32_t j0 = l8 * 16u; j0 < dim; j0 += 128u) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(r8 + j0);
                    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int wi = 0; wi < 4; ++wi) {
                        const v2f lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[wi], false);
                        const v2f hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[wi], true);
                        const float xs[4] = {lo.x, lo.y, hi.x, hi.y};
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float d = s_q[j0 + wi * 4 + i] - xs[i] * inv;
                            acc = fmaf(d, d, acc);
                        }
                    }
                }
                accv[it] = acc;
            }
            const float acc = sum8_transposed(accv, l8);
            if (acte) store_bracket<false>(a, (size_t)q * a.m + ce, dim, acc, mee.y, 0.0f);
        } else {
            constexpr int NP = EX - 1;   // 128-dim passes with the query slice in registers (0: LDS)
            float qr[NP > 0 ? NP : 1][16];
            float q2 = 0.0f;             // |q|^2: the lane's slices in dimension order, then the group's 8 partial sums
            if constexpr (NP > 0) {
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const uint32_t j0 = l8 * 16u + (uint32_t)p * 128u;
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        qr[p][i] = j0 < dim ? s_q[j0 + i] : 0.0f;
                        q2 = fmaf(qr[p][i], qr[p][i], q2);
                    }
                }
            } else {
                for (uint32_t j0 = l8 * 16u; j0 < dim; j0 += 128u)
#pragma unroll
                    for (int i = 0; i < 16; ++i) q2 = fmaf(s_q[j0 + i], s_q[j0 + i], q2);
            }
            q2 = sum8(q2);
            float Dv[R];
            int Nv[R];
#pragma unroll
            for (int it = 0; it < R; ++it) {
                const int8_t *r8 = a.rows8 + (size_t)row[it] * dim;
                float D = 0.0f;
                int N = 0;
                auto pass = [&](uint32_t j0, int &Np, auto qat) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(r8 + j0);
                    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int wi = 0; wi < 4; ++wi) Np = __builtin_amdgcn_sdot4((int)w[wi], (int)w[wi], Np, false);
#pragma unroll
                    for (int i = 0; i < 16; ++i) D = fmaf(qat(i), (float)(int)(int8_t)(w[i >> 2] >> (8 * (i & 3))), D);
                };
                if constexpr (NP > 0) {
                    // no branch around a slice past the row's end: the lane reads the row's first 16 bytes instead,
                    // which its zero query slice keeps out of D and the select keeps out of N
#pragma unroll
                    for (int p = 0; p < NP; ++p) {
                        const uint32_t j0 = l8 * 16u + (uint32_t)p * 128u;
                        int Np = 0;
                        pass(j0 < dim ? j0 : 0u, Np, [&](int i) { return qr[p][i]; });
                        N += j0 < dim ? Np : 0;
                    }
                } else {
                    for (uint32_t j0 = l8 * 16u; j0 < dim; j0 += 128u) pass(j0, N, [&](int i) { return s_q[j0 + i]; });
                }
                Dv[it] = D;
                Nv[it] = N;
            }
            const float D = sum8_transposed(Dv, l8);
            const float Nf = (float)sum8_transposed(Nv, l8);   // <= dim 127^2: exact in f32 up to dim 1040
            const float s = mee.x;
            const float acc = (q2 - (2.0f * s) * D) + (s * s) * Nf;
            // the three terms cancel down to d~: each carries a rounding of up to (dim + 8) 2^-24 of its own
            // magnitude, and Q2 + 2 s |D| + s^2 N <= (|q| + s |x8|)^2
            const float rt = sqrtf(q2) + s * sqrtf(Nf);
            const float B = rt * rt * ((float)(dim + 8) * 1.2e-7f);
            if (acte) store_bracket<true>(a, (size_t)q * a.m + ce, dim, acc, mee.y, B);
        }
    }
}

// K8b, first launch: the bracket [L, U] of every candidate's exact distance from its 8-bit row
int launch_rerank_i8(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st) {
    const size_t lds_rr = (size_t)ix.dim * 4;
    I8RerankArgs ia;
    ia.rows8 = ix.rows8; ia.meta = reinterpret_cast<const float2 *>(ix.rows8_meta); ia.queries = w.queries;
    ia.q_stride = w.q_stride; ia.m = w.m; ia.cand_row = w.cand_row; ia.cand_count = w.cand_count;
    ia.lb = w.rr_lb; ia.ub = w.rr_ub;
    ia.uni_scale = ix.rows8_scale; ia.uni_E = ix.rows8_emax;
    const bool fp8 = ix.rows8_fmt == 1;
    const int ex = !w.i8_expand || (!fp8 && !ix.rows8_uniform) ? 0 : fp8 || ix.dim > 256 ? 1 : ix.dim <= 128 ? 2 : 3;
    // 1: FP8 rows; int8 rows with 2: one scale for all rows, 0: a scale per row
    return with_value<1, 2, 0>(fp8 ? 1 : ix.rows8_uniform ? 2 : 0, [&](auto v) {
        return with_value<0, 1, 2, 3>(ex, [&](auto e) {
            // (per-row int8: EX = 0 only; FP8: 0 or 1; the register forms are the one-scale store's)
            constexpr int EX = v() == 0 ? 0 : (v() == 1 && e() > 1) ? 1 : e();
            return launch((rerank_i8_kernel<v() == 1 ? 1 : 0, v() == 2, EX>), dim3(ceil_div_u32(w.m, kI8PerBlock), w.nq),
                          dim3(256), lds_rr, st, ix.dim, ia);
        });
    });
}

// =====================================================================================
// K8q: re-rank over rows stored quantized (scann_hip_txh_create_quantized).  Every candidate gets the distance a
// quantized brute-force handle gives the same query and row (bf_quant_kernel's arithmetic, quant.h): bf16 / FP8 one
// sequential f32 sum, no FMA; int8 8 FMA chains over full 8-element chunks, horizontal_sum_avx, an unfused tail.
// A sequential sum cannot be split over lanes, so one lane owns one candidate -- and 64 lanes walking 64 different
// rows straight from global memory would fetch a cache line per lane and step.  Instead the workgroup's 256 candidate
// rows pass through LDS in pieces of 128 bytes (one cache line): a group of 8 lanes loads one row's piece as 8 x 16
// bytes, a wave 8 rows per instruction, and every lane has its 8 rows' loads in flight before the first LDS store.
// Row pitch 33 dwords: lane t reads dword 33 t + j, bank (t + j) mod 32 -- no conflict among the 32 lanes of a
// ds_read_b32 group; the stores (row r, dword 4 l8 + i -> bank (r + 4 l8 + i) mod 32, r < 4 per group) have none either.
// The gather of one workgroup overlaps the chains of the others on its CU (35 KB of LDS: four workgroups per CU).
// Rows whose byte stride or base is not a multiple of 16, and the piece that holds a row's last bytes when those are
// not 16, are copied byte by byte: no element past dim is read.  Row offsets are 64-bit.
// =====================================================================================
constexpr uint32_t kQrTile = 256;                  // candidates per workgroup, one per lane
constexpr uint32_t kQrPiece = 128;                 // row bytes in LDS at a time
constexpr uint32_t kQrPitchW = kQrPiece / 4 + 1;   // dwords from one row's piece to the next

static inline size_t rerank_quant_lds(uint32_t dim) {
    return ((size_t)((dim + 3u) & ~3u) + kQrTile + (size_t)kQrTile * kQrPitchW) * 4;
}

template <int FMT, int MEASURE>
__global__ __launch_bounds__(256) void rerank_quant_kernel(TxhIndexDev ix, const float *__restrict__ queries,
                                                           uint32_t q_stride, uint32_t m,
                                                           const uint32_t *__restrict__ cand_row,
                                                           const uint32_t *__restrict__ cand_count,
                                                           float *__restrict__ cand_exact) {
    constexpr uint32_t B = quant_bytes<FMT>(), EPW = 4 / B;   // bytes per element, elements per dword
    constexpr bool FUSED = FMT == SCANN_HIP_ROWS_INT8;
    constexpr int NCH = FUSED ? 8 : 1;
    extern __shared__ __attribute__((aligned(16))) float s_q[];   // [dim, padded to 4] query | [256] rows | [256][33] tile
    const uint32_t q = blockIdx.y, tid = threadIdx.x, dim = ix.dim;
    const uint32_t nsel = cand_count[q];
    const uint32_t c0 = blockIdx.x * kQrTile;
    if (c0 >= nsel) return;   // uniform
    const uint32_t cnt = min(kQrTile, nsel - c0);
    uint32_t *s_row = reinterpret_cast<uint32_t *>(s_q + ((dim + 3u) & ~3u));
    uint32_t *s_tile = s_row + kQrTile;
    for (uint32_t j = tid; j < dim; j += 256) s_q[j] = queries[(size_t)q * q_stride + j];
    s_row[tid] = tid < cnt ? cand_row[(size_t)q * m + c0 + tid] : 0u;
    __syncthreads();
    const uint8_t *base = static_cast<const uint8_t *>(ix.qrows);
    const size_t row_bytes = (size_t)ix.stride * B;
    const bool vec = (row_bytes & 15u) == 0 && (reinterpret_cast<uintptr_t>(base) & 15u) == 0;
    const uint32_t l8 = tid & 7u, g = tid >> 3, off = l8 * 16u;
    const uint32_t dim_bytes = dim * B;
    const bool act = tid < cnt;
    const float inv = ix.inv_mult;
    const uint32_t *trow = s_tile + (size_t)tid * kQrPitchW;
    f32x2q acc[NCH];
#pragma unroll
    for (int t = 0; t < NCH; ++t) acc[t] = f32x2q{0.0f, 0.0f};
    for (uint32_t b0 = 0; b0 < dim_bytes; b0 += kQrPiece) {
        const uint32_t valid = min(kQrPiece, dim_bytes - b0);                  // bytes of the rows in this piece
        const uint32_t nb = off < valid ? min(16u, valid - off) : 0u;          // ... of them in this lane's 16
        if (vec && nb == 16u) {
            uint4 v[8];
#pragma unroll
            for (int p = 0; p < 8; ++p) {   // the 8 rows' loads first: all in flight together
                const uint32_t r = g + 32u * p;
                v[p] = make_uint4(0u, 0u, 0u, 0u);
                if (r < cnt) v[p] = *reinterpret_cast<const uint4 *>(base + (size_t)s_row[r] * row_bytes + b0 + off);
            }
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const uint32_t r = g + 32u * p;
                if (r < cnt) {
                    uint32_t *d = s_tile + (size_t)r * kQrPitchW + l8 * 4u;
                    d[0] = v[p].x; d[1] = v[p].y; d[2] = v[p].z; d[3] = v[p].w;
                }
            }
        } else if (nb) {
            for (uint32_t r = g; r < cnt; r += 32u) {
                const uint8_t *src = base + (size_t)s_row[r] * row_bytes + b0 + off;
                uint8_t *d = reinterpret_cast<uint8_t *>(s_tile + (size_t)r * kQrPitchW) + off;
                for (uint32_t i = 0; i < nb; ++i) d[i] = src[i];
            }
        }
        __syncthreads();
        const uint32_t e0 = b0 / B, ne = valid / B, full = ne & ~7u;
        if (act) {
            for (uint32_t j = 0; j < full; j += 8) {   // full 8-element chunks (int8: the FMA chains)
                uint32_t w[8 / EPW];
#pragma unroll
                for (int i = 0; i < (int)(8 / EPW); ++i) w[i] = trow[j / EPW + i];
#pragma unroll
                for (int t = 0; t < 8; ++t)
                    quant_step<MEASURE, FUSED>(acc[FUSED ? t : 0], f32x2q{s_q[e0 + j + t], 0.0f},
                                               quant_decode<FMT>(w[t / (int)EPW], t % (int)EPW, inv));
            }
            if (b0 + kQrPiece >= dim_bytes) {   // the row's last piece: the tail, then the result
                f32x2q r = acc[0];
                if constexpr (FUSED)   // horizontal_sum_avx
                    r = ((acc[0] + acc[4]) + (acc[1] + acc[5])) + ((acc[2] + acc[6]) + (acc[3] + acc[7]));
                for (uint32_t j = full; j < ne; ++j)   // bf16 / FP8: the rest of the sequential sum; int8: the unfused tail
                    quant_step<MEASURE, false>(r, f32x2q{s_q[e0 + j], 0.0f},
                                               quant_decode<FMT>(trow[j / EPW], (int)(j % EPW), inv));
                float dist = r.x;
                if (MEASURE == SCANN_HIP_DOT_PRODUCT) dist = -dist;
                if (MEASURE == SCANN_HIP_L2) dist = sqrtf(dist);
                cand_exact[(size_t)q * m + c0 + tid] = dist;
            }
        }
        __syncthreads();   // the next piece overwrites the tile
    }
}

int launch_rerank_quant(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st) {
    return with_row_format(ix.qfmt, [&](auto fmt) {
        return with_dot_measure(ix.measure, [&](auto ms) {
            if constexpr (fmt() == 0) {
                return fail(SCANN_HIP_INTERNAL, "quantized re-rank without quantized rows");
            } else {
                return launch((rerank_quant_kernel<fmt(), ms()>), dim3(ceil_div_u32(w.m, kQrTile), w.nq), dim3(256),
                              rerank_quant_lds(ix.dim), st, ix, w.queries, w.q_stride, w.m, w.cand_row, w.cand_count,
                              w.cand_exact);
            }
        });
    });
}

int launch_rows_fp8_build(const float *d_rows, uint64_t n, uint32_t dim, uint32_t stride, uint8_t *d_rows8,
                          void *d_meta, uint32_t *d_mismatch, hipStream_t st) {
    if (n == 0) return SCANN_HIP_OK;
    SCANN_TRY(launch(rows_fp8_build_kernel, dim3((uint32_t)ceil_div_u64(n, 32)), dim3(256), 0, st, d_rows, n, dim,
                     stride, d_rows8, reinterpret_cast<float2 *>(d_meta), d_mismatch));
    return SCANN_HIP_OK;
}

int launch_fp8_quantize(const float *d_values, uint64_t n, float scale, int format, uint8_t *d_out, hipStream_t st) {
    if (n == 0) return SCANN_HIP_OK;
    SCANN_TRY(launch(fp8_quantize_kernel, dim3((uint32_t)std::min<uint64_t>(ceil_div_u64(n, 256), 65535)), dim3(256), 0,
                     st, d_values, n, scale, format, d_out));
    return SCANN_HIP_OK;
}

int launch_fp8_dequantize(const uint8_t *d_bits, uint64_t n, float scale, int format, float *d_out, hipStream_t st) {
    if (n == 0) return SCANN_HIP_OK;
    SCANN_TRY(launch(fp8_dequantize_kernel, dim3((uint32_t)std::min<uint64_t>(ceil_div_u64(n, 256), 65535)), dim3(256),
                     0, st, d_bits, n, scale, format, d_out));
    return SCANN_HIP_OK;
}

int launch_fp8_one_to_many(const float *d_query, uint32_t dim, const uint8_t *d_db, uint64_t stride, uint64_t n,
                           int dot, float *d_out, hipStream_t st) {
    if (n == 0) return SCANN_HIP_OK;
    const size_t lds = (size_t)dim * sizeof(float);
    SCANN_TRY(launch(fp8_one_to_many_kernel, dim3((uint32_t)std::min<uint64_t>(ceil_div_u64(n, 256), 65535)),
                     dim3(256), lds, st, d_query, dim, d_db, stride, n, dot, d_out));
    return SCANN_HIP_OK;
}

int launch_rows_i8_build(const float *d_rows, uint64_t n, uint32_t dim, uint32_t stride, int8_t *d_rows8,
                         void *d_meta, hipStream_t st, float uni_scale) {
    if (n == 0) return SCANN_HIP_OK;
    SCANN_TRY(launch(rows_i8_build_kernel, dim3((uint32_t)ceil_div_u64(n, 32)), dim3(256), 0, st, d_rows, n, dim,
                     stride, d_rows8, reinterpret_cast<float2 *>(d_meta), uni_scale));
    return SCANN_HIP_OK;
}

}  // namespace scann

// bf_int.hip -- the shortlist pass of brute force over integer-coded rows on the integer matrix cores
// (v_mfma_i32_32x32x32_i8), DESIGN.md 3.3b-i.
//
// The row operand is the stored code itself as int8 (packed int4 rows: nibble - 8, unpacked in registers on the way
// into LDS).  The query is split once per batch into D int8 digit planes,
//   q = s_1 d_1 + s_2 d_2 (+ s_3 d_3) + e_q,   s_1 = qmax / 127,  s_{t+1} = s_t / 254,  every digit in [-127, 127],
// so every partial sum x.d_t is an exact i32 and the score is sum_t (s_t inv_mult) (x.d_t), combined in f32 once per
// (row, query).  Each k-step of 32 elements issues D MFMAs of twice the bf16 instruction's depth.  What follows the
// scores (threshold, filter into the candidate lists, selection, exact re-score, verification) is bf.hip's.
#include "bf_int.h"

#include <algorithm>
#include <cmath>

#include "launch.h"
#include "quant.h"

namespace scann {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// Dropped residual: |e_q|inf <= s_D / 2 = delta_D qmax with delta_D = 1 / (2 * 127 * 254^(D-1)), so
// |e_q.x| <= delta_D sqrt(dim) |q||x| (qmax <= |q|, |x|_1 <= sqrt(dim) |x|); the pass carries the tighter per-query
// |e_q|_2 instead (D = 0 here).  The MFMA sums are exact.  What remains, relative to |q||x|:
//   f32 recombination: D products and D - 1 sums of terms <= 1.07 |q||x| (|s_t d_t|_2 <= |q| + sqrt(dim) qmax / 254),
//   the rounded weights s_t inv_mult: under 8 roundings of 2^-24                                   <= 4 * 2^-23
//   the exact path against the real dot product: its sum of dim products (dim + 64 roundings)      <= (dim + 64) 2^-23
//   the reference's rounded elements fl(code inv_mult), as in shortlist_quant_err                  <= 2^-23
float shortlist_int_err(uint32_t dim, int digits) {
    float delta = 0.0f;
    if (digits > 0) {
        delta = 1.0f / 254.0f;
        for (int t = 1; t < digits; ++t) delta /= 254.0f;
    }
    return 1.01f * (delta * std::sqrt((float)dim) + ((float)dim + 64.0f + 4.0f + 1.0f) / 8388608.0f);
}

bool bf_int_eligible(const BfIndexDev &ix) {
    if (ix.fmt != SCANN_HIP_ROWS_INT4) return false;
    if ((ix.stride & 31u) || (reinterpret_cast<uintptr_t>(ix.qrows) & 15u)) return false;   // 16-byte words of 32 nibbles
    switch (ix.dim) {
        case 32: case 64: case 96: case 128: case 192: case 256: return true;
        default: return false;
    }
}

size_t bf_int_digit_bytes(uint32_t nq, uint32_t dim) { return (size_t)kBfIntDigits * nq * dim; }
size_t bf_int_weight_bytes(uint32_t nq) { return (size_t)kBfIntDigits * nq * sizeof(float); }

// One wave per query.  The digits are taken in f64, where every residual q - s_1 d_1 - ... is exact to 2^-53: the only
// query error is the residual that is dropped.  A non-finite query gets digits 0 and a non-finite norm, which no
// verification passes.
template <int D>
__global__ __launch_bounds__(256) void bf_int_q_prep_kernel(const float *__restrict__ src, uint32_t nq, uint32_t dim,
                                                            uint32_t stride, float inv_mult, int8_t *__restrict__ digits,
                                                            float *__restrict__ weights, float *__restrict__ norm2,
                                                            float *__restrict__ q_err) {
    const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (q >= nq) return;
    const float *row = src + (size_t)q * stride;
    float s2 = 0.0f, qmax = 0.0f;
    for (uint32_t j = lane; j < dim; j += 64) {
        const float v = row[j];
        s2 = s2 + v * v;
        qmax = fmaxf(qmax, fabsf(v));
    }
    for (int o = 32; o > 0; o >>= 1) {
        s2 += __shfl_xor(s2, o);
        qmax = fmaxf(qmax, __shfl_xor(qmax, o));
    }
    double s[D];
    s[0] = qmax > 0.0f ? (double)qmax / 127.0 : 1.0 / 127.0;   // an all-zero query: scale 1
    for (int t = 1; t < D; ++t) s[t] = s[t - 1] / 254.0;
    double e2 = 0.0;
    for (uint32_t j = lane; j < dim; j += 64) {
        double r = (double)row[j];
        for (int t = 0; t < D; ++t) {
            double d = rint(r / s[t]);
            if (!(fabs(d) <= 127.0)) d = 0.0;   // NaN / inf elements
            digits[((size_t)t * nq + q) * dim + j] = (int8_t)(int)d;
            r = r - d * s[t];
        }
        e2 = e2 + r * r;
    }
    for (int o = 32; o > 0; o >>= 1) e2 += __shfl_xor(e2, o);
    if (lane == 0) {
        norm2[q] = s2 * 1.0000002f;   // an upper bound of |q|^2, as bf_q_prep_kernel
        q_err[q] = (float)(sqrt(e2) * 1.000001) * 1.0000002f;
        for (int t = 0; t < D; ++t) weights[(size_t)q * D + t] = (float)(s[t] * (double)inv_mult);
    }
}

// packed word of 8 nibbles (elements 8 w .. 8 w + 7) -> the codes nibble - 8 as two words of four int8.
// Per byte, (n | 0x80) - 8 never borrows from its neighbour and ^ 0x80 restores the top bit.
__device__ __forceinline__ void int4_word_to_i8(uint32_t w, uint32_t &lo4, uint32_t &hi4) {
    const uint32_t ev = (((w & 0x0F0F0F0Fu) | 0x80808080u) - 0x08080808u) ^ 0x80808080u;          // elements 0 2 4 6
    const uint32_t od = ((((w >> 4) & 0x0F0F0F0Fu) | 0x80808080u) - 0x08080808u) ^ 0x80808080u;   // elements 1 3 5 7
    lo4 = __builtin_amdgcn_perm(od, ev, 0x05010400u);   // ev0 od0 ev1 od1
    hi4 = __builtin_amdgcn_perm(od, ev, 0x07030602u);   // ev2 od2 ev3 od3
}

constexpr int kIntWaves = 4;   // waves per block, 32 queries each: 128 queries share a stage

// Block = 4 waves x 32 queries, the D x TS query fragments resident in registers.  A stage is RT rows of DIM int8 codes
// in LDS (RT = 128 up to dim 128, 64 above: a packed row is a quarter of the bf16 kernel's bytes, spent on four
// 32-row sub-tiles per barrier instead of one).  Two LDS stages and one stage in registers: the packed 16-byte words
// of stage i + 1 are loaded before the MFMAs of stage i, unpacked and written behind them; one barrier per stage.
// LDS layout: row r, 16-byte chunk c (16 elements) at r * DIM + 16 * (c ^ (r & SW)), the XOR swizzle of
// bf_bf16_kernel (SW + 1 = the largest power of two dividing the 2 TS chunks of a row, at most 16): the 32 rows a
// fragment read touches fall on distinct chunk columns.  v_mfma_i32_32x32x32_i8:
//   A[i = lane & 31][k = 16 h + j] = X[row i][32 t + 16 h + j],  B[k][n = lane & 31] = digit plane[n][32 t + 16 h + j].
template <int TS, int MEASURE, int FMT, int D>
__global__ __launch_bounds__(kIntWaves * 64, 2) void bf_i8mfma_kernel(BfIndexDev ix, BfPass p,
                                                                      const int8_t *__restrict__ qd,
                                                                      const float *__restrict__ qw,
                                                                      const float *__restrict__ qn2, uint32_t nx,
                                                                      uint32_t ny) {
    static_assert(FMT == SCANN_HIP_ROWS_INT4, "packed int4 rows; other integer-coded formats need a stash of their own");
    constexpr int DIM = TS * 32;
    constexpr int CPR = 2 * TS;                                        // 16-byte chunks of an unpacked row
    constexpr uint32_t SW = (CPR % 16 == 0) ? 15u : (CPR % 8 == 0 ? 7u : (CPR % 4 == 0 ? 3u : 1u));
    constexpr int RT = TS <= 4 ? 128 : 64;                             // rows per stage
    constexpr int UPC = 2;                                             // unpacked chunks per 16-byte word of the row
    constexpr int UPR = CPR / UPC;                                     // 16-byte words per stored row
    constexpr int UNITS = RT * UPR;
    constexpr int MYU = (UNITS + kIntWaves * 64 - 1) / (kIntWaves * 64);
    constexpr int STAGE_B = RT * DIM + RT * 4;                         // codes | squared norms
    extern __shared__ __attribute__((aligned(16))) unsigned char xs[];   // [2][STAGE_B]
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t h = lane >> 5, li = lane & 31u;
    const uint32_t bid = blockIdx.x, xcd = bid & 7u, slot = bid >> 3;
    const uint32_t x = xcd + 8u * (slot / ny), y = slot % ny;
    const uint32_t ntiles = (p.nrows + RT - 1u) / RT;
    uint32_t tile = x;
    if (tile >= ntiles) return;   // uniform per block
    const uint32_t q = y * (kIntWaves * 32u) + wave * 32u + li;
    const uint32_t qc = min(q, p.nq - 1u);
    const bool qvalid = q < p.nq;
    v4i qf[D][TS];
    float w[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
#pragma unroll
        for (int t = 0; t < TS; ++t)
            qf[d][t] = *reinterpret_cast<const v4i *>(qd + ((size_t)d * p.nq + qc) * DIM + 32 * t + 16 * h);
        w[d] = qw[(size_t)qc * D + d];
        if (MEASURE == SCANN_HIP_DOT_PRODUCT) w[d] = -w[d];   // the score is -dot
    }
    const float q2 = MEASURE == SCANN_HIP_DOT_PRODUCT ? 0.0f : qn2[qc];
    uint64_t T = 0;
    float Tf = 0.0f;
    if (p.filter) {
        T = p.thr[qc];
        Tf = bf_thr_float(T);
    }
    const size_t row_bytes = quant_row_bytes<FMT>(ix.stride);
    const unsigned char *rows = static_cast<const unsigned char *>(ix.qrows);
    uint4 pre[MYU];
    float pre_n = 0.0f;
    auto fetch = [&](uint32_t tl) {   // the stage's packed words and norms into registers (rows past the end: the last row)
#pragma unroll
        for (int i = 0; i < MYU; ++i) {
            const uint32_t u = tid + (uint32_t)(kIntWaves * 64) * i;
            if (u < (uint32_t)UNITS) {
                const uint32_t vr = min(tl * RT + u / UPR, p.nrows - 1u);
                pre[i] = *reinterpret_cast<const uint4 *>(rows + (size_t)vr * p.row_mult * row_bytes + 16u * (u % UPR));
            }
        }
        if (MEASURE != SCANN_HIP_DOT_PRODUCT && tid < (uint32_t)RT)
            pre_n = ix.norm2[(size_t)min(tl * RT + tid, p.nrows - 1u) * p.row_mult];
    };
    auto stash = [&](uint32_t buf) {   // registers -> LDS stage, unpacked and swizzled
        unsigned char *stage = xs + (size_t)buf * STAGE_B;
#pragma unroll
        for (int i = 0; i < MYU; ++i) {
            const uint32_t u = tid + (uint32_t)(kIntWaves * 64) * i;
            if (u < (uint32_t)UNITS) {
                const uint32_t r = u / UPR, c = (u % UPR) * UPC, sw = r & SW;
                uint32_t o[8];
                int4_word_to_i8(pre[i].x, o[0], o[1]);
                int4_word_to_i8(pre[i].y, o[2], o[3]);
                int4_word_to_i8(pre[i].z, o[4], o[5]);
                int4_word_to_i8(pre[i].w, o[6], o[7]);
                *reinterpret_cast<uint4 *>(stage + r * DIM + 16u * (c ^ sw)) = make_uint4(o[0], o[1], o[2], o[3]);
                *reinterpret_cast<uint4 *>(stage + r * DIM + 16u * ((c + 1u) ^ sw)) = make_uint4(o[4], o[5], o[6], o[7]);
            }
        }
        if (MEASURE != SCANN_HIP_DOT_PRODUCT && tid < (uint32_t)RT)
            reinterpret_cast<float *>(stage + RT * DIM)[tid] = pre_n;
    };
    fetch(tile);
    stash(0);
    __syncthreads();
    const uint32_t sw = li & SW;
    // survivors travel two iterations behind the scores, as in bf_bf16_kernel: the list slot of the one found in
    // iteration i - 1 is reserved at the top of iteration i and written at the top of iteration i + 1
    bool phas = false, fhas = false;
    uint64_t pkey = 0, fkey = 0;
    uint32_t fpos = 0;
    for (uint32_t it = 0; tile < ntiles; tile += nx, ++it) {
        const uint32_t buf = it & 1u;
        const bool more = tile + nx < ntiles;
        if (fhas && fpos < p.cap) p.cand[(size_t)q * p.cap + fpos] = fkey;
        fhas = phas;
        fkey = pkey;
        phas = false;
        if (fhas) fpos = atomicAdd(&p.cand_cnt[q], 1u);
        if (more) fetch(tile + nx);
        const unsigned char *stage = xs + (size_t)buf * STAGE_B;
#pragma unroll
        for (int sub = 0; sub < RT / 32; ++sub) {
            const uint32_t row0 = tile * RT + 32u * sub;
            if (row0 >= p.nrows) break;   // uniform
            const float *nrm = reinterpret_cast<const float *>(stage + RT * DIM) + 32 * sub;
            const unsigned char *xrow = stage + (size_t)(32 * sub + li) * DIM;
            v16i acc[D];
#pragma unroll
            for (int d = 0; d < D; ++d) acc[d] = v16i{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int t = 0; t < TS; ++t) {
                const v4i a = *reinterpret_cast<const v4i *>(xrow + 16u * ((2u * t + h) ^ sw));
#pragma unroll
                for (int d = 0; d < D; ++d) acc[d] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, qf[d][t], acc[d], 0, 0, 0);
            }
            float sc[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float dot = (float)acc[0][r] * w[0];   // |acc| <= 128 * 127 * 256 < 2^24: the conversion is exact
#pragma unroll
                for (int d = 1; d < D; ++d) dot = dot + (float)acc[d][r] * w[d];
                if (MEASURE == SCANN_HIP_DOT_PRODUCT) sc[r] = dot;   // the weights carry the sign
                else sc[r] = (q2 + nrm[(r & 3) + 8 * (r >> 2) + 4 * h]) - 2.0f * dot;
            }
            const bool full = row0 + 32u <= p.nrows;
            if (p.filter) {
                float dmin = sc[0];
#pragma unroll
                for (int r = 1; r < 16; ++r) dmin = fminf(dmin, sc[r]);
                if (__any(qvalid && (dmin <= Tf || !full))) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const uint32_t vrow = row0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                        if (qvalid && vrow < p.nrows && sc[r] <= Tf) {
                            const uint64_t key = make_key(sc[r], vrow * p.row_mult);
                            if (key <= T) {
                                if (!phas) {
                                    pkey = key;
                                    phas = true;
                                } else {   // a second survivor of this lane
                                    const uint32_t pos = atomicAdd(&p.cand_cnt[q], 1u);
                                    if (pos < p.cap) p.cand[(size_t)q * p.cap + pos] = key;
                                }
                            }
                        }
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint32_t vrow = row0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (qvalid && vrow < p.nrows) p.out[(size_t)q * p.ld + vrow] = sc[r];
                }
            }
        }
        if (more) stash(buf ^ 1u);   // every wave left that stage at the last barrier
        __syncthreads();
    }
    if (fhas && fpos < p.cap) p.cand[(size_t)q * p.cap + fpos] = fkey;
    if (phas) {
        const uint32_t pos = atomicAdd(&p.cand_cnt[q], 1u);
        if (pos < p.cap) p.cand[(size_t)q * p.cap + pos] = pkey;
    }
}

int bf_int_q_prep(const BfIndexDev &ix, const float *d_queries, uint32_t nq, uint32_t q_stride, int8_t *q_digits,
                  float *q_weights, float *q_n2, float *q_err, hipStream_t st) {
    return launch(bf_int_q_prep_kernel<kBfIntDigits>, dim3(ceil_div_u32(nq, 4)), dim3(256), 0, st, d_queries, nq, ix.dim,
                  q_stride, ix.inv_mult, q_digits, q_weights, q_n2, q_err);
}

template <int TS>
static int launch_i8mfma(const BfIndexDev &ix, const BfPass &p, const int8_t *qd, const float *qw, const float *qn2,
                         hipStream_t st) {
    constexpr uint32_t RT = TS <= 4 ? 128 : 64;
    const uint32_t ny = ceil_div_u32(p.nq, kIntWaves * 32);
    const uint32_t ntiles = ceil_div_u32(p.nrows, RT);
    uint32_t want = std::max<uint32_t>(1, (2u * (uint32_t)num_cus()) / ny);
    want = std::min(want, ntiles);
    const uint32_t nx = 8u * ceil_div_u32(want, 8);
    const size_t lds = (size_t)2 * (RT * TS * 32 + RT * 4);
    return with_value<SCANN_HIP_DOT_PRODUCT, SCANN_HIP_SQUARED_L2>(ix.measure, [&](auto m) {
        return launch((bf_i8mfma_kernel<TS, m(), SCANN_HIP_ROWS_INT4, kBfIntDigits>), dim3(nx * ny), dim3(kIntWaves * 64),
                      lds, st, ix, p, qd, qw, qn2, nx, ny);
    });
}

int bf_int_pass(const BfIndexDev &ix, const BfPass &p, const int8_t *q_digits, const float *q_weights,
                const float *q_n2, hipStream_t st) {
    if (!bf_int_eligible(ix)) return fail(SCANN_HIP_INTERNAL, "integer shortlist pass on rows it cannot read");
    if (p.nq == 0 || p.nrows == 0) return SCANN_HIP_OK;
    return with_value<1, 2, 3, 4, 6, 8>((int)(ix.dim / 32), [&](auto ts) {
        return launch_i8mfma<ts()>(ix, p, q_digits, q_weights, q_n2, st);
    });
}

}  // namespace scann

// bf.hip -- batched brute force (BruteForceSearcher::search_batched,
// brute_force/searcher.rs:77-208) for gfx950.
//
// The reference computes, per (query, row), one_to_many_{squared_l2,dot_product}_avx2
// (simd/x86.rs:195-346): 8 independent FMA lane chains over 8-float chunks, a fixed
// horizontal-sum tree (x86.rs:31-44), a non-fused scalar tail, and then pushes every row
// into a TopK heap (top_k.rs:66-81) whose survivors are the k lexicographically smallest
// (distance, index) pairs.
//
//  * DotProduct, dim % 16 == 0: f32 MFMA (v_mfma_f32_32x32x2_f32).  Each MFMA result is a
//    k-ordered fmaf chain, so feeding chain j with k = j, 8+j, 16+j, ... reproduces AVX2
//    lane j exactly; the 8 chains are 8 accumulator tiles combined by the hsum tree.
//    Distances are therefore bit-identical to the CPU path.
//  * SquaredL2 / L2 / other dims: VALU kernel with the same 8-chain arithmetic.
//  * top-k: a strided row sample gives a valid upper bound of the k-th best key; the full
//    pass keeps only (distance, index) keys <= bound; a per-query LDS sort finishes.
#include "bf.h"
#include "launch.h"
#include "quant.h"

#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace scann {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr uint32_t kBfSortCap = 8192;
constexpr uint32_t kBfMaxK = 2048;
constexpr uint32_t kBfSelectThreads = 1024;
constexpr uint32_t kBfInvalid = 0xFFFFFFFFu;

enum { BF_CNT_STATUS = 0, BF_CNT_N = 4 };

struct BfPass {
    const float *queries;   // device [nq][q_stride]
    uint32_t nq, q_stride;
    uint32_t nrows;         // virtual rows of this pass
    uint32_t row_mult;      // real row = virtual row * row_mult
    int filter;             // 0: store all to out[nq][ld]; 1: threshold filter -> candidates
    float *out;
    uint32_t ld;
    const uint64_t *thr;    // [nq]
    uint32_t *cand_cnt;     // [nq]
    uint64_t *cand;         // [nq][cap]
    uint32_t cap;
    // allow-list filter (scann_hip_search_opts.allow_bitmap); both null on an unfiltered search.
    const uint32_t *ids;    // compacted form: real row = ids[virtual row * row_mult], ascending allowed datapoints
    const uint64_t *allow;  // bit-test form: a row is a candidate only if its bit is set (tested at the emit)
    uint32_t allow_bits;    // capacity of the bitmap clipped to the row count
};

// datapoint index of a virtual row (the row that is read, and the index half of its key)
__device__ __forceinline__ uint32_t bf_real_row(const BfPass &p, uint32_t vrow) {
    const uint32_t r = vrow * p.row_mult;
    return p.ids ? p.ids[r] : r;
}

// RestrictFilter::is_allowed (restricts/mod.rs:17-30) on the bitmap form: indices at or past the capacity are
// not allowed (allowlist.rs:97-100).
__device__ __forceinline__ bool bf_row_allowed(const uint64_t *allow, uint32_t allow_bits, uint32_t row) {
    return row < allow_bits && ((allow[row >> 6] >> (row & 63u)) & 1ull);
}

__device__ __forceinline__ void bf_emit(const BfPass &p, uint32_t q, uint32_t vrow, float dist,
                                        float Tf, uint64_t T) {
    if (!p.filter) {
        p.out[(size_t)q * p.ld + vrow] = dist;
    } else if (dist <= Tf) {
        const uint32_t row = bf_real_row(p, vrow);
        if (p.allow && !bf_row_allowed(p.allow, p.allow_bits, row)) return;   // skipped before scoring: mod.rs:327-332
        const uint64_t key = make_key(dist, row);
        if (key <= T) {
            const uint32_t pos = atomicAdd(&p.cand_cnt[q], 1u);
            if (pos < p.cap) p.cand[(size_t)q * p.cap + pos] = key;
        }
    }
}

__device__ __forceinline__ float bf_thr_float(uint64_t T) {
    const uint32_t hi = (uint32_t)(T >> 32);
    return hi == 0xFFFFFFFFu ? __builtin_inff() : ordered_to_f32(hi);
}

// =====================================================================================
// Generic VALU kernel: any dim, all three measures; one row per thread, QT queries from
// LDS.  Arithmetic = simd/x86.rs:139-165 / :72-96 lane for lane.
// =====================================================================================
constexpr int kBfGenQT = 8;

// wide 0.7 f32x8::reduce_add in a build without target_feature = "avx" (the reference has no RUSTFLAGS):
// two f32x4 halves, each summed sequentially -- the horizontal sum of cosine_similarity_f32_simd
// (one_to_one.rs:559-604).  Third-party order, restated; see scann_hip.h.
__device__ __forceinline__ float wide07_reduce_add(const float (&v)[8]) {
    const float lo = ((v[0] + v[1]) + v[2]) + v[3];
    const float hi = ((v[4] + v[5]) + v[6]) + v[7];
    return lo + hi;
}

template <int MEASURE>
__global__ __launch_bounds__(256) void bf_generic_kernel(BfIndexDev ix, BfPass p) {
    extern __shared__ __attribute__((aligned(16))) float qs[];  // [kBfGenQT][dimp] (+ [kBfGenQT] query norms)
    const uint32_t dim = ix.dim, dimp = (dim + 3u) & ~3u;
    const uint32_t q0 = blockIdx.y * kBfGenQT;
    for (uint32_t i = threadIdx.x; i < kBfGenQT * dimp; i += blockDim.x) {
        uint32_t qi = i / dimp, j = i - qi * dimp;
        qs[i] = (q0 + qi < p.nq && j < dim) ? p.queries[(size_t)(q0 + qi) * p.q_stride + j] : 0.0f;
    }
    __syncthreads();
    const uint32_t chunks = dim >> 3;
    float *s_qn = qs + kBfGenQT * dimp;   // Cosine: sum of squares of every query, in the pair kernel's order
    if (MEASURE == SCANN_HIP_COSINE) {
        if (threadIdx.x < (uint32_t)kBfGenQT) {
            const float *qv = qs + threadIdx.x * dimp;
            float aa[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            for (uint32_t c = 0; c < chunks; ++c)
#pragma unroll
                for (int j = 0; j < 8; ++j) aa[j] = aa[j] + qv[8 * c + j] * qv[8 * c + j];
            float saa = wide07_reduce_add(aa);
            for (uint32_t j = chunks * 8; j < dim; ++j) saa = saa + qv[j] * qv[j];
            s_qn[threadIdx.x] = saa;
        }
        __syncthreads();
    }
    const uint32_t vrow = blockIdx.x * blockDim.x + threadIdx.x;
    if (vrow >= p.nrows) return;
    const float *row = ix.rows + (size_t)bf_real_row(p, vrow) * ix.stride;
    // The 8 AVX2 lane chains of a (query, row) pair are independent accumulators: pairs of
    // them go through the packed-f32 pipe (v_pk_add_f32 / v_pk_fma_f32: two IEEE operations per
    // instruction, same results as the scalar ones).
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    f32x2 accv[kBfGenQT][4];
    f32x2 bbv[4] = {f32x2{0.0f, 0.0f}, f32x2{0.0f, 0.0f}, f32x2{0.0f, 0.0f}, f32x2{0.0f, 0.0f}};   // Cosine: row norm chains
#pragma unroll
    for (int qi = 0; qi < kBfGenQT; ++qi)
#pragma unroll
        for (int j = 0; j < 4; ++j) accv[qi][j] = f32x2{0.0f, 0.0f};
    const bool vec = ((ix.stride & 3u) == 0) && ((reinterpret_cast<uintptr_t>(ix.rows) & 15u) == 0);
    for (uint32_t c = 0; c < chunks; ++c) {
        f32x2 x[4];
        if (vec) {
            const float4 a = *reinterpret_cast<const float4 *>(row + 8 * c);
            const float4 b = *reinterpret_cast<const float4 *>(row + 8 * c + 4);
            x[0] = f32x2{a.x, a.y}; x[1] = f32x2{a.z, a.w};
            x[2] = f32x2{b.x, b.y}; x[3] = f32x2{b.z, b.w};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = f32x2{row[8 * c + 2 * j], row[8 * c + 2 * j + 1]};
        }
        if (MEASURE == SCANN_HIP_COSINE)
#pragma unroll
            for (int j = 0; j < 4; ++j) bbv[j] = bbv[j] + x[j] * x[j];   // add(mul): not fused
#pragma unroll
        for (int qi = 0; qi < kBfGenQT; ++qi) {
            const float4 qa = *reinterpret_cast<const float4 *>(qs + qi * dimp + 8 * c);
            const float4 qb = *reinterpret_cast<const float4 *>(qs + qi * dimp + 8 * c + 4);
            const f32x2 qv[4] = {f32x2{qa.x, qa.y}, f32x2{qa.z, qa.w}, f32x2{qb.x, qb.y},
                                 f32x2{qb.z, qb.w}};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (MEASURE == SCANN_HIP_DOT_PRODUCT) {
                    accv[qi][j] = __builtin_elementwise_fma(qv[j], x[j], accv[qi][j]);
                } else if (MEASURE == SCANN_HIP_L1) {          // _mm256_add_ps(sum, andnot(sign, a - b))
                    accv[qi][j] = accv[qi][j] + __builtin_elementwise_abs(qv[j] - x[j]);
                } else if (MEASURE == SCANN_HIP_COSINE) {      // dot_ab.add(va.mul(vb)): two roundings
                    accv[qi][j] = accv[qi][j] + qv[j] * x[j];
                } else {
                    const f32x2 d = qv[j] - x[j];
                    accv[qi][j] = __builtin_elementwise_fma(d, d, accv[qi][j]);
                }
            }
        }
    }
    float acc[kBfGenQT][8];
#pragma unroll
    for (int qi = 0; qi < kBfGenQT; ++qi)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[qi][2 * j] = accv[qi][j].x;
            acc[qi][2 * j + 1] = accv[qi][j].y;
        }
    float sbb = 0.0f;
    if (MEASURE == SCANN_HIP_COSINE) {
        const float bb[8] = {bbv[0].x, bbv[0].y, bbv[1].x, bbv[1].y, bbv[2].x, bbv[2].y, bbv[3].x, bbv[3].y};
        sbb = wide07_reduce_add(bb);
        for (uint32_t j = chunks * 8; j < dim; ++j) sbb = sbb + row[j] * row[j];
    }
#pragma unroll
    for (int qi = 0; qi < kBfGenQT; ++qi) {
        if (q0 + qi >= p.nq) continue;
        float r;
        if (MEASURE == SCANN_HIP_COSINE) {
            r = wide07_reduce_add(acc[qi]);
        } else {   // horizontal_sum_f32_avx2 (x86.rs:31-44)
            const float s0 = acc[qi][0] + acc[qi][4], s1 = acc[qi][1] + acc[qi][5];
            const float s2 = acc[qi][2] + acc[qi][6], s3 = acc[qi][3] + acc[qi][7];
            r = (s0 + s1) + (s2 + s3);
        }
        for (uint32_t j = chunks * 8; j < dim; ++j) {
            const float qv = qs[qi * dimp + j];
            if (MEASURE == SCANN_HIP_DOT_PRODUCT || MEASURE == SCANN_HIP_COSINE) {
                r = r + qv * row[j];
            } else if (MEASURE == SCANN_HIP_L1) {
                r = r + fabsf(qv - row[j]);
            } else {
                const float d = qv - row[j];
                r = r + d * d;
            }
        }
        float dist = r;
        if (MEASURE == SCANN_HIP_DOT_PRODUCT) dist = -r;
        if (MEASURE == SCANN_HIP_L2) dist = sqrtf(r);
        if (MEASURE == SCANN_HIP_COSINE) {   // one_to_one.rs:596-612
            const float na = sqrtf(s_qn[qi]), nb = sqrtf(sbb);
            const float sim = (na == 0.0f || nb == 0.0f) ? 0.0f : r / (na * nb);
            dist = 1.0f - sim;
        }
        uint64_t T = 0;
        float Tf = 0.0f;
        if (p.filter) {
            T = p.thr[q0 + qi];
            Tf = bf_thr_float(T);
        }
        bf_emit(p, q0 + qi, vrow, dist, Tf, T);
    }
}

// =====================================================================================
// Streaming kernel for SMALL batches (a handful of queries: the single-query search of
// BruteForceSearcher::search): the pass is one read of the database, so it must run at HBM
// speed.  A row-per-lane global read (bf_generic_kernel) touches 64 cache lines per instruction;
// here each WAVE stages 64 rows x 32 dims through its own LDS slice with fully coalesced 16-byte
// loads (8 lanes per 128-byte row segment), the next slice's loads already in flight, and every
// lane then reads ITS row back (pitch 36 floats: conflict-free ds_read_b128).  No workgroup
// barrier in the loop: a wave's LDS operations execute in order.  Arithmetic as bf_generic_kernel.
// =====================================================================================
constexpr int kStQT = 8;              // queries per database pass
constexpr uint32_t kStDims = 32;      // dims per staged slice
constexpr uint32_t kStLd = kStDims + 4;

template <int MEASURE>
__global__ __launch_bounds__(256) void bf_stream_kernel(BfIndexDev ix, BfPass p) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) float qs[];   // [kStQT][dimp] | [4 waves][64][kStLd]
    const uint32_t dim = ix.dim, dimp = (dim + 3u) & ~3u, chunks = dim >> 3, cdim = chunks * 8;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t q0 = blockIdx.y * kStQT;
    for (uint32_t i = tid; i < kStQT * dimp; i += 256) {
        const uint32_t qi = i / dimp, j = i - qi * dimp;
        qs[i] = (q0 + qi < p.nq && j < dim) ? p.queries[(size_t)(q0 + qi) * p.q_stride + j] : 0.0f;
    }
    __syncthreads();
    float *xw = qs + kStQT * dimp + wave * 64 * kStLd;
    const uint32_t ngroups = (p.nrows + 63u) / 64u;
    const uint32_t part = lane & 7u, rsub = lane >> 3;   // staging: 8 lanes per row segment, 8 rows per load
    for (uint32_t g = blockIdx.x * 4u + wave; g < ngroups; g += gridDim.x * 4u) {
        const uint32_t vrow0 = g * 64u;
        // this lane's 8 staging pieces: row rsub + 8 i, 16 bytes at float offset part * 4 of the slice
        const float *src[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
            src[i] = ix.rows + (size_t)bf_real_row(p, min(vrow0 + rsub + 8u * i, p.nrows - 1u)) * ix.stride;
        float4 s0, s1, s2, s3, s4, s5, s6, s7;
        // lanes past a short last slice re-read its last piece (never stored)
#define SCANN_ST_FETCH(d0_)                                                                  \
    do {                                                                                       \
        const uint32_t o_ = (d0_) + min(part * 4u, min(kStDims, cdim - (d0_)) - 4u);           \
        s0 = *reinterpret_cast<const float4 *>(src[0] + o_);                                   \
        s1 = *reinterpret_cast<const float4 *>(src[1] + o_);                                   \
        s2 = *reinterpret_cast<const float4 *>(src[2] + o_);                                   \
        s3 = *reinterpret_cast<const float4 *>(src[3] + o_);                                   \
        s4 = *reinterpret_cast<const float4 *>(src[4] + o_);                                   \
        s5 = *reinterpret_cast<const float4 *>(src[5] + o_);                                   \
        s6 = *reinterpret_cast<const float4 *>(src[6] + o_);                                   \
        s7 = *reinterpret_cast<const float4 *>(src[7] + o_);                                   \
    } while (0)
#define SCANN_ST_COMMIT(d0_)                                                                 \
    do {                                                                                       \
        if (part * 4u < min(kStDims, cdim - (d0_))) {                                          \
            float *dst_ = xw + rsub * kStLd + part * 4u;                                       \
            *reinterpret_cast<float4 *>(dst_ + 0 * 8 * kStLd) = s0;                            \
            *reinterpret_cast<float4 *>(dst_ + 1 * 8 * kStLd) = s1;                            \
            *reinterpret_cast<float4 *>(dst_ + 2 * 8 * kStLd) = s2;                            \
            *reinterpret_cast<float4 *>(dst_ + 3 * 8 * kStLd) = s3;                            \
            *reinterpret_cast<float4 *>(dst_ + 4 * 8 * kStLd) = s4;                            \
            *reinterpret_cast<float4 *>(dst_ + 5 * 8 * kStLd) = s5;                            \
            *reinterpret_cast<float4 *>(dst_ + 6 * 8 * kStLd) = s6;                            \
            *reinterpret_cast<float4 *>(dst_ + 7 * 8 * kStLd) = s7;                            \
        }                                                                                      \
    } while (0)
        f32x2 accv[kStQT][4];
#pragma unroll
        for (int qi = 0; qi < kStQT; ++qi)
#pragma unroll
            for (int u = 0; u < 4; ++u) accv[qi][u] = f32x2{0.0f, 0.0f};
        if (cdim) SCANN_ST_FETCH(0u);
        for (uint32_t d0 = 0; d0 < cdim; d0 += kStDims) {
            const uint32_t nd = min(kStDims, cdim - d0);
            SCANN_ST_COMMIT(d0);
            if (d0 + kStDims < cdim) SCANN_ST_FETCH(d0 + kStDims);   // in flight during the compute
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const float *xr = xw + lane * kStLd;
            for (uint32_t c = 0; c < nd; c += 8) {
                const float4 xa = *reinterpret_cast<const float4 *>(xr + c);
                const float4 xb = *reinterpret_cast<const float4 *>(xr + c + 4);
                const f32x2 x[4] = {f32x2{xa.x, xa.y}, f32x2{xa.z, xa.w}, f32x2{xb.x, xb.y}, f32x2{xb.z, xb.w}};
#pragma unroll
                for (int qi = 0; qi < kStQT; ++qi) {
                    const float4 qa = *reinterpret_cast<const float4 *>(qs + qi * dimp + d0 + c);
                    const float4 qb = *reinterpret_cast<const float4 *>(qs + qi * dimp + d0 + c + 4);
                    const f32x2 qv[4] = {f32x2{qa.x, qa.y}, f32x2{qa.z, qa.w}, f32x2{qb.x, qb.y},
                                         f32x2{qb.z, qb.w}};
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (MEASURE == SCANN_HIP_DOT_PRODUCT) {
                            accv[qi][u] = __builtin_elementwise_fma(qv[u], x[u], accv[qi][u]);
                        } else {
                            const f32x2 d = qv[u] - x[u];
                            accv[qi][u] = __builtin_elementwise_fma(d, d, accv[qi][u]);
                        }
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();                     // reads done before the next commit
        }
        const uint32_t vrow = vrow0 + lane;
        if (vrow < p.nrows) {
            const float *row = ix.rows + (size_t)bf_real_row(p, vrow) * ix.stride;
#pragma unroll
            for (int qi = 0; qi < kStQT; ++qi) {
                if (q0 + qi >= p.nq) continue;
                const f32x2 s01 = accv[qi][0] + accv[qi][2], s23 = accv[qi][1] + accv[qi][3];
                float r = (s01.x + s01.y) + (s23.x + s23.y);   // hsum tree, x86.rs:31-44
                for (uint32_t j = cdim; j < dim; ++j) {         // scalar tail, not fused
                    const float qv = qs[qi * dimp + j];
                    if (MEASURE == SCANN_HIP_DOT_PRODUCT) {
                        r = r + qv * row[j];
                    } else {
                        const float d = qv - row[j];
                        r = r + d * d;
                    }
                }
                float dist = r;
                if (MEASURE == SCANN_HIP_DOT_PRODUCT) dist = -r;
                if (MEASURE == SCANN_HIP_L2) dist = sqrtf(r);
                uint64_t T = 0;
                float Tf = 0.0f;
                if (p.filter) {
                    T = p.thr[q0 + qi];
                    Tf = bf_thr_float(T);
                }
                bf_emit(p, q0 + qi, vrow, dist, Tf, T);
            }
        }
    }
#undef SCANN_ST_FETCH
#undef SCANN_ST_COMMIT
}

// =====================================================================================
// SquaredL2 / L2 kernel with one QUERY per lane (dim = 8 * DC <= 128).  (q - x)^2 cannot go
// through MFMA bit-exactly, so this is the VALU roofline: a lane keeps its whole query in
// registers (DC * 4 packed pairs), a block of 4 waves (256 queries) shares 32-row tiles of
// the database staged in LDS, and every row value is a wave-uniform LDS broadcast read.  Per
// (row, 8 dims, 64 queries): 2 ds_read_b128 + 4 v_pk_add_f32 + 4 v_pk_fma_f32 -- the 8 AVX2
// lane chains of simd/x86.rs:139-165 as 4 packed accumulators, combined by the same hsum tree.
// (Feeding the rows through the scalar cache as SGPR operands instead was slower: a row needs
// 128 SGPRs, so nothing can be prefetched while the previous row computes.)
// =====================================================================================
constexpr int kVqRows = 32;   // rows per LDS tile

template <int MEASURE, int DC>
__global__ __launch_bounds__(256, 2) void bf_vq_kernel(BfIndexDev ix, BfPass p, uint32_t nx) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    constexpr int DIM = DC * 8;
    constexpr int LD4 = kVqRows * DIM / 4 / 256;                  // float4 staged per thread
    __shared__ __attribute__((aligned(16))) float tile[2][kVqRows * DIM];
    const uint32_t tid = threadIdx.x;
    const uint32_t bx = blockIdx.x % nx, by = blockIdx.x / nx;
    const uint32_t q = by * 256 + tid;
    const bool qok = q < p.nq;
    f32x2 qv[DC * 4];
    {
        const float *qrow = p.queries + (size_t)(qok ? q : 0) * p.q_stride;
#pragma unroll
        for (int i = 0; i < DC * 4; ++i) qv[i] = qok ? f32x2{qrow[2 * i], qrow[2 * i + 1]} : f32x2{0.0f, 0.0f};
    }
    uint64_t T = 0;
    float Tf = 0.0f, Tpre = __builtin_inff();
    if (p.filter && qok) {
        T = p.thr[q];
        Tf = bf_thr_float(T);
        // L2: sqrt only for distances that can pass the bound (sqrt is monotone; the margin
        // covers its rounding, the exact test on the rooted value follows in bf_emit)
        Tpre = MEASURE == SCANN_HIP_L2 ? Tf * Tf * 1.000001f + 1e-30f : Tf;
    }
    const uint32_t ntiles = (p.nrows + kVqRows - 1) / kVqRows;
    float4 stage[LD4];
    auto fetch = [&](uint32_t t) {
#pragma unroll
        for (int i = 0; i < LD4; ++i) {
            const uint32_t e = (tid + i * 256) * 4;              // float index inside the tile
            const uint32_t r = e / DIM, j = e - r * DIM;
            const uint32_t vrow = t * kVqRows + r;
            stage[i] = vrow < p.nrows
                           ? *reinterpret_cast<const float4 *>(ix.rows + (size_t)bf_real_row(p, vrow) * ix.stride + j)
                           : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    };
    auto commit = [&](uint32_t buf) {
#pragma unroll
        for (int i = 0; i < LD4; ++i) *reinterpret_cast<float4 *>(&tile[buf][(tid + i * 256) * 4]) = stage[i];
    };
    uint32_t t = bx;
    if (t < ntiles) {
        fetch(t);
        commit(0);
    }
    __syncthreads();
    for (uint32_t it = 0; t < ntiles; t += nx, ++it) {
        const uint32_t buf = it & 1u;
        const bool more = t + nx < ntiles;
        if (more) fetch(t + nx);                                  // in flight during the compute
        const float *tl = tile[buf];
        // one row at a time (a real loop: 4 packed accumulators live), its chunks software-
        // pipelined one deep; sched_barrier pins the order so the scheduler cannot hoist all of a
        // row's broadcast reads on top of the 128-VGPR resident query
#pragma unroll 1
        for (int r = 0; r < kVqRows; ++r) {
            const float *xr = tl + r * DIM;                      // wave-uniform: LDS broadcast reads
            f32x2 acc[4] = {f32x2{0.0f, 0.0f}, f32x2{0.0f, 0.0f}, f32x2{0.0f, 0.0f}, f32x2{0.0f, 0.0f}};
            float4 xa[2], xb[2];
            xa[0] = *reinterpret_cast<const float4 *>(xr);
            xb[0] = *reinterpret_cast<const float4 *>(xr + 4);
#pragma unroll
            for (int c = 0; c < DC; ++c) {
                if (c + 1 < DC) {
                    xa[(c + 1) & 1] = *reinterpret_cast<const float4 *>(xr + 8 * (c + 1));
                    xb[(c + 1) & 1] = *reinterpret_cast<const float4 *>(xr + 8 * (c + 1) + 4);
                }
                const float4 ca = xa[c & 1], cb = xb[c & 1];
                const f32x2 x[4] = {f32x2{ca.x, ca.y}, f32x2{ca.z, ca.w}, f32x2{cb.x, cb.y}, f32x2{cb.z, cb.w}};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x2 d = qv[4 * c + j] - x[j];
                    acc[j] = __builtin_elementwise_fma(d, d, acc[j]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            // hsum tree (x86.rs:31-44): (a0+a4, a1+a5), (a2+a6, a3+a7) -> (s0+s1) + (s2+s3)
            const f32x2 s01 = acc[0] + acc[2], s23 = acc[1] + acc[3];
            const float v = (s01.x + s01.y) + (s23.x + s23.y);
            const uint32_t vrow = t * kVqRows + r;
            if (qok && vrow < p.nrows && (!p.filter || v <= Tpre)) {
                const float dist = MEASURE == SCANN_HIP_L2 ? sqrtf(v) : v;
                bf_emit(p, q, vrow, dist, Tf, T);
            }
        }
        if (more) commit(buf ^ 1u);
        __syncthreads();
    }
}

// =====================================================================================
// MFMA kernel: DotProduct, dim = 16 * TS (dim % 32 == 0).  Block = 4 waves; wave w owns
// 32 queries (Q fragments resident in VGPRs); all waves share a 32-row X tile that is
// DMA'd global -> LDS (global_load_lds_dwordx4, no VGPR staging), double-buffered.  The
// LDS image is linear (DMA writes wave-base + lane*16); bank conflicts of the
// row-per-lane ds_read_b128 are removed by XOR-swizzling the 16-B chunk index with the
// row number on the SOURCE address and again on the read.  Two blocks per CU
// (<= 256 VGPR+AGPR) so one block's epilogue overlaps the other's MFMAs.
// Operand maps (v_mfma_f32_32x32x2_f32):
//   A[i = lane & 31][k = lane >> 5] = X[row i][16t + 8h + j]
//   B[k = lane >> 5][n = lane & 31] = Q[query n][16t + 8h + j]
//   D[row = (r&3) + 8*(r>>2) + 4h][col = lane & 31]
// Chain j accumulates k = j, 8+j, 16+j, ... in ascending order == AVX2 lane j.
// =====================================================================================
template <int TS>
__global__ __launch_bounds__(256, 2) void bf_mfma_dot_kernel(BfIndexDev ix, BfPass p, uint32_t nx,
                                                             uint32_t ny) {
    constexpr int DIM = TS * 16;
    constexpr int CPR = DIM / 4;                       // 16-B chunks per row
    constexpr uint32_t SW = (CPR % 16 == 0) ? 15u : 7u; // swizzle mask (CPR % 8 == 0)
    constexpr int TILE_F = 32 * DIM;                   // floats per tile
    constexpr int DMA_PER_WAVE = DIM / 32;             // 1 KiB wave-instructions per wave
    static_assert(TS % 2 == 0, "dim must be a multiple of 32");
    extern __shared__ __attribute__((aligned(16))) float xs[];   // [2][32][DIM]

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t h = lane >> 5, li = lane & 31u;
    // XCD-aware mapping: blocks that share an X tile (same x, all y) sit on one XCD.
    const uint32_t bid = blockIdx.x, xcd = bid & 7u, slot = bid >> 3;
    const uint32_t x = xcd + 8u * (slot / ny), y = slot % ny;
    const uint32_t ntiles = (p.nrows + 31u) / 32u;

    // resident query fragments
    const uint32_t q = y * 128u + wave * 32u + li;
    const uint32_t qc = min(q, p.nq - 1u);
    float qf[TS * 8];
    {
        const float *qrow = p.queries + (size_t)qc * p.q_stride;
#pragma unroll
        for (int t = 0; t < TS; ++t)
#pragma unroll
            for (int j = 0; j < 8; ++j) qf[t * 8 + j] = qrow[16 * t + 8 * h + j];
    }
    uint64_t T = 0;
    float Tf = 0.0f;
    if (p.filter) {
        T = p.thr[qc];
        Tf = bf_thr_float(T);
    }
    const bool qvalid = q < p.nq;

    auto dma_tile = [&](uint32_t tile, uint32_t buf) {
#pragma unroll
        for (int t = 0; t < DMA_PER_WAVE; ++t) {
            const uint32_t gi = wave * DMA_PER_WAVE + t;          // wave-uniform
            const uint32_t ci = gi * 64u + lane;                  // linear chunk index in the tile
            const uint32_t r = ci / CPR, pos = ci - r * CPR;
            const uint32_t vr = min(tile * 32u + r, p.nrows - 1u);
            const float *src = ix.rows + (size_t)bf_real_row(p, vr) * ix.stride + 4u * (pos ^ (r & SW));
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void *)src,
                (__attribute__((address_space(3))) void *)(xs + (size_t)buf * TILE_F + gi * 256u), 16, 0, 0);
        }
    };

    uint32_t tile = x;
    if (tile >= ntiles) return;   // uniform per block
    dma_tile(tile, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    uint32_t buf = 0;
    const f32x16 zero = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f,
                         0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const uint32_t sw = li & SW;
    for (; tile < ntiles; tile += nx) {
        const uint32_t next = tile + nx;
        if (next < ntiles) dma_tile(next, buf ^ 1u);

        f32x16 acc[8];
        const float *xrow = xs + (size_t)buf * TILE_F + li * DIM;
#pragma unroll
        for (int t = 0; t < TS; ++t) {
            const uint32_t c0 = 4u * t + 2u * h;
            const float4 a0 = *reinterpret_cast<const float4 *>(xrow + 4u * (c0 ^ sw));
            const float4 a1 = *reinterpret_cast<const float4 *>(xrow + 4u * ((c0 + 1u) ^ sw));
            const float xa[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
            for (int j = 0; j < 8; ++j)
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[j], qf[t * 8 + j], t == 0 ? zero : acc[j],
                                                              0, 0, 0);
        }
        // epilogue: horizontal_sum_f32_avx2 tree, negate
        float dist[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float s0 = acc[0][r] + acc[4][r], s1 = acc[1][r] + acc[5][r];
            const float s2 = acc[2][r] + acc[6][r], s3 = acc[3][r] + acc[7][r];
            dist[r] = -((s0 + s1) + (s2 + s3));
        }
        const bool full = tile * 32u + 32u <= p.nrows;
        if (p.filter) {
            // one wave-level test per tile; survivors are rare
            float dmin = dist[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) dmin = fminf(dmin, dist[r]);
            if (__any(qvalid && (dmin <= Tf || !full))) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint32_t vrow = tile * 32u + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (qvalid && vrow < p.nrows) bf_emit(p, q, vrow, dist[r], Tf, T);
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t vrow = tile * 32u + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (qvalid && (full || vrow < p.nrows)) p.out[(size_t)q * p.ld + vrow] = dist[r];
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // next tile's DMA has landed
        __syncthreads();
        buf ^= 1u;
    }
}

// =====================================================================================
// Nearest centre of every row (k-means assignment / residual partitioning).
// TreePartitioner::partition(x, 1) (partitioning/tree_partitioner.rs:175-229) as called by
// TreeXHybridSearcher::compute_residuals (tree_x_hybrid/mod.rs:212-237) and, with the same
// arithmetic, KMeans::assign_clusters (trees/kmeans.rs:352-379): strictly sequential scalar
// sum of (x_j - c_j)^2, argmin with the lowest index on ties (stable sort / strict '<').
// One thread per row; centres are staged in LDS tiles and read as broadcasts.
// =====================================================================================
constexpr int kAsgTC = 16;   // centres per LDS tile
constexpr int kAsgTCWide = 8;   // ... when 16 rows of dimp floats exceed the LDS (dim > 2560): reaches dim 5120
constexpr int kAsgDJ = 32;   // row values held in registers at a time

template <int TC>
__global__ __launch_bounds__(256) void assign_nearest_kernel(BfIndexDev ix, const float *__restrict__ centers,
                                                             uint32_t k, uint32_t *__restrict__ out_idx,
                                                             float *__restrict__ out_dist) {
    extern __shared__ __attribute__((aligned(16))) float cs[];   // [TC][dimp]
    const uint32_t dim = ix.dim, dimp = (dim + 3u) & ~3u;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = i < ix.n;
    const float *row = ix.rows + (act ? i : 0) * ix.stride;
    const bool vec = ((ix.stride & 3u) == 0) && ((reinterpret_cast<uintptr_t>(ix.rows) & 15u) == 0);
    float best = __builtin_inff();
    uint32_t bi = 0;
    for (uint32_t c0 = 0; c0 < k; c0 += TC) {
        for (uint32_t e = threadIdx.x; e < TC * dimp; e += blockDim.x) {
            const uint32_t c = e / dimp, j = e - c * dimp;
            cs[e] = (c0 + c < k && j < dim) ? centers[(size_t)(c0 + c) * dim + j] : 0.0f;
        }
        __syncthreads();
        float acc[TC];
#pragma unroll
        for (int c = 0; c < TC; ++c) acc[c] = 0.0f;
        for (uint32_t j0 = 0; j0 < dim; j0 += kAsgDJ) {
            float x[kAsgDJ];
            if (vec && j0 + kAsgDJ <= dim) {
#pragma unroll
                for (int j = 0; j < kAsgDJ; j += 4) {
                    const float4 v = *reinterpret_cast<const float4 *>(row + j0 + j);
                    x[j] = v.x; x[j + 1] = v.y; x[j + 2] = v.z; x[j + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < kAsgDJ; ++j) x[j] = (j0 + j < dim) ? row[j0 + j] : 0.0f;
            }
            const uint32_t nj = min((uint32_t)kAsgDJ, dim - j0);
#pragma unroll
            for (int c = 0; c < TC; ++c) {
                const float *cr = cs + c * dimp + j0;
                float a = acc[c];
                if (nj == (uint32_t)kAsgDJ) {
#pragma unroll
                    for (int j = 0; j < kAsgDJ; ++j) {
                        const float d = x[j] - cr[j];
                        a = a + d * d;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < kAsgDJ; ++j)
                        if ((uint32_t)j < nj) {
                            const float d = x[j] - cr[j];
                            a = a + d * d;
                        }
                }
                acc[c] = a;
            }
        }
#pragma unroll
        for (int c = 0; c < TC; ++c)
            if (c0 + c < k && acc[c] < best) {
                best = acc[c];
                bi = c0 + c;
            }
        __syncthreads();
    }
    if (act) {
        out_idx[i] = bi;
        if (out_dist) out_dist[i] = best;
    }
}

// The tile size a launch of assign_nearest_kernel takes: the tiles are walked in centre order and the minimum is
// strict, so the result does not depend on it.
template <typename... Args>
static int launch_assign_nearest(uint32_t dim, dim3 grid, hipStream_t st, Args &&...args) {
    const uint32_t dimp = (dim + 3u) & ~3u;
    const int tc = (size_t)kAsgTC * dimp * sizeof(float) <= kMaxLdsBytes ? kAsgTC : kAsgTCWide;
    return with_value<kAsgTC, kAsgTCWide>(tc, [&](auto t) {
        return launch(assign_nearest_kernel<t()>, grid, dim3(256), (size_t)t() * dimp * sizeof(float), st, args...);
    });
}

// The same assignment with squared_l2_avx2's summation order (simd/x86.rs:139-165), taken by
// KMeans::squared_distance_with_threshold when dim >= simd_threshold (trees/kmeans.rs:419-431):
// lane chain j accumulates fma(d, d, acc) over the dims = j (mod 8), the chains are combined by the
// fixed tree ((s0+s4 + s1+s5) + (s2+s6 + s3+s7)) of horizontal_sum_f32_avx2 (x86.rs:31-44), the
// dims past the last whole chunk of 8 are added unfused.  One thread per row, kAvxTC centres per
// LDS tile, the 8 chains of a centre as 4 packed-f32 pairs (v_pk_fma_f32 keeps both halves exact).
constexpr int kAvxTC = 8;

__global__ __launch_bounds__(256) void assign_nearest_avx_kernel(BfIndexDev ix, const float *__restrict__ centers,
                                                                 uint32_t k, uint32_t *__restrict__ out_idx,
                                                                 float *__restrict__ out_dist) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) float cs[];   // [kAvxTC][dimp]
    const uint32_t dim = ix.dim, dimp = (dim + 3u) & ~3u, chunks = dim >> 3;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = i < ix.n;
    const float *row = ix.rows + (act ? i : 0) * ix.stride;
    const bool vec = ((ix.stride & 3u) == 0) && ((reinterpret_cast<uintptr_t>(ix.rows) & 15u) == 0);
    float best = __builtin_inff();
    uint32_t bi = 0;
    for (uint32_t c0 = 0; c0 < k; c0 += kAvxTC) {
        for (uint32_t e = threadIdx.x; e < kAvxTC * dimp; e += blockDim.x) {
            const uint32_t c = e / dimp, j = e - c * dimp;
            cs[e] = (c0 + c < k && j < dim) ? centers[(size_t)(c0 + c) * dim + j] : 0.0f;
        }
        __syncthreads();
        f32x2 acc[kAvxTC][4];
#pragma unroll
        for (int c = 0; c < kAvxTC; ++c)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[c][u] = f32x2{0.0f, 0.0f};
        for (uint32_t ch = 0; ch < chunks; ++ch) {
            float4 xa, xb;
            if (vec) {
                xa = *reinterpret_cast<const float4 *>(row + 8 * ch);
                xb = *reinterpret_cast<const float4 *>(row + 8 * ch + 4);
            } else {
                xa = make_float4(row[8 * ch], row[8 * ch + 1], row[8 * ch + 2], row[8 * ch + 3]);
                xb = make_float4(row[8 * ch + 4], row[8 * ch + 5], row[8 * ch + 6], row[8 * ch + 7]);
            }
            const f32x2 x[4] = {f32x2{xa.x, xa.y}, f32x2{xa.z, xa.w}, f32x2{xb.x, xb.y}, f32x2{xb.z, xb.w}};
#pragma unroll
            for (int c = 0; c < kAvxTC; ++c) {
                const float4 ca = *reinterpret_cast<const float4 *>(cs + c * dimp + 8 * ch);
                const float4 cb = *reinterpret_cast<const float4 *>(cs + c * dimp + 8 * ch + 4);
                const f32x2 cv[4] = {f32x2{ca.x, ca.y}, f32x2{ca.z, ca.w}, f32x2{cb.x, cb.y}, f32x2{cb.z, cb.w}};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const f32x2 d = x[u] - cv[u];
                    acc[c][u] = __builtin_elementwise_fma(d, d, acc[c][u]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < kAvxTC; ++c) {
            // chains 0..7 = acc[0].x acc[0].y acc[1].x acc[1].y acc[2].x ...: (v0+v4, v1+v5), (v2+v6, v3+v7)
            const f32x2 s01 = acc[c][0] + acc[c][2], s23 = acc[c][1] + acc[c][3];
            float r = (s01.x + s01.y) + (s23.x + s23.y);
            for (uint32_t j = chunks * 8; j < dim; ++j) {   // scalar tail, not fused
                const float d = row[j] - cs[c * dimp + j];
                r = r + d * d;
            }
            if (c0 + c < k && r < best) {
                best = r;
                bi = c0 + c;
            }
        }
        __syncthreads();
    }
    if (act) {
        out_idx[i] = bi;
        if (out_dist) out_dist[i] = best;
    }
}

// =====================================================================================
// bf16 shortlist path (exact results, verified).  MI355X runs bf16 MFMA at 16x the f32 MFMA
// rate, but bf16 scores cannot meet the parity bar.  They CAN order the database
// coarsely: a bf16 pass shortlists kp >= 4k rows per query, the reference's f32 arithmetic
// re-scores only those, and the result is accepted when the k-th exact distance is below
// (kp-th smallest bf16 score) - E, where E bounds |bf16 score - exact| for EVERY row, so no row
// outside the shortlist can beat or tie the k-th result.  Plain bf16 (u = 2^-8) gives
// E = 2u |q||x|, as large as the gaps between neighbours at 1M x 128; the pass therefore uses
// SPLIT operands x = hi + lo (both bf16, lo = bf16(x - hi)) and three MFMAs per k-step,
//   q.x ~ qh.xh + qh.xl + ql.xh,   |error| <= (3 u^2 + O(u^3)) |q||x| + f32 accumulation
// -- 3/16 of the f32-MFMA time at 1/200 of the plain-bf16 error.  Queries that fail the test set
// status Aborted (and a per-query flag) and are repeated on the exact kernels (bf_search_host does
// it itself).  Accepted results are bit-identical to the exact path: same arithmetic, same rows.
// =====================================================================================
// |q.x - (qh.xh + qh.xl + ql.xh)| <= c(dim) |q||x| for EVERY row, with u = 2^-8:
//   dropped terms  ql.xl + qh.ex + eq.x (+ O(u^3))        <= 3.1 u^2 |q||x|
//   f32 accumulation of the 3 dim exact products (one rounding each, <= 2^-23 relative to the
//   running magnitude, which covers truncating alignment) and of the exact path itself
//                                                          <= (3 dim + 64) 2^-23 |q||x|
static inline float shortlist_dot_err(uint32_t dim) {
    return 1.01f * (3.1f / 65536.0f + (3.0f * (float)dim + 64.0f) / 8388608.0f);
}
// Quantized rows (fmt != 0): the row operand is exact in bf16 (bf16 itself; |i8| <= 128 fits 8 significant
// bits; every E4M3 value has <= 4 significant bits and an exponent in [-8, 8]), so only the query is split and
// the dropped terms shrink to eq.x <= 1.1 u^2 |q||x|; the accumulation term above is kept (2 dim MFMA products
// + the exact path's sequential sum of dim products stay under 3 dim + 64 roundings).  INT8: the MFMA scores
// q.i8 and the pass multiplies by s once (<= 2^-24 |q||x|), while the reference sums fl(i8 s), off by
// <= 2^-24 |i8 s| per element (<= 2^-24 |q||x| in total): + 2^-23.
static inline float shortlist_quant_err(uint32_t dim, int fmt) {
    return 1.01f * (1.1f / 65536.0f + (3.0f * (float)dim + 64.0f) / 8388608.0f +
                    (fmt == SCANN_HIP_ROWS_INT8 ? 1.0f / 8388608.0f : 0.0f));
}
constexpr float kF32SqErr = 6.0e-5f;       // f32 rounding of the norms, of |q|^2 + |x|^2 - 2 q.x and of the
                                           // exact (q - x)^2 sum, relative to |q|^2 + |x|^2 (dim <= 256)
constexpr uint32_t kShortMax = 256;        // largest shortlist per query

// (the element decoders of quantized rows and quant_step: quant.h, shared with the tree re-rank of txh_rows.hip)

__device__ __forceinline__ uint16_t f32_to_bf16_rne(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40u);   // NaN stays NaN
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

__device__ __forceinline__ float bf16_bits_to_f32(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }

// rows (or queries) -> split bf16 [n][dim] (hi, lo) + squared norms (f32, sequential)
__global__ void bf_to_bf16_kernel(const float *__restrict__ src, uint64_t n, uint32_t dim, uint32_t stride,
                                  uint16_t *__restrict__ dst_hi, uint16_t *__restrict__ dst_lo,
                                  float *__restrict__ norm2) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *row = src + i * stride;
    float s2 = 0.0f;
    for (uint32_t j = 0; j < dim; j += 8) {
        uint16_t bh[8], bl[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = row[j + e];
            s2 = s2 + v * v;
            bh[e] = f32_to_bf16_rne(v);
            bl[e] = f32_to_bf16_rne(v - bf16_bits_to_f32(bh[e]));   // exact difference, then rounded
        }
        uint4 ph, pl;
        ph.x = bh[0] | ((uint32_t)bh[1] << 16); ph.y = bh[2] | ((uint32_t)bh[3] << 16);
        ph.z = bh[4] | ((uint32_t)bh[5] << 16); ph.w = bh[6] | ((uint32_t)bh[7] << 16);
        pl.x = bl[0] | ((uint32_t)bl[1] << 16); pl.y = bl[2] | ((uint32_t)bl[3] << 16);
        pl.z = bl[4] | ((uint32_t)bl[5] << 16); pl.w = bl[6] | ((uint32_t)bl[7] << 16);
        *reinterpret_cast<uint4 *>(dst_hi + i * dim + j) = ph;
        *reinterpret_cast<uint4 *>(dst_lo + i * dim + j) = pl;
    }
    norm2[i] = s2;
}

// queries -> split bf16 + squared norms, one WAVE per query (a batch has few rows: the row-per-
// thread kernel above would run on a handful of threads)
__global__ __launch_bounds__(256) void bf_q_prep_kernel(const float *__restrict__ src, uint32_t nq, uint32_t dim,
                                                        uint32_t stride, uint16_t *__restrict__ dst_hi,
                                                        uint16_t *__restrict__ dst_lo, float *__restrict__ norm2) {
    const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (q >= nq) return;
    const float *row = src + (size_t)q * stride;
    float s2 = 0.0f;
    for (uint32_t j = lane; j < dim; j += 64) {
        const float v = row[j];
        s2 = s2 + v * v;
        const uint16_t bh = f32_to_bf16_rne(v);
        dst_hi[(size_t)q * dim + j] = bh;
        dst_lo[(size_t)q * dim + j] = f32_to_bf16_rne(v - bf16_bits_to_f32(bh));
    }
    for (int o = 32; o > 0; o >>= 1) s2 += __shfl_xor(s2, o);
    // upper bound of |q|^2 is what the error bound needs: one ulp of slack for the tree order
    if (lane == 0) norm2[q] = s2 * 1.0000002f;
}

__global__ void bf_max_norm_kernel(const float *__restrict__ norm2, uint64_t n, uint32_t *__restrict__ out_bits) {
    float m = 0.0f;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const float v = norm2[i];
        m = (v > m || v != v) ? v : m;     // NaN propagates -> nothing verifies -> exact path
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float t = __shfl_xor(m, o);
        m = (t > m || t != t) ? t : m;
    }
    if ((threadIdx.x & 63u) == 0) atomicMax(out_bits, __float_as_uint(m));   // non-negative floats order as uints
}

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// bf16 MFMA pass.  Block = 4 waves x 32 queries (B fragments resident), 32-row X tiles
// LDS-DMA'd and XOR-swizzled like bf_mfma_dot_kernel; v_mfma_f32_32x32x16_bf16:
//   A[i = lane & 31][k = 8h + j] = X[row i][16t + 8h + j], B[k][n = lane & 31] = Q[n][16t + 8h + j].
// Score = -dot (DotProduct) or |q|^2 + |x|^2 - 2 dot (SquaredL2 / L2: squared domain).
constexpr int kB16Waves = 4;      // waves per block: 8 x 32 = 256 queries share a stage
#ifndef SCANN_B16_OCC
#define SCANN_B16_OCC 3
#endif
#ifndef SCANN_B16_RING
#define SCANN_B16_RING 2
#endif
constexpr int kB16Occ = SCANN_B16_OCC;     // workgroups per CU = waves per SIMD (TS <= 8)
constexpr int kB16Ring = SCANN_B16_RING;   // LDS stages per workgroup
constexpr int kB16Sub = 1;        // 32-row sub-tiles per stage (one barrier per 64 rows)


// s_waitcnt vmcnt(2 * pairs): all but the wave's `pairs` youngest (hi, lo) DMA instruction pairs have
// completed.  pairs is wave-uniform; the immediate must be a constant.
__device__ __forceinline__ void wait_all_but_pairs(uint32_t pairs) {
    switch (pairs) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    }
}

// FMT != 0 (quantized rows): the row operand is the stored value as bf16 (exact, see shortlist_quant_err; INT8:
// the code i8, the score scaled by inv_mult), decoded by plain loads + LDS writes in the DMA's layout, and only
// two MFMAs per k-step (x.qh + x.ql); the lo half of the stage stays unused.
template <int TS, int MEASURE, int FMT>
__global__ __launch_bounds__(kB16Waves * 64, (TS <= 8 ? kB16Occ : 2)) void bf_bf16_kernel(BfIndexDev ix, BfPass p,
                                                                    const uint16_t *__restrict__ qb,
                                                                    const uint16_t *__restrict__ qbl,
                                                                    const float *__restrict__ qn2, uint32_t nx,
                                                                    uint32_t ny) {
    constexpr int DIM = TS * 16;
    constexpr int CPR = DIM / 8;                                       // 16-B chunks per bf16 row
    constexpr uint32_t SW = (CPR % 16 == 0) ? 15u : (CPR % 8 == 0 ? 7u : (CPR % 4 == 0 ? 3u : 1u));
    constexpr int RT = 32 * kB16Sub;                                   // rows per stage
    constexpr int TILE_B = RT * DIM * 2;                               // bytes of one (hi or lo) stage
    constexpr int NI = TILE_B / 1024;                                  // 1 KiB wave-instructions per stage
    constexpr int NBUF = kB16Ring;                                     // stages: this one + DIST in flight
    constexpr uint32_t DIST = NBUF - 1;
    constexpr int STAGE_B = 2 * TILE_B + 256;                          // hi | lo | RT norms (<= 64)
    constexpr int MYI = (NI + kB16Waves - 1) / kB16Waves;              // DMA instruction pairs per wave
    static_assert(RT <= 64, "one 4-byte DMA instruction carries the stage's norms");
    static_assert(MYI <= 4, "wait_all_but_pairs covers up to 4 pairs");
    extern __shared__ __attribute__((aligned(16))) unsigned char xsb[];   // [NBUF][STAGE_B] | survivor stages
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t h = lane >> 5, li = lane & 31u;
    const uint32_t bid = blockIdx.x, xcd = bid & 7u, slot = bid >> 3;
    const uint32_t x = xcd + 8u * (slot / ny), y = slot % ny;
    const uint32_t ntiles = (p.nrows + RT - 1u) / RT;
    // A survivor of the filter is held in a register of its lane and appended to the global
    // candidate list two iterations later: the returning atomic that reserves the list slot is
    // issued at the top of the next iteration, BEFORE that iteration's DMA, and its result is
    // consumed one iteration after that.  Emitting in place put an atomic round trip (~1-2 us)
    // into nearly every iteration; staging through LDS made the compiler wait for ALL outstanding
    // LDS-DMA before each staging write (it cannot prove that the DMA's LDS writes do not alias).
    const uint32_t q = y * (kB16Waves * 32u) + wave * 32u + li;
    const uint32_t qc = min(q, p.nq - 1u);
    bf16x8 qf[TS], ql[TS];
#pragma unroll
    for (int t = 0; t < TS; ++t) {
        qf[t] = *reinterpret_cast<const bf16x8 *>(qb + (size_t)qc * DIM + 16 * t + 8 * h);
        ql[t] = *reinterpret_cast<const bf16x8 *>(qbl + (size_t)qc * DIM + 16 * t + 8 * h);
        if (MEASURE == SCANN_HIP_DOT_PRODUCT) {   // the score is -dot: negate the query once (sign bits:
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // exact), not every score
            u32x4 a = __builtin_bit_cast(u32x4, qf[t]), b = __builtin_bit_cast(u32x4, ql[t]);
            a ^= 0x80008000u;
            b ^= 0x80008000u;
            qf[t] = __builtin_bit_cast(bf16x8, a);
            ql[t] = __builtin_bit_cast(bf16x8, b);
        }
    }
    const float q2 = MEASURE == SCANN_HIP_DOT_PRODUCT ? 0.0f : qn2[qc];
    uint64_t T = 0;
    float Tf = 0.0f;
    if (p.filter) {
        T = p.thr[qc];
        Tf = bf_thr_float(T);
    }
    const bool qvalid = q < p.nq;

    // per-lane pieces of the DMA source address that do not depend on the tile
    uint32_t lane_row[MYI], lane_col[MYI];
#pragma unroll
    for (int i = 0; i < MYI; ++i) {
        const uint32_t ci = (wave + (uint32_t)kB16Waves * i) * 64u + lane;   // linear chunk index in the stage
        const uint32_t r = ci / CPR, pos = ci - r * CPR;
        lane_row[i] = r;
        lane_col[i] = 8u * (pos ^ (r & SW));
    }
    uint32_t my_pairs = 0;                                             // DMA pairs this wave issues per stage
#pragma unroll
    for (int i = 0; i < MYI; ++i) my_pairs += (wave + (uint32_t)kB16Waves * i < (uint32_t)NI) ? 1u : 0u;
    my_pairs = __builtin_amdgcn_readfirstlane(my_pairs);
    const size_t row_pitch = (size_t)p.row_mult * DIM;                 // elements between virtual rows
    auto dma_tile = [&](uint32_t tile, uint32_t buf) {
        unsigned char *stage = xsb + (size_t)buf * STAGE_B;
        const bool last = tile * RT + RT > p.nrows;                    // wave-uniform: clamp only here
#pragma unroll
        for (int i = 0; i < MYI; ++i) {
            const uint32_t gi = wave + (uint32_t)kB16Waves * i;
            if constexpr (FMT != 0) {
                if (gi < (uint32_t)NI) {
                    uint32_t vr = tile * RT + lane_row[i];
                    if (last) vr = min(vr, p.nrows - 1u);
                    const size_t e0 = (size_t)vr * p.row_mult * ix.stride + lane_col[i];
                    const unsigned char *src = static_cast<const unsigned char *>(ix.qrows) + e0 * quant_bytes<FMT>();
                    uint32_t w[4];
                    if constexpr (FMT == SCANN_HIP_ROWS_BF16) {
                        const uint4 v = *reinterpret_cast<const uint4 *>(src);
                        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
                    } else {
                        const uint2 v = *reinterpret_cast<const uint2 *>(src);
                        const uint32_t b[2] = {v.x, v.y};
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const uint32_t wb = b[j >> 1] >> (16 * (j & 1));
                            // INT8: the code itself (exact in bf16); FP8: the decoded value (exact in bf16)
                            const float lo = FMT == SCANN_HIP_ROWS_INT8 ? (float)(int)(int8_t)(wb & 0xFFu)
                                                                        : fp8_e4m3_to_f32(wb & 0xFFu);
                            const float hi = FMT == SCANN_HIP_ROWS_INT8 ? (float)(int)(int8_t)((wb >> 8) & 0xFFu)
                                                                        : fp8_e4m3_to_f32((wb >> 8) & 0xFFu);
                            w[j] = (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xFFFF0000u);
                        }
                    }
                    *reinterpret_cast<uint4 *>(stage + gi * 1024u + lane * 16u) = make_uint4(w[0], w[1], w[2], w[3]);
                }
                continue;
            }
            if (gi < (uint32_t)NI) {
                uint32_t vr = tile * RT + lane_row[i];
                if (last) vr = min(vr, p.nrows - 1u);
                const size_t off = (size_t)vr * row_pitch + lane_col[i];
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void *)(ix.rows_b + off),
                    (__attribute__((address_space(3))) void *)(stage + gi * 1024u), 16, 0, 0);
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void *)(ix.rows_bl + off),
                    (__attribute__((address_space(3))) void *)(stage + TILE_B + gi * 1024u), 16, 0, 0);
            }
        }
        if (MEASURE != SCANN_HIP_DOT_PRODUCT && tid < (uint32_t)RT) {
            const uint32_t vr = min(tile * RT + tid, p.nrows - 1u);
            reinterpret_cast<float *>(stage + 2 * TILE_B)[tid] = ix.norm2[(size_t)vr * p.row_mult];
        }
    };
    // squared norms of the stage's rows (plain loads: staged after the MFMAs so that their wait
    // coincides with the end-of-iteration wait for the DMA)
    auto stage_norms = [&](uint32_t tile, uint32_t buf) {
        if (MEASURE != SCANN_HIP_DOT_PRODUCT && tid < (uint32_t)RT) {
            const uint32_t vr = min(tile * RT + tid, p.nrows - 1u);
            reinterpret_cast<float *>(xsb + (size_t)buf * STAGE_B + 2 * TILE_B)[tid] =
                ix.norm2[(size_t)vr * p.row_mult];
        }
    };

    uint32_t tile = x;
    if (tile >= ntiles) return;   // uniform per block
    dma_tile(tile, 0);
    stage_norms(tile, 0);
    if (DIST == 2 && tile + nx < ntiles) {   // second stage in flight; only the first must have landed
        dma_tile(tile + nx, 1);
        stage_norms(tile + nx, 1);
        if (MEASURE == SCANN_HIP_DOT_PRODUCT) wait_all_but_pairs(my_pairs);
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    const f32x16 zero = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f,
                         0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const uint32_t sw = li & SW;
    bool phas = false, fhas = false;       // this lane's survivor found / slot reservation in flight
    uint64_t pkey = 0, fkey = 0;
    uint32_t fpos = 0;
    for (uint32_t it = 0; tile < ntiles; tile += nx, ++it) {
        const uint32_t buf = it % NBUF, buf2 = (it + DIST) % NBUF;
        const bool more = tile + DIST * nx < ntiles;      // a stage DIST tiles ahead to fetch
        // Survivors travel two iterations behind: the one found in iteration i-1 gets its list slot
        // reserved now, the one reserved in iteration i-1 is stored now -- both before this
        // iteration's DMA, so the counted wait at the end never waits for the DMA itself.
        if (fhas && fpos < p.cap) p.cand[(size_t)q * p.cap + fpos] = fkey;
        fhas = phas;
        fkey = pkey;
        phas = false;
        if (fhas) fpos = atomicAdd(&p.cand_cnt[q], 1u);
        if (more) dma_tile(tile + DIST * nx, buf2);       // lands during the MFMAs of the stages before it
        const unsigned char *stage = xsb + (size_t)buf * STAGE_B;
#pragma unroll
        for (int sub = 0; sub < kB16Sub; ++sub) {
            const uint32_t row0 = tile * RT + 32u * sub;
            if (row0 >= p.nrows) break;                                 // uniform
            const float *nrm = reinterpret_cast<const float *>(stage + 2 * TILE_B) + 32 * sub;
            f32x16 acc = zero;
            const unsigned char *xrow = stage + (size_t)(32 * sub + li) * DIM * 2;
#pragma unroll
            for (int t = 0; t < TS; ++t) {
                const uint32_t c0 = 2u * t + h;
                const bf16x8 a = *reinterpret_cast<const bf16x8 *>(xrow + 16u * (c0 ^ sw));
                bf16x8 al;
                if constexpr (FMT == 0) al = *reinterpret_cast<const bf16x8 *>(xrow + TILE_B + 16u * (c0 ^ sw));
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qf[t], acc, 0, 0, 0);
                if constexpr (FMT == 0) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, qf[t], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, ql[t], acc, 0, 0, 0);
            }
            if constexpr (FMT == SCANN_HIP_ROWS_INT8) acc = acc * ix.inv_mult;   // q.i8 -> q.(i8 s)
            float sc[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (MEASURE == SCANN_HIP_DOT_PRODUCT) {
                    sc[r] = acc[r];     // the query fragments carry the sign
                } else {
                    sc[r] = (q2 + nrm[(r & 3) + 8 * (r >> 2) + 4 * h]) - 2.0f * acc[r];
                }
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
                                } else {                                   // a second survivor of this lane
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
                    if (qvalid && (full || vrow < p.nrows)) p.out[(size_t)q * p.ld + vrow] = sc[r];
                }
            }
        }
        if (more) stage_norms(tile + DIST * nx, buf2);
        // The NEXT stage must have landed; the one just issued may stay in flight.  vmcnt counts in
        // issue order, and at least this wave's DMA instructions of this iteration are younger than
        // the next stage's (the survivor atomic / store, when issued, only make the wait stricter).
        if (DIST == 2 && more && MEASURE == SCANN_HIP_DOT_PRODUCT) wait_all_but_pairs(my_pairs);
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    // drain: the slot reserved in the last iteration, then the survivor found in it
    if (fhas && fpos < p.cap) p.cand[(size_t)q * p.cap + fpos] = fkey;
    if (phas) {
        const uint32_t pos = atomicAdd(&p.cand_cnt[q], 1u);
        if (pos < p.cap) p.cand[(size_t)q * p.cap + pos] = pkey;
    }
}

// exact f32 score of the shortlisted rows with the reference's arithmetic (simd/x86.rs:72-96,
// 139-165): 8 lanes per candidate = the 8 AVX2 FMA lane chains, hsum tree by shuffles, scalar tail.
template <int MEASURE>
__global__ __launch_bounds__(256) void bf_rerank_kernel(BfIndexDev ix, const float *__restrict__ queries,
                                                        uint32_t q_stride, uint32_t kp,
                                                        const uint32_t *__restrict__ sl_idx,
                                                        const uint32_t *__restrict__ sl_cnt,
                                                        float *__restrict__ sl_exact) {
    extern __shared__ __attribute__((aligned(16))) float s_q[];   // [dim]
    const uint32_t q = blockIdx.y, tid = threadIdx.x;
    const uint32_t nsel = min(sl_cnt[q], kp);
    const uint32_t c0 = blockIdx.x * 32u;
    if (c0 >= nsel) return;   // uniform
    const uint32_t dim = ix.dim;
    for (uint32_t j = tid; j < dim; j += blockDim.x) s_q[j] = queries[(size_t)q * q_stride + j];
    __syncthreads();
    const uint32_t chunks = dim >> 3, lane8 = tid & 7u;
    const uint32_t c = c0 + (tid >> 3);
    const bool act = c < nsel;
    float accv = 0.0f;
    const float *row = ix.rows;
    if (act) row = ix.rows + (size_t)sl_idx[(size_t)q * kp + c] * ix.stride;
    for (uint32_t i0 = 0; i0 < chunks; i0 += 8) {
        float xv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) xv[u] = (act && i0 + u < chunks) ? row[8 * (i0 + u) + lane8] : 0.0f;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (i0 + u < chunks) {
                const float qv = s_q[8 * (i0 + u) + lane8];
                if (MEASURE == SCANN_HIP_DOT_PRODUCT) {
                    accv = fmaf(qv, xv[u], accv);
                } else {
                    const float diff = qv - xv[u];
                    accv = fmaf(diff, diff, accv);
                }
            }
        }
    }
    float s = accv + __shfl_down(accv, 4, 8);
    float t = s + __shfl_down(s, 1, 8);
    float r = t + __shfl_down(t, 2, 8);
    if (act && lane8 == 0) {
        for (uint32_t j = chunks * 8; j < dim; ++j) {   // scalar tail, not fused
            if (MEASURE == SCANN_HIP_DOT_PRODUCT) {
                r = r + s_q[j] * row[j];
            } else {
                const float diff = s_q[j] - row[j];
                r = r + diff * diff;
            }
        }
        sl_exact[(size_t)q * kp + c] = MEASURE == SCANN_HIP_DOT_PRODUCT ? -r : r;   // L2: squared here
    }
}

// Quantized rows: exact score of the shortlisted rows with bf_quant_kernel's arithmetic (one_to_many_asymmetric.rs:
// bf16 / FP8 one sequential sum; INT8 8 FMA chains + horizontal_sum_avx + unfused tail), one candidate per thread.
template <int FMT, int MEASURE>
__global__ __launch_bounds__(256) void bf_quant_rerank_kernel(BfIndexDev ix, const float *__restrict__ queries,
                                                              uint32_t q_stride, uint32_t kp,
                                                              const uint32_t *__restrict__ sl_idx,
                                                              const uint32_t *__restrict__ sl_cnt,
                                                              float *__restrict__ sl_exact) {
    extern __shared__ __attribute__((aligned(16))) float s_q[];   // [dim]
    const uint32_t q = blockIdx.y, tid = threadIdx.x, dim = ix.dim;
    const uint32_t nsel = min(sl_cnt[q], kp);
    if (blockIdx.x * 256u >= nsel) return;   // uniform
    for (uint32_t j = tid; j < dim; j += blockDim.x) s_q[j] = queries[(size_t)q * q_stride + j];
    __syncthreads();
    const uint32_t c = blockIdx.x * 256u + tid;
    if (c >= nsel) return;
    constexpr bool FUSED = FMT == SCANN_HIP_ROWS_INT8;
    const float inv = ix.inv_mult;
    const uint8_t *row = static_cast<const uint8_t *>(ix.qrows) +
                         (size_t)sl_idx[(size_t)q * kp + c] * ix.stride * quant_bytes<FMT>();
    f32x2q acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = f32x2q{0.0f, 0.0f};
    uint32_t e = 0;
    for (; e + 8 <= dim; e += 8)
#pragma unroll
        for (int t = 0; t < 8; ++t)
            quant_step<MEASURE, FUSED>(acc[FUSED ? t : 0], f32x2q{s_q[e + t], 0.0f}, quant_load1<FMT>(row, e + t, inv));
    float r = acc[0].x;
    if (FUSED) {   // horizontal_sum_avx
        const float s0 = acc[0].x + acc[4].x, s1 = acc[1].x + acc[5].x, s2 = acc[2].x + acc[6].x,
                    s3 = acc[3].x + acc[7].x;
        r = (s0 + s1) + (s2 + s3);
    }
    for (; e < dim; ++e) {
        f32x2q rv = f32x2q{r, 0.0f};
        quant_step<MEASURE, false>(rv, f32x2q{s_q[e], 0.0f}, quant_load1<FMT>(row, e, inv));
        r = rv.x;
    }
    sl_exact[(size_t)q * kp + c] = MEASURE == SCANN_HIP_DOT_PRODUCT ? -r : r;   // L2: squared here
}

// Quantized rows: squared norms of the decoded values (sequential f32, as bf_to_bf16_kernel) for the shortlist bound.
template <int FMT>
__global__ void bf_quant_norms_kernel(BfIndexDev ix, float *__restrict__ norm2) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ix.n) return;
    const uint8_t *row = static_cast<const uint8_t *>(ix.qrows) + i * ix.stride * quant_bytes<FMT>();
    float s2 = 0.0f;
    for (uint32_t j = 0; j < ix.dim; ++j) {
        const float v = quant_load1<FMT>(row, j, ix.inv_mult);
        s2 = s2 + v * v;
    }
    norm2[i] = s2;
}

// per query (one wave): sort the shortlist by (exact, index), emit the first k, verify.
template <int MEASURE>
__global__ __launch_bounds__(64) void bf_shortlist_final_kernel(
    uint32_t n, uint32_t k, uint32_t kp, float max_norm, float dot_err, const float *__restrict__ qn2,
    const uint64_t *__restrict__ thr, const uint32_t *__restrict__ sl_idx, const float *__restrict__ sl_approx,
    const uint32_t *__restrict__ sl_cnt, const float *__restrict__ sl_exact,
    uint32_t *__restrict__ counters, uint32_t *__restrict__ fail_flag, uint32_t *__restrict__ out_idx,
    float *__restrict__ out_dist, uint32_t *__restrict__ out_count) {
    __shared__ uint64_t skeys[kShortMax];
    const uint32_t q = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const uint32_t nsel = min(sl_cnt[q], kp);
    uint32_t n2 = 1;
    while (n2 < nsel) n2 <<= 1;
    // L2: key on the root, as the exact kernels do -- two squared distances can round to one L2 distance, and
    // those rows tie and go by index
    for (uint32_t i = tid; i < n2; i += nt) {
        float e = i < nsel ? sl_exact[(size_t)q * kp + i] : 0.0f;
        if (MEASURE == SCANN_HIP_L2) e = sqrtf(e);
        skeys[i] = i < nsel ? make_key(e, sl_idx[(size_t)q * kp + i]) : SCANN_KEY_MAX;
    }
    __syncthreads();
    bitonic_sort_lds(skeys, n2);
    const uint32_t nout = min(k, nsel);
    for (uint32_t i = tid; i < k; i += nt) {
        float d = __builtin_inff();
        uint32_t id = kBfInvalid;
        if (i < nout) {
            id = (uint32_t)skeys[i];
            d = ordered_to_f32((uint32_t)(skeys[i] >> 32));
        }
        out_idx[(size_t)q * k + i] = id;
        out_dist[(size_t)q * k + i] = d;
    }
    if (tid == 0) {
        out_count[q] = nout;
        bool ok = nsel >= n;                         // everything was re-scored
        if (!ok && nout == k) {
            // every row outside the shortlist scores >= the shortlist's largest bf16 score; a
            // shortlist shorter than kp holds EVERY row that passed the filter, so the rest score
            // >= the filter's bound
            const float floor_b = nsel == kp ? sl_approx[(size_t)q * kp + kp - 1] : bf_thr_float(thr[q]);
            const float dk = ordered_to_f32((uint32_t)(skeys[k - 1] >> 32));   // k-th exact (the root for L2)
            const float qn = sqrtf(qn2[q]);
            float E;
            if (MEASURE == SCANN_HIP_DOT_PRODUCT) E = dot_err * qn * max_norm;
            else E = 2.0f * dot_err * qn * max_norm + kF32SqErr * (qn * qn + max_norm * max_norm);
            // L2: every row outside scores >= floor_b - E squared, so its root is >= the root of that (sqrtf is
            // monotone); strictly above dk, no root ties it
            const float lb = floor_b - E * 1.0001f;
            ok = MEASURE == SCANN_HIP_L2 ? dk < sqrtf(lb) : dk < lb;   // NaNs compare false -> exact path
        }
        fail_flag[q] = ok ? 0u : 1u;
        if (!ok) atomicMax(&counters[BF_CNT_STATUS], (uint32_t)SCANN_HIP_ABORTED);
    }
}

// =====================================================================================
// threshold from the sample matrix [nq][ns]; when the sample is the whole dataset
// (row_mult == 1, ns == n) the sorted sample IS the answer and is written directly.
// =====================================================================================
__global__ __launch_bounds__(kBfSelectThreads) void bf_threshold_kernel(
    const float *__restrict__ sample, uint32_t ns, uint32_t row_mult, uint32_t k, int direct,
    uint64_t *__restrict__ thr, uint32_t *__restrict__ out_idx, float *__restrict__ out_dist,
    uint32_t *__restrict__ out_count, const uint32_t *__restrict__ ids, const uint64_t *__restrict__ allow,
    uint32_t allow_bits) {
    extern __shared__ __attribute__((aligned(16))) uint64_t skeys[];   // [next_pow2(ns)]
    const uint32_t q = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    uint32_t n2 = 1;
    while (n2 < ns) n2 <<= 1;
    // Key of sample i.  Under a filter the index half is the datapoint index (ids: the compacted list), and a
    // sample whose datapoint the bitmap rejects is ABSENT (SCANN_KEY_MAX), not a distance: the bound is taken over
    // allowed samples only -- with fewer than k of them the k-th key is SCANN_KEY_MAX, the no-bound value.
    auto sample_key = [&](uint32_t i) -> uint64_t {
        const uint32_t r = i * row_mult, row = ids ? ids[r] : r;
        if (allow && !bf_row_allowed(allow, allow_bits, row)) return SCANN_KEY_MAX;
        return make_key(sample[(size_t)q * ns + i], row);
    };
    if (!direct) {
        // the k-th smallest sample key bounds the k-th smallest key of the whole dataset; a
        // histogram rank-select finds it without sorting the 8192 samples
        const SelCfg cfg = sel_cfg(ns);
        uint32_t *s_hist = reinterpret_cast<uint32_t *>(skeys + n2);
        uint64_t *s_list = reinterpret_cast<uint64_t *>(s_hist + cfg.bins);
        uint64_t *s_red = s_list + cfg.list;
        for (uint32_t i = tid; i < ns; i += nt) skeys[i] = sample_key(i);
        __syncthreads();
        uint64_t T = SCANN_KEY_MAX;
        if (ns >= k && k > 0) T = block_select<uint64_t>(skeys, ns, k, cfg, s_hist, s_list, s_red);
        if (tid == 0) thr[q] = T;
        return;
    }
    uint32_t *s_absent = reinterpret_cast<uint32_t *>(skeys + n2);   // rows the bitmap rejects
    if (tid == 0) *s_absent = 0;
    __syncthreads();
    for (uint32_t i = tid; i < n2; i += nt) {
        const uint64_t key = (i < ns) ? sample_key(i) : SCANN_KEY_MAX;
        if (allow && i < ns && key == SCANN_KEY_MAX) atomicAdd(s_absent, 1u);   // (no real key of an allowed row is
        skeys[i] = key;                                                          // MAX: its index half is a row < n)
    }
    __syncthreads();
    bitonic_sort_lds(skeys, n2);
    const uint32_t nout = min(k, ns - *s_absent);
    for (uint32_t i = tid; i < k; i += nt) {
        out_idx[(size_t)q * k + i] = (i < nout) ? (uint32_t)skeys[i] : kBfInvalid;
        out_dist[(size_t)q * k + i] =
            (i < nout) ? ordered_to_f32((uint32_t)(skeys[i] >> 32)) : __builtin_inff();
    }
    if (tid == 0) out_count[q] = nout;
}

// =====================================================================================
// Allow-list compaction: the ascending list of allowed datapoint indices.  Word w of the bitmap covers datapoints
// [64 w, 64 w + 64); bits at or past `bits` (the capacity clipped to the row count) are masked off.  Two launches:
// per-block popcounts of kCompactWords words, then every block adds up the blocks before it, scans its own words
// and writes their set bits in order.  *total = the allowed count A.
// =====================================================================================
constexpr uint32_t kCompactWords = 256;   // bitmap words per block = one per thread

__device__ __forceinline__ uint64_t bf_allow_word(const uint64_t *allow, uint32_t bits, uint32_t w) {
    if ((uint64_t)w * 64u >= bits) return 0;
    const uint64_t v = allow[w];
    const uint32_t rem = bits - w * 64u;
    return rem >= 64u ? v : (v & ((1ull << rem) - 1ull));
}

__global__ __launch_bounds__(kCompactWords) void bf_allow_count_kernel(const uint64_t *__restrict__ allow, uint32_t bits,
                                                                       uint32_t *__restrict__ block_sums) {
    __shared__ uint32_t s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    const uint32_t c = (uint32_t)__popcll(bf_allow_word(allow, bits, blockIdx.x * kCompactWords + threadIdx.x));
    if (c) atomicAdd(&s_sum, c);
    __syncthreads();
    if (threadIdx.x == 0) block_sums[blockIdx.x] = s_sum;
}

__global__ __launch_bounds__(kCompactWords) void bf_allow_compact_kernel(const uint64_t *__restrict__ allow, uint32_t bits,
                                                                         const uint32_t *__restrict__ block_sums,
                                                                         uint32_t *__restrict__ ids, uint32_t ids_cap,
                                                                         uint32_t *__restrict__ total) {
    __shared__ uint32_t s_base, s_wave[kCompactWords / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0) s_base = 0;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t b = tid; b < blockIdx.x; b += kCompactWords) before += block_sums[b];
    if (before) atomicAdd(&s_base, before);
    const uint32_t w = blockIdx.x * kCompactWords + tid;
    uint64_t word = bf_allow_word(allow, bits, w);
    const uint32_t c = (uint32_t)__popcll(word);
    uint32_t incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
        if ((int)lane >= o) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t pos = s_base + incl - c;
    for (uint32_t w2 = 0; w2 < wave; ++w2) pos += s_wave[w2];
    while (word) {
        const uint32_t b = (uint32_t)__builtin_ctzll(word);
        word &= word - 1ull;
        if (pos < ids_cap) ids[pos] = w * 64u + b;
        ++pos;
    }
    if (blockIdx.x == gridDim.x - 1 && tid == kCompactWords - 1) *total = pos;
}

// In-place stable compaction (keys <= T) by one block.
__device__ static uint32_t bf_block_compact_le(uint64_t *list, uint32_t cnt, uint64_t T,
                                               uint32_t *s_wave, uint32_t *s_base) {
    const uint32_t tid = threadIdx.x, nt = blockDim.x, wave = tid >> 6, nw = nt >> 6;
    if (tid == 0) *s_base = 0;
    __syncthreads();
    for (uint32_t b = 0; b < cnt; b += nt) {
        const uint32_t i = b + tid;
        uint64_t key = 0;
        bool keep = false;
        if (i < cnt) {
            key = list[i];
            keep = key <= T;
        }
        uint32_t wtot;
        const uint32_t wpre = wave_prefix_count(keep, &wtot);
        if ((tid & 63u) == 0) s_wave[wave] = wtot;
        __syncthreads();
        uint32_t off = *s_base;
        for (uint32_t w = 0; w < wave; ++w) off += s_wave[w];
        if (keep) list[off + wpre] = key;
        __syncthreads();
        if (tid == 0) {
            uint32_t t = 0;
            for (uint32_t w = 0; w < nw; ++w) t += s_wave[w];
            *s_base += t;
        }
        __syncthreads();
    }
    return *s_base;
}

__global__ __launch_bounds__(kBfSelectThreads) void bf_select_kernel(
    uint32_t k, uint32_t cap, uint32_t *__restrict__ cand_cnt, uint64_t *__restrict__ cand,
    uint32_t *__restrict__ counters, uint32_t *__restrict__ out_idx, float *__restrict__ out_dist,
    uint32_t *__restrict__ out_count) {
    extern __shared__ __attribute__((aligned(16))) uint64_t skeys[];   // [kBfSortCap]
    uint32_t *s_wave = reinterpret_cast<uint32_t *>(skeys + kBfSortCap);
    uint32_t *s_base = s_wave + kBfSelectThreads / 64;
    const uint32_t q = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    uint32_t cnt = cand_cnt[q];
    uint64_t *list = cand + (size_t)q * cap;
    bool bad = cnt > cap;
    while (!bad && cnt > kBfSortCap) {
        const uint32_t stride = (cnt + kBfSortCap / 2 - 1) / (kBfSortCap / 2);
        const uint32_t ns = (cnt + stride - 1) / stride;
        uint32_t n2 = 1;
        while (n2 < ns) n2 <<= 1;
        for (uint32_t i = tid; i < n2; i += nt)
            skeys[i] = (i < ns) ? list[(size_t)i * stride] : SCANN_KEY_MAX;
        __syncthreads();
        bitonic_sort_lds(skeys, n2);
        const uint64_t T = (ns >= k) ? skeys[k - 1] : SCANN_KEY_MAX;
        __syncthreads();
        const uint32_t nc = bf_block_compact_le(list, cnt, T, s_wave, s_base);
        __syncthreads();
        if (nc >= cnt) bad = true; else cnt = nc;
    }
    if (bad) {
        if (tid == 0) {
            atomicMax(&counters[BF_CNT_STATUS], (uint32_t)SCANN_HIP_RESOURCE_EXHAUSTED);
            out_count[q] = 0;
        }
        return;
    }
    // the k smallest of the cnt survivors: rank-select the k-th key, sort only those k
    const uint32_t nout = min(k, cnt);
    uint32_t k2 = 1;
    while (k2 < nout) k2 <<= 1;
    const SelCfg cfg = sel_cfg(kBfSortCap);
    uint64_t *s_top = reinterpret_cast<uint64_t *>(s_base + 4);            // [kBfMaxK]
    uint32_t *s_hist = reinterpret_cast<uint32_t *>(s_top + kBfMaxK);
    uint64_t *s_list = reinterpret_cast<uint64_t *>(s_hist + cfg.bins);
    uint64_t *s_red = s_list + cfg.list;
    for (uint32_t i = tid; i < cnt; i += nt) skeys[i] = list[i];
    for (uint32_t i = tid; i < k2; i += nt) s_top[i] = SCANN_KEY_MAX;
    if (tid == 0) *s_base = 0;
    __syncthreads();
    if (nout) {
        const uint64_t T = cnt > nout ? block_select<uint64_t>(skeys, cnt, nout, cfg, s_hist, s_list, s_red)
                                      : SCANN_KEY_MAX;
        for (uint32_t i = tid; i < cnt; i += nt) {
            const uint64_t key = skeys[i];
            if (key <= T) s_top[atomicAdd(s_base, 1u)] = key;   // exactly nout keys (unique)
        }
        __syncthreads();
        bitonic_sort_lds(s_top, k2);
    }
    for (uint32_t i = tid; i < k; i += nt) {
        out_idx[(size_t)q * k + i] = (i < nout) ? (uint32_t)s_top[i] : kBfInvalid;
        out_dist[(size_t)q * k + i] =
            (i < nout) ? ordered_to_f32((uint32_t)(s_top[i] >> 32)) : __builtin_inff();
    }
    if (tid == 0) out_count[q] = nout;
}

// =====================================================================================
// Quantized rows (scann_hip_bf_create_quantized): f32 queries against bf16 / E4M3 / int8 rows,
// one_to_many_{bf16,fp8,int8}_float_{dot_product,squared_l2} (distance_measures/one_to_many_asymmetric.rs).
//  * BF16, FP8_E4M3 (:267-377): one sequential f32 sum per (query, row), no FMA.
//  * INT8, the AVX2 form (:78-142, :208-257): x = (float)i8 * inv_multiplier (rounded), 8 FMA lane chains
//    over full 8-element chunks, horizontal_sum_avx = ((c0+c4)+(c1+c5)) + ((c2+c6)+(c3+c7)), unfused tail.
// Dot products are negated; L2 = sqrtf(SquaredL2) (brute_force/scalar_quantized.rs:217-224).
// One row per lane, QT queries from LDS ([dim][QT], a query pair = one 8-byte broadcast read) computed in
// pairs on the packed-f32 pipe (v_pk_*: two IEEE operations, the results of the scalar ones).  A lane reads
// its row 64 elements at a time (8 x 16-byte loads in flight for bf16, 4 for the byte formats, so a cache line
// of the row is consumed in one or two consecutive visits) and decodes in registers.  (128 byte-format elements
// at a time spill: the compiler decodes them all before the first use.)
// =====================================================================================
template <int FMT, int MEASURE, int QT>
__global__ __launch_bounds__(256) void bf_quant_kernel(BfIndexDev ix, BfPass p) {
    static_assert(QT % 2 == 0, "queries travel in pairs");
    constexpr int NCH = FMT == SCANN_HIP_ROWS_INT8 ? 8 : 1;   // accumulator chains per query
    constexpr bool FUSED = FMT == SCANN_HIP_ROWS_INT8;
    constexpr uint32_t B = quant_bytes<FMT>(), EPW = 4 / B, EPV = 16 / B;   // elements per word / per 16 B
    constexpr int NV = 64 / EPV;                                             // 16-byte loads per 64 elements
    extern __shared__ __attribute__((aligned(16))) float qs[];   // [dim][QT]
    const uint32_t dim = ix.dim;
    const uint32_t q0 = blockIdx.y * QT;
    for (uint32_t i = threadIdx.x; i < QT * dim; i += blockDim.x) {
        const uint32_t j = i / QT, qi = i - j * QT;
        qs[i] = q0 + qi < p.nq ? p.queries[(size_t)(q0 + qi) * p.q_stride + j] : 0.0f;
    }
    __syncthreads();
    const uint32_t vrow = blockIdx.x * blockDim.x + threadIdx.x;
    if (vrow >= p.nrows) return;
    const float inv = ix.inv_mult;
    const uint8_t *row = static_cast<const uint8_t *>(ix.qrows) + (size_t)bf_real_row(p, vrow) * ix.stride * B;
    const bool vec = (((size_t)ix.stride * B) & 15u) == 0 && (reinterpret_cast<uintptr_t>(ix.qrows) & 15u) == 0;
    f32x2q acc[QT / 2][NCH];
#pragma unroll
    for (int h = 0; h < QT / 2; ++h)
#pragma unroll
        for (int c = 0; c < NCH; ++c) acc[h][c] = f32x2q{0.0f, 0.0f};
    // element e0 + t of the row, t a compile-time offset with e0 % 8 == 0: chain t & 7
    auto consume = [&](uint32_t e0, int t, float x) {
#pragma unroll
        for (int h = 0; h < QT / 2; ++h) {
            const float2 qv = *reinterpret_cast<const float2 *>(qs + (size_t)(e0 + t) * QT + 2 * h);
            quant_step<MEASURE, FUSED>(acc[h][NCH == 8 ? (t & 7) : 0], f32x2q{qv.x, qv.y}, x);
        }
    };
    uint32_t e = 0;
    if (vec) {
        for (; e + 64 <= dim; e += 64) {
            uint4 r[NV];
#pragma unroll
            for (int i = 0; i < NV; ++i) r[i] = *reinterpret_cast<const uint4 *>(row + (size_t)e * B + 16 * i);
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const uint32_t w[4] = {r[i].x, r[i].y, r[i].z, r[i].w};
#pragma unroll
                for (int wi = 0; wi < 4; ++wi)
#pragma unroll
                    for (int s = 0; s < (int)EPW; ++s)
                        consume(e, i * EPV + wi * EPW + s, quant_decode<FMT>(w[wi], s, inv));
            }
        }
        for (; e + EPV <= dim; e += EPV) {
            const uint4 r = *reinterpret_cast<const uint4 *>(row + (size_t)e * B);
            const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
            for (int wi = 0; wi < 4; ++wi)
#pragma unroll
                for (int s = 0; s < (int)EPW; ++s) consume(e, wi * EPW + s, quant_decode<FMT>(w[wi], s, inv));
        }
    }
    for (; e + 8 <= dim; e += 8)   // full 8-element chunks (int8: the FMA chains)
#pragma unroll
        for (int t = 0; t < 8; ++t) consume(e, t, quant_load1<FMT>(row, e + t, inv));
    f32x2q r[QT / 2];
#pragma unroll
    for (int h = 0; h < QT / 2; ++h) {
        if constexpr (NCH == 8) {   // horizontal_sum_avx (one_to_many_asymmetric.rs:386-399)
            const f32x2q s0 = acc[h][0] + acc[h][4], s1 = acc[h][1] + acc[h][5];
            const f32x2q s2 = acc[h][2] + acc[h][6], s3 = acc[h][3] + acc[h][7];
            r[h] = (s0 + s1) + (s2 + s3);
        } else {
            r[h] = acc[h][0];
        }
    }
    for (; e < dim; ++e) {   // bf16 / FP8: the rest of the sequential sum; int8: the unfused scalar tail
        const float x = quant_load1<FMT>(row, e, inv);
#pragma unroll
        for (int h = 0; h < QT / 2; ++h) {
            const float2 qv = *reinterpret_cast<const float2 *>(qs + (size_t)e * QT + 2 * h);
            quant_step<MEASURE, false>(r[h], f32x2q{qv.x, qv.y}, x);
        }
    }
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) {
        if (q0 + qi >= p.nq) continue;
        float dist = (qi & 1) ? r[qi / 2].y : r[qi / 2].x;
        if (MEASURE == SCANN_HIP_DOT_PRODUCT) dist = -dist;
        if (MEASURE == SCANN_HIP_L2) dist = sqrtf(dist);
        uint64_t T = 0;
        float Tf = 0.0f;
        if (p.filter) {
            T = p.thr[q0 + qi];
            Tf = bf_thr_float(T);
        }
        bf_emit(p, q0 + qi, vrow, dist, Tf, T);
    }
}

// half::bf16::from_f32 over n values (bf16_from_f32, quant.h)
__global__ __launch_bounds__(256) void bf16_quantize_kernel(const float *__restrict__ values, uint64_t n,
                                                            uint16_t *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        out[i] = (uint16_t)bf16_from_f32(values[i]);
    }
}

// =====================================================================================
// host side
// =====================================================================================
// row length -> template argument of the MFMA kernels (dim / 16; default: 16) and of bf_vq_kernel (dim / 8; default: 16)
template <typename F>
static int with_dim16(uint32_t dim, F &&f) {
    return with_value<2, 4, 6, 8, 12, 16>((int)(dim / 16), std::forward<F>(f));
}
template <typename F>
static int with_dim8(uint32_t dim, F &&f) {
    return with_value<4, 8, 12, 16>((int)(dim / 8), std::forward<F>(f));
}

template <int TS>
static int launch_mfma(const BfIndexDev &ix, const BfPass &p, hipStream_t st) {
    const uint32_t ny = ceil_div_u32(p.nq, 128);
    const uint32_t ntiles = ceil_div_u32(p.nrows, 32);
    uint32_t want = std::max<uint32_t>(1, (4u * (uint32_t)num_cus()) / ny);
    want = std::min(want, ntiles);
    const uint32_t nx = 8u * ceil_div_u32(want, 8);
    const size_t lds = (size_t)2 * 32 * (TS * 16) * sizeof(float);
    return launch(bf_mfma_dot_kernel<TS>, dim3(nx * ny), dim3(256), lds, st, ix, p, nx, ny);
}

static bool mfma_eligible(const BfIndexDev &ix) {
    if (ix.measure != SCANN_HIP_DOT_PRODUCT) return false;
    if ((ix.stride & 3u) || (reinterpret_cast<uintptr_t>(ix.rows) & 15u)) return false;
    switch (ix.dim) {
        case 32: case 64: case 96: case 128: case 192: case 256: return true;
        default: return false;
    }
}

// one-query-per-lane kernel: SquaredL2 / L2, dim in {32, 64, 96, 128}, enough queries to fill waves
static bool vq_eligible(const BfIndexDev &ix, const BfPass &p) {
    if (ix.measure != SCANN_HIP_SQUARED_L2 && ix.measure != SCANN_HIP_L2) return false;
    if ((ix.stride & 3u) || (reinterpret_cast<uintptr_t>(ix.rows) & 15u)) return false;
    if (ix.dim != 32 && ix.dim != 64 && ix.dim != 96 && ix.dim != 128) return false;
    return p.nq >= 128;
}

// LDS of bf_stream_kernel: kStQT queries and the four waves' staging slices (the kernel has no static arrays)
static size_t stream_lds_bytes(uint32_t dim) {
    const uint32_t dimp = (dim + 3u) & ~3u;
    return ((size_t)kStQT * dimp + 4u * 64u * kStLd) * sizeof(float);
}

// streaming kernel: a few queries (at most 16, one database pass per 8), 16-byte-loadable rows, and a dim whose
// queries fit the LDS beside the staging slices (up to 3968; wider rows take bf_generic_kernel: the same arithmetic)
static bool stream_eligible(const BfIndexDev &ix, const BfPass &p) {
    if (ix.measure > SCANN_HIP_DOT_PRODUCT) return false;   // L1 / Cosine: the pair-at-a-time kernel
    if ((ix.stride & 3u) || (reinterpret_cast<uintptr_t>(ix.rows) & 15u) || ix.dim < 8) return false;
    if (stream_lds_bytes(ix.dim) > kMaxLdsBytes) return false;
    return p.nq <= 16;
}

template <int FMT, int QT>
static int launch_quant(const BfIndexDev &ix, const BfPass &p, hipStream_t st) {
    const size_t lds = (size_t)ix.dim * QT * sizeof(float);
    const dim3 grid(ceil_div_u32(p.nrows, 256), ceil_div_u32(p.nq, QT));
    if (ix.measure > SCANN_HIP_DOT_PRODUCT)
        return fail(SCANN_HIP_UNIMPLEMENTED, "quantized rows: SquaredL2, L2 and DotProduct only");
    return with_dot_measure(ix.measure, [&](auto m) {
        return launch((bf_quant_kernel<FMT, m(), QT>), grid, dim3(256), lds, st, ix, p);
    });
}

// quantized rows: every pass (sample, filter, dense matrix, radius) on bf_quant_kernel; one query pair per
// workgroup row for the one- and two-query searches, four pairs otherwise
static int launch_quant_pass(const BfIndexDev &ix, const BfPass &p, hipStream_t st) {
    // (one pair too where four pairs of queries exceed the LDS, dim > 5120: the same arithmetic per pair of values)
    const bool few = p.nq <= 2 || (size_t)ix.dim * 8 * sizeof(float) > kMaxLdsBytes;
    if (ix.fmt != SCANN_HIP_ROWS_BF16 && ix.fmt != SCANN_HIP_ROWS_FP8_E4M3 && ix.fmt != SCANN_HIP_ROWS_INT8)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "unknown row format");
    return with_value<SCANN_HIP_ROWS_BF16, SCANN_HIP_ROWS_FP8_E4M3, SCANN_HIP_ROWS_INT8>(ix.fmt, [&](auto fmt) {
        return few ? launch_quant<fmt(), 2>(ix, p, st) : launch_quant<fmt(), 8>(ix, p, st);
    });
}

// name of the kernel launch_pass picks for a batch of nq queries (timing reports)
const char *bf_pass_kernel_name(const BfIndexDev &ix, uint32_t nq) {
    if (ix.fmt) return "bf_quant_kernel";
    BfPass p{};
    p.nq = nq;
    if (stream_eligible(ix, p)) return "bf_stream_kernel";
    if (mfma_eligible(ix)) return "bf_mfma_dot_kernel";
    if (vq_eligible(ix, p)) return "bf_vq_kernel";
    return "bf_generic_kernel";
}

// LDS of bf_generic_kernel, the pass every f32 search can end in (no static arrays)
static size_t generic_lds_bytes(uint32_t dim) {
    const uint32_t dimp = (dim + 3u) & ~3u;
    return ((size_t)kBfGenQT * dimp + kBfGenQT) * sizeof(float);
}

bool bf_pass_fits(const BfIndexDev &ix) {
    return ix.fmt ? (size_t)ix.dim * 2 * sizeof(float) <= kMaxLdsBytes : generic_lds_bytes(ix.dim) <= kMaxLdsBytes;
}

static int launch_pass(const BfIndexDev &ix, const BfPass &p, hipStream_t st) {
    if (p.nq == 0 || p.nrows == 0) return SCANN_HIP_OK;
    if (ix.fmt) return launch_quant_pass(ix, p, st);
    if (stream_eligible(ix, p)) {
        const size_t lds = stream_lds_bytes(ix.dim);
        const uint32_t ny = ceil_div_u32(p.nq, kStQT);
        const uint32_t ngroups = ceil_div_u32(p.nrows, 64);
        const uint32_t nx = std::max(1u, std::min(ceil_div_u32(ngroups, 4), 4u * (uint32_t)num_cus()));
        dim3 grid(nx, ny);
        return with_dot_measure(ix.measure, [&](auto m) {
            return launch(bf_stream_kernel<m()>, grid, dim3(256), lds, st, ix, p);
        });
    }
    if (mfma_eligible(ix)) return with_dim16(ix.dim, [&](auto ts) { return launch_mfma<ts()>(ix, p, st); });
    if (vq_eligible(ix, p)) {
        const uint32_t ny = ceil_div_u32(p.nq, 256);
        const uint32_t ntiles = ceil_div_u32(p.nrows, kVqRows);
        const uint32_t nx = std::max(1u, std::min(ntiles, (2u * (uint32_t)num_cus() + ny - 1) / ny));
        return with_value<SCANN_HIP_L2, SCANN_HIP_SQUARED_L2>(ix.measure, [&](auto m) {
            return with_dim8(ix.dim, [&](auto dcv) {
                return launch((bf_vq_kernel<m(), dcv()>), dim3(nx * ny), dim3(256), 0, st, ix, p, nx);
            });
        });
    }
    const size_t lds = generic_lds_bytes(ix.dim);
    dim3 grid(ceil_div_u32(p.nrows, 256), ceil_div_u32(p.nq, kBfGenQT));
    return with_measure(ix.measure, [&](auto m) {
        return launch(bf_generic_kernel<m()>, grid, dim3(256), lds, st, ix, p);
    });
}

struct BfPlan {
    uint32_t n, k, ns, rs, cap;
    bool direct;
};

// n: the rows the passes run over -- ix.n, or the allowed count A of a compacted filtered search
static int make_plan(uint32_t n, uint32_t k, bool full_cap, BfPlan *pl) {
    k = std::min(k, n);  // brute_force/searcher.rs:91
    if (k > kBfMaxK)
        return fail(SCANN_HIP_UNIMPLEMENTED, "k > " + std::to_string(kBfMaxK) + " on the GPU path");
    pl->n = n;
    pl->k = k;
    pl->direct = n <= kBfSampleRows;
    pl->ns = std::min(n, kBfSampleRows);
    pl->rs = pl->direct ? 1u : n / kBfSampleRows;
    const uint64_t cap = full_cap ? n : std::min<uint64_t>(n, 2ull * k * pl->rs + 16ull * pl->rs + 256ull);
    pl->cap = (uint32_t)cap;
    return SCANN_HIP_OK;
}

static int ensure_ws(const BfIndexDev &ix, BfWorkspace &w, uint32_t nq, const BfPlan &pl,
                     bool own_q, uint32_t q_stride, bool own_out) {
    (void)ix;
    if (own_q) SCANN_TRY(w.queries.ensure((size_t)nq * q_stride * 4));
    SCANN_TRY(w.sample.ensure((size_t)nq * pl.ns * 4));
    SCANN_TRY(w.thr.ensure((size_t)nq * 8));
    SCANN_TRY(w.cand_cnt.ensure((size_t)nq * 4));
    if (!pl.direct) SCANN_TRY(w.cand.ensure((size_t)nq * pl.cap * 8));
    SCANN_TRY(w.counters.ensure(BF_CNT_N * 4));
    if (own_out) {
        SCANN_TRY(w.out_idx.ensure((size_t)nq * std::max(1u, pl.k) * 4));
        SCANN_TRY(w.out_dist.ensure((size_t)nq * std::max(1u, pl.k) * 4));
        SCANN_TRY(w.out_count.ensure((size_t)nq * 4));
    }
    return SCANN_HIP_OK;
}

// What a pass needs of the allow-list, on the device.  ids: compacted form (nrows = allowed count); allow: bit test.
struct BfFilterDev {
    const uint32_t *ids = nullptr;
    const uint64_t *allow = nullptr;
    uint32_t allow_bits = 0;
};

uint64_t bf_allowed_count(const uint64_t *bitmap, uint64_t bits, uint64_t n) {
    const uint64_t eff = std::min(bits, n);
    uint64_t count = 0;
    for (uint64_t w = 0; w * 64 < eff; ++w) {
        const uint64_t rem = eff - w * 64;
        count += (uint64_t)__builtin_popcountll(rem >= 64 ? bitmap[w] : (bitmap[w] & ((1ull << rem) - 1ull)));
    }
    return count;
}

// Host bitmap -> workspace copy (and, compacted form, the id list of its `count` allowed rows).
static int upload_filter(const BfIndexDev &ix, BfWorkspace &w, const BfFilter &f, bool compact, uint32_t count,
                         BfFilterDev *fd, hipStream_t st) {
    const uint32_t bits = (uint32_t)std::min<uint64_t>(f.bits, ix.n);
    const size_t words = ((size_t)bits + 63) / 64;
    SCANN_TRY(w.allow.ensure(std::max<size_t>(words, 1) * 8));
    if (words) SCANN_HIP_CHECK(hipMemcpyAsync(w.allow.p, f.bitmap, words * 8, hipMemcpyHostToDevice, st));
    fd->allow = w.allow.as<uint64_t>();
    fd->allow_bits = bits;
    if (!compact) return SCANN_HIP_OK;
    const uint32_t blocks = std::max(1u, ceil_div_u32((uint32_t)words, kCompactWords));
    SCANN_TRY(w.ids.ensure(std::max<size_t>(count, 1) * 4));
    SCANN_TRY(w.allow_sums.ensure((size_t)(blocks + 1) * 4));
    uint32_t *sums = w.allow_sums.as<uint32_t>();
    SCANN_TRY(launch(bf_allow_count_kernel, dim3(blocks), dim3(kCompactWords), 0, st, fd->allow, bits, sums));
    SCANN_TRY(launch(bf_allow_compact_kernel, dim3(blocks), dim3(kCompactWords), 0, st, fd->allow, bits, sums,
                     w.ids.as<uint32_t>(), count, sums + blocks));
    fd->ids = w.ids.as<uint32_t>();
    fd->allow = nullptr;   // every listed row is allowed
    fd->allow_bits = 0;
    return SCANN_HIP_OK;
}

int bf_reserve(const BfIndexDev &ix, BfWorkspace &w, uint32_t max_nq, uint32_t max_k, bool filtered) {
    if (ix.n == 0) return SCANN_HIP_OK;
    BfPlan pl;
    SCANN_TRY(make_plan((uint32_t)ix.n, max_k, false, &pl));
    if (filtered) {   // host entries: bitmap copy, id list, block sums (the device entry reads the caller's bitmap)
        const size_t words = ((size_t)ix.n + 63) / 64;
        SCANN_TRY(w.allow.ensure(words * 8));
        SCANN_TRY(w.ids.ensure((size_t)ix.n * 4));
        SCANN_TRY(w.allow_sums.ensure((size_t)(ceil_div_u32((uint32_t)words, kCompactWords) + 1) * 4));
    }
    return ensure_ws(ix, w, max_nq, pl, false, 0, false);
}

// k_out: row pitch of the caller's output arrays (the caller's k, >= pl.k).
// fd: the allow-list; compacted form: pl was made for its allowed count and the passes run over fd.ids.
static int enqueue_search(const BfIndexDev &ix, BfWorkspace &w, const BfPlan &pl, const BfFilterDev &fd,
                          const float *d_queries, uint32_t nq, uint32_t q_stride,
                          uint32_t *d_out_idx, float *d_out_dist, uint32_t *d_out_count,
                          hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
    SCANN_HIP_CHECK(hipMemsetAsync(w.counters.p, 0, BF_CNT_N * 4, st));
    BfPass a{};
    a.queries = d_queries;
    a.nq = nq;
    a.q_stride = q_stride;
    a.nrows = pl.ns;
    a.row_mult = pl.rs;
    a.filter = 0;
    a.out = w.sample.as<float>();
    a.ld = pl.ns;
    a.ids = fd.ids;
    a.allow = fd.allow;
    a.allow_bits = fd.allow_bits;
    if (pl.direct && ev0) SCANN_HIP_CHECK(hipEventRecord(ev0, st));
    SCANN_TRY(launch_pass(ix, a, st));
    if (pl.direct && ev1) SCANN_HIP_CHECK(hipEventRecord(ev1, st));
    const SelCfg tcfg = sel_cfg(pl.ns);
    const size_t lds_thr = (size_t)next_pow2_u32(pl.ns) * 8 + (size_t)tcfg.bins * 4 + (size_t)tcfg.list * 8 + 48 * 8;
    SCANN_TRY(launch(bf_threshold_kernel, dim3(nq), dim3(kBfSelectThreads), lds_thr, st,
                     w.sample.as<float>(), pl.ns, pl.rs, pl.k, pl.direct ? 1 : 0,
                     w.thr.as<uint64_t>(), d_out_idx, d_out_dist, d_out_count, fd.ids, fd.allow, fd.allow_bits));
    if (pl.direct) return SCANN_HIP_OK;

    SCANN_HIP_CHECK(hipMemsetAsync(w.cand_cnt.p, 0, (size_t)nq * 4, st));
    BfPass b = a;
    b.nrows = fd.ids ? pl.n : (uint32_t)ix.n;
    b.row_mult = 1;
    b.filter = 1;
    b.out = nullptr;
    b.ld = 0;
    b.thr = w.thr.as<uint64_t>();
    b.cand_cnt = w.cand_cnt.as<uint32_t>();
    b.cand = w.cand.as<uint64_t>();
    b.cap = pl.cap;
    if (ev0) SCANN_HIP_CHECK(hipEventRecord(ev0, st));
    SCANN_TRY(launch_pass(ix, b, st));
    if (ev1) SCANN_HIP_CHECK(hipEventRecord(ev1, st));
    const SelCfg scfg = sel_cfg(kBfSortCap);
    const size_t lds_sel = (size_t)kBfSortCap * 8 + (kBfSelectThreads / 64 + 4) * 4 + (size_t)kBfMaxK * 8 +
                           (size_t)scfg.bins * 4 + (size_t)scfg.list * 8 + 48 * 8;
    SCANN_TRY(launch(bf_select_kernel, dim3(nq), dim3(kBfSelectThreads), lds_sel, st, pl.k, pl.cap,
                     w.cand_cnt.as<uint32_t>(), w.cand.as<uint64_t>(), w.counters.as<uint32_t>(),
                     d_out_idx, d_out_dist, d_out_count));
    return SCANN_HIP_OK;
}

// ---- bf16 shortlist path --------------------------------------------------------------------
static bool shortlist_dims_ok(uint32_t dim) {
    switch (dim) {
        case 32: case 64: case 96: case 128: case 192: case 256: return true;
        default: return false;
    }
}

int bf_build_shortlist_data(const BfIndexDev &ix, DevBuf &rows_b, DevBuf &rows_bl, DevBuf &norm2,
                            float *max_norm, hipStream_t st) {
    *max_norm = 0.0f;
    if (ix.n == 0 || !shortlist_dims_ok(ix.dim)) return SCANN_HIP_OK;
    // SCANN_HIP_BF_SHORTLIST_MIN_ROWS: below this the exact kernels are fast enough (tests set 1)
    if (ix.n < read_knobs().bf_shortlist_min_rows) return SCANN_HIP_OK;
    if (ix.measure > SCANN_HIP_DOT_PRODUCT) return SCANN_HIP_OK;   // L1 / Cosine: no bf16 bound is derived for them
    // quantized rows: the pass reads 8 elements per load (stride % 8) and needs only the norms, no row copy
    if (ix.fmt && ((ix.stride & 7u) || (reinterpret_cast<uintptr_t>(ix.qrows) & 15u))) return SCANN_HIP_OK;
    if (!ix.fmt) {
        SCANN_TRY(rows_b.ensure((size_t)ix.n * ix.dim * 2));
        SCANN_TRY(rows_bl.ensure((size_t)ix.n * ix.dim * 2));
    }
    SCANN_TRY(norm2.ensure((size_t)ix.n * 4));
    DevBuf mx;
    SCANN_TRY(mx.ensure(4));
    SCANN_HIP_CHECK(hipMemsetAsync(mx.p, 0, 4, st));
    const dim3 grid_n((uint32_t)ceil_div_u64(ix.n, 256));
    SCANN_TRY(with_row_format(ix.fmt, [&](auto fmt) {
        if constexpr (fmt() != 0)
            return launch(bf_quant_norms_kernel<fmt()>, grid_n, dim3(256), 0, st, ix, norm2.as<float>());
        else
            return launch(bf_to_bf16_kernel, grid_n, dim3(256), 0, st, ix.rows, ix.n, ix.dim, ix.stride,
                          rows_b.as<uint16_t>(), rows_bl.as<uint16_t>(), norm2.as<float>());
    }));
    SCANN_TRY(launch(bf_max_norm_kernel, dim3(256), dim3(256), 0, st, norm2.as<float>(), ix.n,
                     mx.as<uint32_t>()));
    uint32_t bits = 0;
    SCANN_HIP_CHECK(hipMemcpyAsync(&bits, mx.p, 4, hipMemcpyDeviceToHost, st));
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    float m2;
    std::memcpy(&m2, &bits, 4);
    *max_norm = std::sqrt(m2) * 1.000001f;
    return SCANN_HIP_OK;
}

// shortlist size: 4k, at least 32, at most kShortMax
static uint32_t shortlist_size(uint32_t k) { return std::min(kShortMax, std::max(32u, 4u * k)); }

bool bf_shortlist_eligible(const BfIndexDev &ix, uint32_t nq, uint32_t k, const Knobs &kn) {
    if (!ix.norm2 || (!ix.fmt && (!ix.rows_b || !ix.rows_bl))) return false;   // quantized rows: norms only
    if (!(ix.max_norm == ix.max_norm) || std::isinf(ix.max_norm)) return false;
    if (k == 0 || 4u * k > kShortMax) return false;
    if ((uint64_t)shortlist_size(k) * 8 > ix.n) return false;   // a shortlist that is most of the data
    return nq >= kn.bf_shortlist_min_queries;
}

template <int TS, int FMT>
static int launch_bf16(const BfIndexDev &ix, const BfPass &p, const uint16_t *qb, const uint16_t *qbl,
                       const float *qn2, hipStream_t st) {
    const uint32_t ny = ceil_div_u32(p.nq, kB16Waves * 32);
    const uint32_t ntiles = ceil_div_u32(p.nrows, 32 * kB16Sub);
    uint32_t want = std::max<uint32_t>(1, ((uint32_t)(TS <= 8 ? kB16Occ : 2) * (uint32_t)num_cus()) / ny);
    want = std::min(want, ntiles);
    const uint32_t nx = 8u * ceil_div_u32(want, 8);
    const size_t lds = (size_t)kB16Ring * (2 * 32 * kB16Sub * (TS * 16) * 2 + 256) +   // (hi | lo | norms) stages
                       16;
    return with_value<SCANN_HIP_DOT_PRODUCT, SCANN_HIP_SQUARED_L2>(ix.measure, [&](auto m) {
        return launch((bf_bf16_kernel<TS, m(), FMT>), dim3(nx * ny), dim3(kB16Waves * 64), lds, st, ix, p, qb, qbl, qn2,
                      nx, ny);
    });
}

static int launch_bf16_pass(const BfIndexDev &ix, const BfPass &p, const uint16_t *qb, const uint16_t *qbl,
                            const float *qn2, hipStream_t st) {
    return with_row_format(ix.fmt, [&](auto fmt) {
        return with_dim16(ix.dim, [&](auto ts) { return launch_bf16<ts(), fmt()>(ix, p, qb, qbl, qn2, st); });
    });
}

// exact re-score of the shortlist of quantized rows (SquaredL2 serves L2: the final kernel takes the root)
template <int MEASURE>
static int launch_rerank(const BfIndexDev &ix, const float *d_queries, uint32_t q_stride, uint32_t kp, BfWorkspace &w,
                         uint32_t nq, hipStream_t st) {
    return with_row_format(ix.fmt, [&](auto fmt) {
        if constexpr (fmt() != 0)
            return launch((bf_quant_rerank_kernel<fmt(), MEASURE>), dim3(ceil_div_u32(kp, 256), nq), dim3(256),
                          (size_t)ix.dim * 4, st, ix, d_queries, q_stride, kp, w.sl_idx.as<uint32_t>(),
                          w.sl_cnt.as<uint32_t>(), w.sl_exact.as<float>());
        else
            return launch(bf_rerank_kernel<MEASURE>, dim3(ceil_div_u32(kp, 32), nq), dim3(256), (size_t)ix.dim * 4, st,
                          ix, d_queries, q_stride, kp, w.sl_idx.as<uint32_t>(), w.sl_cnt.as<uint32_t>(),
                          w.sl_exact.as<float>());
    });
}

// bf16 scores -> shortlist of kp rows -> exact re-score -> first k + verification
static int enqueue_shortlist_search(const BfIndexDev &ix, BfWorkspace &w, uint32_t k, double tail, const float *d_queries,
                                    uint32_t nq, uint32_t q_stride, uint32_t *d_out_idx, float *d_out_dist,
                                    uint32_t *d_out_count, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
    const uint32_t n = (uint32_t)ix.n, kp = shortlist_size(k);
    const uint32_t ns = std::min(n, kBfSampleRows), rs = n / ns;
    const uint32_t cap = (uint32_t)std::min<uint64_t>(n, 2ull * kp * rs + 16ull * rs + 256ull);
    SCANN_TRY(w.q_b.ensure((size_t)nq * ix.dim * 2));
    SCANN_TRY(w.q_bl.ensure((size_t)nq * ix.dim * 2));
    SCANN_TRY(w.sl_fail.ensure((size_t)nq * 4));
    SCANN_TRY(w.q_n2.ensure((size_t)nq * 4));
    SCANN_TRY(w.sample.ensure((size_t)nq * ns * 4));
    SCANN_TRY(w.thr.ensure((size_t)nq * 8));
    SCANN_TRY(w.cand_cnt.ensure((size_t)nq * 4));
    SCANN_TRY(w.cand.ensure((size_t)nq * cap * 8));
    SCANN_TRY(w.counters.ensure(BF_CNT_N * 4));
    SCANN_TRY(w.sl_idx.ensure((size_t)nq * kp * 4));
    SCANN_TRY(w.sl_approx.ensure((size_t)nq * kp * 4));
    SCANN_TRY(w.sl_exact.ensure((size_t)nq * kp * 4));
    SCANN_TRY(w.sl_cnt.ensure((size_t)nq * 4));
    SCANN_HIP_CHECK(hipMemsetAsync(w.counters.p, 0, BF_CNT_N * 4, st));
    SCANN_HIP_CHECK(hipMemsetAsync(w.cand_cnt.p, 0, (size_t)nq * 4, st));
    SCANN_TRY(launch(bf_q_prep_kernel, dim3(ceil_div_u32(nq, 4)), dim3(256), 0, st, d_queries, nq, ix.dim,
                     q_stride, w.q_b.as<uint16_t>(), w.q_bl.as<uint16_t>(), w.q_n2.as<float>()));
    // 1. bf16 scores of an evenly spaced sample -> bound of the kp-th best bf16 score
    BfPass a{};
    a.queries = d_queries;
    a.nq = nq;
    a.q_stride = q_stride;
    a.nrows = ns;
    a.row_mult = rs;
    a.filter = 0;
    a.out = w.sample.as<float>();
    a.ld = ns;
    SCANN_TRY(launch_bf16_pass(ix, a, w.q_b.as<uint16_t>(), w.q_bl.as<uint16_t>(), w.q_n2.as<float>(), st));
    const SelCfg tcfg = sel_cfg(ns);
    const size_t lds_thr = (size_t)next_pow2_u32(ns) * 8 + (size_t)tcfg.bins * 4 + (size_t)tcfg.list * 8 + 48 * 8;
    // Sample rank of the filter bound.  The kp-th smallest sample score is a certain bound of the
    // kp-th smallest score overall but lets ~kp * rs rows through; the j-th smallest with
    // P(Poisson(kp / rs) >= j) <= 1e-6 -- the chance that j of the overall best kp fell into the
    // 1-in-rs sample -- lets ~j * rs through.  Should it cut deeper, the shortlist is merely shorter
    // than kp and the final kernel proves the result against the bound itself (or flags the query).
    uint32_t jthr = kp;
    {   // (tail: SCANN_HIP_BF_SHORTLIST_TAIL, read per call: tests force the short-shortlist paths through it)
        const double lam = (double)kp / (double)rs;
        double term = std::exp(-lam), cdf = term;   // P(X <= 0)
        for (uint32_t j = 1; j < kp; ++j) {         // smallest j with P(X >= j) = 1 - P(X <= j-1) <= 1e-6
            if (1.0 - cdf <= tail) { jthr = j; break; }
            term *= lam / (double)j;
            cdf += term;
        }
    }
    SCANN_TRY(launch(bf_threshold_kernel, dim3(nq), dim3(kBfSelectThreads), lds_thr, st, w.sample.as<float>(),
                     ns, rs, jthr, 0, w.thr.as<uint64_t>(), (uint32_t *)nullptr, (float *)nullptr,
                     (uint32_t *)nullptr, (const uint32_t *)nullptr, (const uint64_t *)nullptr, 0u));
    // 2. bf16 scores of every row, filtered by that bound
    BfPass b = a;
    b.nrows = n;
    b.row_mult = 1;
    b.filter = 1;
    b.out = nullptr;
    b.ld = 0;
    b.thr = w.thr.as<uint64_t>();
    b.cand_cnt = w.cand_cnt.as<uint32_t>();
    b.cand = w.cand.as<uint64_t>();
    b.cap = cap;
    if (ev0) SCANN_HIP_CHECK(hipEventRecord(ev0, st));
    SCANN_TRY(launch_bf16_pass(ix, b, w.q_b.as<uint16_t>(), w.q_bl.as<uint16_t>(), w.q_n2.as<float>(), st));
    if (ev1) SCANN_HIP_CHECK(hipEventRecord(ev1, st));
    // 3. the kp best bf16 scores (sorted): the shortlist
    const SelCfg scfg = sel_cfg(kBfSortCap);
    const size_t lds_sel = (size_t)kBfSortCap * 8 + (kBfSelectThreads / 64 + 4) * 4 + (size_t)kBfMaxK * 8 +
                           (size_t)scfg.bins * 4 + (size_t)scfg.list * 8 + 48 * 8;
    SCANN_TRY(launch(bf_select_kernel, dim3(nq), dim3(kBfSelectThreads), lds_sel, st, kp, cap,
                     w.cand_cnt.as<uint32_t>(), w.cand.as<uint64_t>(), w.counters.as<uint32_t>(),
                     w.sl_idx.as<uint32_t>(), w.sl_approx.as<float>(), w.sl_cnt.as<uint32_t>()));
    // 4. exact f32 score of the shortlist, 5. first k + verification
    const float err = ix.fmt ? shortlist_quant_err(ix.dim, ix.fmt) : shortlist_dot_err(ix.dim);
    return with_value<SCANN_HIP_DOT_PRODUCT, SCANN_HIP_L2, SCANN_HIP_SQUARED_L2>(ix.measure, [&](auto m) {
        constexpr int kRerank = m() == SCANN_HIP_DOT_PRODUCT ? SCANN_HIP_DOT_PRODUCT : SCANN_HIP_SQUARED_L2;
        SCANN_TRY(launch_rerank<kRerank>(ix, d_queries, q_stride, kp, w, nq, st));
        return launch(bf_shortlist_final_kernel<m()>, dim3(nq), dim3(64), 0, st, n, k, kp, ix.max_norm, err,
                      w.q_n2.as<float>(), w.thr.as<uint64_t>(), w.sl_idx.as<uint32_t>(), w.sl_approx.as<float>(),
                      w.sl_cnt.as<uint32_t>(), w.sl_exact.as<float>(), w.counters.as<uint32_t>(),
                      w.sl_fail.as<uint32_t>(), d_out_idx, d_out_dist, d_out_count);
    });
}

int bf_last_status(const BfWorkspace &w, hipStream_t st) {
    if (!w.counters.p) return SCANN_HIP_OK;
    uint32_t counters[BF_CNT_N];
    SCANN_HIP_CHECK(hipMemcpyAsync(counters, w.counters.p, sizeof(counters), hipMemcpyDeviceToHost, st));
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    if (counters[BF_CNT_STATUS] == SCANN_HIP_ABORTED)
        return fail(SCANN_HIP_ABORTED, "a bf16-shortlist result could not be verified: repeat the batch with "
                                       "opts.bf_exact = 1 (the host entry point does it itself)");
    if (counters[BF_CNT_STATUS] != SCANN_HIP_OK)
        return fail((int)counters[BF_CNT_STATUS], "candidate buffer overflow on the device path (use the host "
                                                  "entry point, which retries with a full-size buffer)");
    return SCANN_HIP_OK;
}

int bf_search_device(const BfIndexDev &ix, BfWorkspace &w, const float *d_queries, uint32_t nq,
                     uint32_t q_stride, uint32_t k, bool shortlist, double tail, const BfFilter &flt,
                     uint32_t *d_out_idx, float *d_out_dist,
                     uint32_t *d_out_count, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
    if (ix.n == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "empty dataset on the device path");
    BfPlan pl;
    SCANN_TRY(make_plan((uint32_t)ix.n, k, false, &pl));
    if (pl.k != k)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "k > dataset size on the device path (row pitch)");
    BfFilterDev fd;
    if (flt.bitmap) {   // bit test at the emit: the allowed count is not known without a synchronisation
        fd.allow = flt.bitmap;
        fd.allow_bits = (uint32_t)std::min<uint64_t>(flt.bits, ix.n);
        shortlist = false;
    }
    if (shortlist)
        return enqueue_shortlist_search(ix, w, k, tail, d_queries, nq, q_stride, d_out_idx, d_out_dist, d_out_count, st,
                                        ev0, ev1);
    SCANN_TRY(ensure_ws(ix, w, nq, pl, false, q_stride, false));
    return enqueue_search(ix, w, pl, fd, d_queries, nq, q_stride, d_out_idx, d_out_dist, d_out_count, st,
                          ev0, ev1);
}

int bf_search_host(const BfIndexDev &ix, BfWorkspace &w, const float *queries, uint32_t nq,
                   uint32_t q_stride, uint32_t k, bool shortlist, double tail, const BfFilter &flt, uint32_t *out_idx,
                   float *out_dist, uint32_t *out_count, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
    // Filtered search: the answer of an unfiltered search over the allowed rows alone.  The allowed count A comes
    // from the host bitmap; the bf16 shortlist is not taken (its proof would have to hold over allowed rows only).
    uint32_t allowed = (uint32_t)ix.n;
    bool compact = false;
    if (flt.bitmap) {
        allowed = (uint32_t)bf_allowed_count(flt.bitmap, flt.bits, ix.n);
        shortlist = false;
        if (allowed == 0) {
            for (size_t i = 0; i < (size_t)nq * k; ++i) {
                out_idx[i] = kBfInvalid;
                out_dist[i] = INFINITY;
            }
            for (uint32_t q = 0; q < nq; ++q) out_count[q] = 0;
            return SCANN_HIP_OK;
        }
        compact = flt.mechanism == 1 || (flt.mechanism == 0 && (double)allowed <= flt.compact_max_fraction * (double)ix.n);
    }
    // attempt 0: bf16 shortlist (if the search qualifies); 1: exact kernels; 2: exact, full buffers (a filtered
    // search whose bit-test pass overflowed -- too few allowed rows in the sample for a bound -- repeats compacted)
    for (int attempt = shortlist ? 0 : 1; attempt < 3; ++attempt) {
        if (attempt == 2 && flt.bitmap && flt.mechanism != 2) compact = true;
        BfPlan pl;
        SCANN_TRY(make_plan(compact ? allowed : (uint32_t)ix.n, std::min(k, allowed), attempt == 2, &pl));
        SCANN_TRY(ensure_ws(ix, w, nq, pl, true, q_stride, true));
        BfFilterDev fd;
        if (flt.bitmap) SCANN_TRY(upload_filter(ix, w, flt, compact, allowed, &fd, st));
        SCANN_HIP_CHECK(hipMemcpyAsync(w.queries.p, queries, (size_t)nq * q_stride * 4,
                                       hipMemcpyHostToDevice, st));
        if (attempt == 0)
            SCANN_TRY(enqueue_shortlist_search(ix, w, k, tail, w.queries.as<float>(), nq, q_stride,
                                               w.out_idx.as<uint32_t>(), w.out_dist.as<float>(),
                                               w.out_count.as<uint32_t>(), st, ev0, ev1));
        else
            SCANN_TRY(enqueue_search(ix, w, pl, fd, w.queries.as<float>(), nq, q_stride,
                                     w.out_idx.as<uint32_t>(), w.out_dist.as<float>(),
                                     w.out_count.as<uint32_t>(), st, ev0, ev1));
        uint32_t counters[BF_CNT_N];
        SCANN_HIP_CHECK(hipMemcpyAsync(counters, w.counters.p, sizeof(counters), hipMemcpyDeviceToHost, st));
        std::vector<uint32_t> ti((size_t)nq * pl.k);
        std::vector<float> td((size_t)nq * pl.k);
        SCANN_HIP_CHECK(hipMemcpyAsync(ti.data(), w.out_idx.p, ti.size() * 4, hipMemcpyDeviceToHost, st));
        SCANN_HIP_CHECK(hipMemcpyAsync(td.data(), w.out_dist.p, td.size() * 4, hipMemcpyDeviceToHost, st));
        SCANN_HIP_CHECK(hipMemcpyAsync(out_count, w.out_count.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
        SCANN_HIP_CHECK(hipStreamSynchronize(st));
        if (counters[BF_CNT_STATUS] == SCANN_HIP_OK) {
            for (uint32_t q = 0; q < nq; ++q)       // caller's rows have pitch k
                for (uint32_t i = 0; i < k; ++i) {
                    out_idx[(size_t)q * k + i] = i < pl.k ? ti[(size_t)q * pl.k + i] : kBfInvalid;
                    out_dist[(size_t)q * k + i] = i < pl.k ? td[(size_t)q * pl.k + i] : INFINITY;
                }
            return SCANN_HIP_OK;
        }
        if (attempt == 0 && counters[BF_CNT_STATUS] == SCANN_HIP_ABORTED) {
            // shortlist results that could not be proven exact: only those queries go through the
            // exact kernels again
            std::vector<uint32_t> flags(nq);
            SCANN_HIP_CHECK(hipMemcpy(flags.data(), w.sl_fail.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
            std::vector<uint32_t> redo;
            for (uint32_t q = 0; q < nq; ++q) {
                if (flags[q]) {
                    redo.push_back(q);
                    continue;
                }
                for (uint32_t i = 0; i < k; ++i) {
                    out_idx[(size_t)q * k + i] = i < pl.k ? ti[(size_t)q * pl.k + i] : kBfInvalid;
                    out_dist[(size_t)q * k + i] = i < pl.k ? td[(size_t)q * pl.k + i] : INFINITY;
                }
            }
            const uint32_t nr = (uint32_t)redo.size();
            std::vector<float> sub((size_t)nr * q_stride);
            for (uint32_t r = 0; r < nr; ++r)
                std::memcpy(&sub[(size_t)r * q_stride], queries + (size_t)redo[r] * q_stride, (size_t)q_stride * 4);
            std::vector<uint32_t> ri((size_t)nr * k), rc(nr);
            std::vector<float> rd((size_t)nr * k);
            SCANN_TRY(bf_search_host(ix, w, sub.data(), nr, q_stride, k, false, tail, BfFilter{}, ri.data(), rd.data(),
                                     rc.data(), st, nullptr, nullptr));
            for (uint32_t r = 0; r < nr; ++r) {
                std::memcpy(out_idx + (size_t)redo[r] * k, &ri[(size_t)r * k], (size_t)k * 4);
                std::memcpy(out_dist + (size_t)redo[r] * k, &rd[(size_t)r * k], (size_t)k * 4);
                out_count[redo[r]] = rc[r];
            }
            return SCANN_HIP_OK;
        }
        const bool retry = (attempt == 0) || (attempt == 1 && counters[BF_CNT_STATUS] == SCANN_HIP_RESOURCE_EXHAUSTED);
        if (!retry) return fail((int)counters[BF_CNT_STATUS], "device reported a search failure");
    }
    return fail(SCANN_HIP_INTERNAL, "unreachable");
}

int bf16_quantize_host(const float *values, uint64_t n, uint16_t *out_bits, hipStream_t st) {
    if (n == 0) return SCANN_HIP_OK;
    DevBuf dv, dout;
    SCANN_TRY(upload(dv, values, (size_t)n * 4));
    SCANN_TRY(dout.ensure((size_t)n * 2));
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(ceil_div_u64(n, 256), 65535);
    SCANN_TRY(launch(bf16_quantize_kernel, dim3(blocks), dim3(256), 0, st, dv.as<float>(), n, dout.as<uint16_t>()));
    SCANN_HIP_CHECK(hipMemcpyAsync(out_bits, dout.p, (size_t)n * 2, hipMemcpyDeviceToHost, st));
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    return SCANN_HIP_OK;
}

int bf_distances_host(const BfIndexDev &ix, BfWorkspace &w, const float *queries, uint32_t nq,
                      uint32_t q_stride, float *out, hipStream_t st) {
    DevBuf dq, dout;
    (void)w;
    SCANN_TRY(upload(dq, queries, (size_t)nq * q_stride * 4));
    SCANN_TRY(dout.ensure((size_t)nq * ix.n * 4));
    BfPass a{};
    a.queries = dq.as<float>();
    a.nq = nq;
    a.q_stride = q_stride;
    a.nrows = (uint32_t)ix.n;
    a.row_mult = 1;
    a.filter = 0;
    a.out = dout.as<float>();
    a.ld = (uint32_t)ix.n;
    SCANN_TRY(launch_pass(ix, a, st));
    SCANN_HIP_CHECK(hipMemcpyAsync(out, dout.p, (size_t)nq * ix.n * 4, hipMemcpyDeviceToHost, st));
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    return SCANN_HIP_OK;
}

// BruteForceSearcher::search_radius (brute_force/searcher.rs:142-167): every datapoint with
// distance <= radius, stable-sorted by distance (key order = (distance, index)).  The filter
// pass of the search keeps keys <= (radius, max index); a device radix sort orders them.
__global__ void bf_decode_keys_kernel(const uint64_t *__restrict__ keys, uint32_t n,
                                      uint32_t *__restrict__ out_idx, float *__restrict__ out_dist) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = keys[i];
    out_idx[i] = (uint32_t)key;
    out_dist[i] = ordered_to_f32((uint32_t)(key >> 32));
}

int bf_search_radius_host(const BfIndexDev &ix, BfWorkspace &w, const float *query, uint32_t q_stride,
                          float radius, const BfFilter &flt, uint32_t *out_idx, float *out_dist, uint64_t capacity,
                          uint64_t *out_count, hipStream_t st) {
    const uint32_t n = (uint32_t)ix.n;
    DevBuf dq, dthr, dcnt, dcand, dsorted, dtmp, didx, ddist;
    SCANN_TRY(upload(dq, query, (size_t)q_stride * 4));
    // NaN radius: nothing compares <= NaN (searcher.rs:161)
    const uint64_t T = (radius != radius) ? 0ull : (((uint64_t)f32_to_ordered(radius) << 32) | 0xFFFFFFFFull);
    if (radius != radius) {
        *out_count = 0;
        return SCANN_HIP_OK;
    }
    // allow-list: the same pass over the allowed rows only (compacted id list), or with the bit test at the emit
    uint32_t allowed = n;
    BfFilterDev fd;
    if (flt.bitmap) {
        allowed = (uint32_t)bf_allowed_count(flt.bitmap, flt.bits, ix.n);
        if (allowed == 0) {
            *out_count = 0;
            return SCANN_HIP_OK;
        }
        const bool compact =
            flt.mechanism == 1 || (flt.mechanism == 0 && (double)allowed <= flt.compact_max_fraction * (double)n);
        SCANN_TRY(upload_filter(ix, w, flt, compact, allowed, &fd, st));
    }
    SCANN_TRY(upload(dthr, &T, 8));
    SCANN_TRY(dcnt.ensure(4));
    SCANN_TRY(dcand.ensure((size_t)allowed * 8));
    SCANN_HIP_CHECK(hipMemsetAsync(dcnt.p, 0, 4, st));
    BfPass b{};
    b.queries = dq.as<float>();
    b.nq = 1;
    b.q_stride = q_stride;
    b.nrows = fd.ids ? allowed : n;
    b.row_mult = 1;
    b.filter = 1;
    b.thr = dthr.as<uint64_t>();
    b.cand_cnt = dcnt.as<uint32_t>();
    b.cand = dcand.as<uint64_t>();
    b.cap = allowed;
    b.ids = fd.ids;
    b.allow = fd.allow;
    b.allow_bits = fd.allow_bits;
    SCANN_TRY(launch_pass(ix, b, st));
    uint32_t cnt = 0;
    SCANN_HIP_CHECK(hipMemcpyAsync(&cnt, dcnt.p, 4, hipMemcpyDeviceToHost, st));
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    *out_count = cnt;
    if (cnt == 0) return SCANN_HIP_OK;
    SCANN_TRY(dsorted.ensure((size_t)cnt * 8));
    size_t tmp_bytes = 0;
    SCANN_HIP_CHECK(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, dcand.as<uint64_t>(),
                                                      dsorted.as<uint64_t>(), (int)cnt, 0, 64, st));
    SCANN_TRY(dtmp.ensure(tmp_bytes));
    SCANN_HIP_CHECK(hipcub::DeviceRadixSort::SortKeys(dtmp.p, tmp_bytes, dcand.as<uint64_t>(),
                                                      dsorted.as<uint64_t>(), (int)cnt, 0, 64, st));
    const uint32_t nout = (uint32_t)std::min<uint64_t>(cnt, capacity);
    if (nout == 0) return SCANN_HIP_OK;
    SCANN_TRY(didx.ensure((size_t)nout * 4));
    SCANN_TRY(ddist.ensure((size_t)nout * 4));
    SCANN_TRY(launch(bf_decode_keys_kernel, dim3(ceil_div_u32(nout, 256)), dim3(256), 0, st,
                     dsorted.as<uint64_t>(), nout, didx.as<uint32_t>(), ddist.as<float>()));
    SCANN_HIP_CHECK(hipMemcpyAsync(out_idx, didx.p, (size_t)nout * 4, hipMemcpyDeviceToHost, st));
    SCANN_HIP_CHECK(hipMemcpyAsync(out_dist, ddist.p, (size_t)nout * 4, hipMemcpyDeviceToHost, st));
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    return SCANN_HIP_OK;
}

// centres, assignments and (optional) distances on the device; enqueue only.  Reads ix.rows, n, dim and stride.
int bf_assign_nearest_device(const BfIndexDev &ix, const float *d_centers, uint32_t k, uint32_t *d_out_idx,
                             float *d_out_dist, hipStream_t st) {
    if (ix.n == 0) return SCANN_HIP_OK;
    return launch_assign_nearest(ix.dim, dim3((uint32_t)ceil_div_u64(ix.n, 256)), st, ix, d_centers, k, d_out_idx,
                                 d_out_dist);
}

int bf_assign_nearest_host(const BfIndexDev &ix, const float *centers, uint32_t k, uint32_t *out_idx,
                           float *out_dist, hipStream_t st) {
    if (ix.n == 0) return SCANN_HIP_OK;
    DevBuf dc, di, dd;
    SCANN_TRY(upload(dc, centers, (size_t)k * ix.dim * 4));
    SCANN_TRY(di.ensure((size_t)ix.n * 4));
    if (out_dist) SCANN_TRY(dd.ensure((size_t)ix.n * 4));
    SCANN_TRY(bf_assign_nearest_device(ix, dc.as<float>(), k, di.as<uint32_t>(), out_dist ? dd.as<float>() : nullptr, st));
    SCANN_HIP_CHECK(hipMemcpyAsync(out_idx, di.p, (size_t)ix.n * 4, hipMemcpyDeviceToHost, st));
    if (out_dist) SCANN_HIP_CHECK(hipMemcpyAsync(out_dist, dd.p, (size_t)ix.n * 4, hipMemcpyDeviceToHost, st));
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    return SCANN_HIP_OK;
}

// =====================================================================================
// K-means on the GPU (index build).  KMeans::fit_single
// (trees/kmeans.rs:210-263) over the rows of a brute-force index, optionally a column window
// [col_offset, col_offset + sub_dim) of them (per-subspace codebook training,
// hashes/codebook.rs:177-199):
//   assign_clusters :352-379   nearest centre, strict '<' (lowest index on ties); sequential
//                              scalar SquaredL2 below simd_threshold dims, squared_l2_avx2's order
//                              from there on (:419-431): assign_nearest_kernel / _avx_kernel
//   inertia :376               f64 sum of the minimum distances in datapoint order: a reduction
//                              tree when provably exact (then every order agrees), else the chain
//   update_centers :382-414    f64 sums in ascending datapoint order per (cluster, dim), mean
//                              cast to f32; empty cluster c takes row c % n
// =====================================================================================
// blockIdx.y = the list (one per subspace in the batched codebook training, build.hip; the primitives launch one):
// list y reads v + y * n, writes partials + y * gridDim.x and min_pos_bits + y * min_pos_stride, and is skipped when
// skip[y * skip_stride] is set.
__global__ __launch_bounds__(256) void km_sum_f64_kernel(const float *__restrict__ v, uint64_t n,
                                                         double *__restrict__ partials,
                                                         uint32_t *__restrict__ min_pos_bits, uint32_t min_pos_stride,
                                                         const uint32_t *__restrict__ skip, uint32_t skip_stride) {
    __shared__ double s[256];
    if (skip && skip[blockIdx.y * skip_stride]) return;   // (block-uniform)
    v += (uint64_t)blockIdx.y * n;
    partials += (size_t)blockIdx.y * gridDim.x;
    if (min_pos_bits) min_pos_bits += (size_t)blockIdx.y * min_pos_stride;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const float x = i < n ? v[i] : 0.0f;
    s[threadIdx.x] = (double)x;
    // smallest positive term (bit pattern order == value order for positive floats)
    if (min_pos_bits) {   // kernel-uniform
        uint32_t b = x > 0.0f ? __float_as_uint(x) : 0xFFFFFFFFu;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) b = min(b, (uint32_t)__shfl_xor((int)b, o));
        if ((threadIdx.x & 63u) == 0 && b != 0xFFFFFFFFu) atomicMin(min_pos_bits, b);
    }
    __syncthreads();
    for (uint32_t o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = s[0];
}

// inertia as the reference computes it (kmeans.rs:376): f64 += (f64)min_dist in datapoint order, one
// dependent chain.  Only used when the tree sum above is not provably exact.  One block: waves 1-3
// stage the next 4096 values in LDS while lane 0 adds the current ones.
// blockIdx.x = the list: reads v + x * n, writes total_out[x * out_stride]; runs only where need[x * need_stride] is set
// (need null: always).
__global__ __launch_bounds__(256) void km_sum_f64_sequential_kernel(const float *__restrict__ v, uint64_t n,
                                                                    double *__restrict__ total_out, uint32_t out_stride,
                                                                    const uint32_t *__restrict__ need,
                                                                    uint32_t need_stride) {
    constexpr uint32_t T = 4096;
    __shared__ float s_x[2][T];
    const uint32_t tid = threadIdx.x;
    if (need && !need[blockIdx.x * need_stride]) return;   // (block-uniform)
    v += (uint64_t)blockIdx.x * n;
    total_out += (size_t)blockIdx.x * out_stride;
    auto stage = [&](uint64_t i0, uint32_t buf, uint32_t t0, uint32_t nt) {
        const uint32_t cnt = (uint32_t)min((uint64_t)T, n - i0);
        for (uint32_t f = t0; f < cnt; f += nt) s_x[buf][f] = v[i0 + f];
    };
    if (n) stage(0, 0, tid, 256);
    __syncthreads();
    double sum = 0.0;
    uint32_t buf = 0;
    for (uint64_t i0 = 0; i0 < n; i0 += T, buf ^= 1u) {
        const uint32_t cnt = (uint32_t)min((uint64_t)T, n - i0);
        if (tid >= 64) {
            if (i0 + T < n) stage(i0 + T, buf ^ 1u, tid - 64, 192);
        } else if (tid == 0) {
            for (uint32_t f = 0; f < cnt; ++f) sum += (double)s_x[buf][f];
        }
        __syncthreads();
    }
    if (tid == 0) *total_out = sum;
}

// partials -> total (fixed order: per-thread chunks, then the 256 chunk sums in order); optional
// k-means++ pick: first i with cumulative min_d >= u * total (kmeans.rs:318-331), or `fallback`
// if total == 0.  One block of 256 threads per list (blockIdx.x; the primitives launch one): list x reads
// partials + x * nb and min_d + x * n, draws (u_tab[x], fallback_tab[x]) when the tables are given, and writes
// total_out[x * total_stride] and pick_out[x * pick_stride].
__global__ __launch_bounds__(256) void km_total_pick_kernel(const double *__restrict__ partials, uint32_t nb,
                                                            const float *__restrict__ min_d, uint64_t n,
                                                            double u, uint32_t fallback,
                                                            const double *__restrict__ u_tab,
                                                            const uint32_t *__restrict__ fallback_tab,
                                                            double *__restrict__ total_out, uint32_t total_stride,
                                                            uint32_t *__restrict__ pick_out, uint32_t pick_stride) {
    __shared__ double s_chunk[256];
    __shared__ float s_vals[256];
    __shared__ uint32_t s_blk;
    __shared__ double s_cum;
    const uint32_t t = threadIdx.x;
    partials += (size_t)blockIdx.x * nb;
    if (min_d) min_d += (uint64_t)blockIdx.x * n;
    total_out += (size_t)blockIdx.x * total_stride;
    if (pick_out) pick_out += (size_t)blockIdx.x * pick_stride;
    if (u_tab) {
        u = u_tab[blockIdx.x];
        fallback = fallback_tab[blockIdx.x];
    }
    const uint32_t per = (nb + 255u) / 256u;
    const uint32_t b0 = min(nb, t * per), b1 = min(nb, b0 + per);
    double mine = 0.0;
    for (uint32_t b = b0; b < b1; ++b) mine += partials[b];
    s_chunk[t] = mine;
    __syncthreads();
    if (t == 0) {
        double total = 0.0;
        for (uint32_t c = 0; c < 256; ++c) total += s_chunk[c];
        *total_out = total;
        s_blk = 0xFFFFFFFFu;
        if (pick_out) {
            if (!(total > 0.0)) {
                *pick_out = fallback;
            } else {
                const double thr = u * total;
                double cum = 0.0;
                uint32_t c = 0;
                for (; c + 1 < 256; ++c) {   // chunk holding the threshold
                    if (cum + s_chunk[c] >= thr) break;
                    cum += s_chunk[c];
                }
                uint32_t b = min(nb, c * per);
                const uint32_t be = min(nb, b + per);
                for (; b + 1 < be; ++b) {    // block of 256 rows inside the chunk
                    if (cum + partials[b] >= thr) break;
                    cum += partials[b];
                }
                s_blk = min(b, nb - 1);
                s_cum = cum;
            }
        }
    }
    __syncthreads();
    if (s_blk == 0xFFFFFFFFu) return;
    const uint64_t i0 = (uint64_t)s_blk * 256;
    s_vals[t] = (i0 + t < n) ? min_d[i0 + t] : 0.0f;
    __syncthreads();
    if (t == 0) {
        const double thr = u * (*total_out);
        const uint32_t cnt = (uint32_t)min((uint64_t)256, n - i0);
        double cum = s_cum;
        uint32_t sel = cnt - 1;
        for (uint32_t i = 0; i < cnt; ++i) {
            cum += (double)s_vals[i];
            if (cum >= thr) {
                sel = i;
                break;
            }
        }
        *pick_out = (uint32_t)(i0 + sel);
    }
}

// min_d[i] = min(min_d[i], ||row_i - row_sel||^2)  (kmeans.rs:303-345); first = overwrite.
// avx: squared_l2_avx2's order (dim >= simd_threshold), else the sequential scalar sum.
__global__ __launch_bounds__(256) void km_mind_update_kernel(BfIndexDev ix, const uint32_t *__restrict__ sel,
                                                             int first, int avx, float *__restrict__ min_d) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ix.n) return;
    const float *row = ix.rows + i * ix.stride, *c = ix.rows + (uint64_t)(*sel) * ix.stride;
    float d = 0.0f;
    uint32_t j = 0;
    if (avx) {
        float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (; j + 8 <= ix.dim; j += 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float t = row[j + u] - c[j + u];
                acc[u] = fmaf(t, t, acc[u]);
            }
        }
        d = ((acc[0] + acc[4]) + (acc[1] + acc[5])) + ((acc[2] + acc[6]) + (acc[3] + acc[7]));
    } else if (((ix.stride & 3u) == 0) && ((reinterpret_cast<uintptr_t>(ix.rows) & 15u) == 0)) {
        for (; j + 4 <= ix.dim; j += 4) {   // 16-byte loads, same sequential sum
            const float4 x = *reinterpret_cast<const float4 *>(row + j);
            const float4 y = *reinterpret_cast<const float4 *>(c + j);
            float t = x.x - y.x; d = d + t * t;
            t = x.y - y.y; d = d + t * t;
            t = x.z - y.z; d = d + t * t;
            t = x.w - y.w; d = d + t * t;
        }
    }
    for (; j < ix.dim; ++j) {
        const float t = row[j] - c[j];
        d = d + t * t;
    }
    min_d[i] = (first || d < min_d[i]) ? d : min_d[i];
}

__global__ void km_gather_rows_kernel(BfIndexDev ix, const uint32_t *__restrict__ picks, uint32_t k,
                                      float *__restrict__ centers) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= k * ix.dim) return;
    const uint32_t c = e / ix.dim, j = e - c * ix.dim;
    centers[e] = ix.rows[(uint64_t)picks[c] * ix.stride + j];
}

__global__ void km_make_keys_kernel(const uint32_t *__restrict__ assign, uint64_t n,
                                    uint64_t *__restrict__ keys) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = ((uint64_t)assign[i] << 32) | (uint32_t)i;
}

// offsets[c] = first position of cluster c in the sorted keys (lower bound), offsets[k] = n
__global__ void km_offsets_kernel(const uint64_t *__restrict__ sorted, uint64_t n, uint32_t k,
                                  uint32_t *__restrict__ offsets) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > k) return;
    const uint64_t target = (uint64_t)c << 32;
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (sorted[mid] < target) lo = mid + 1; else hi = mid;
    }
    offsets[c] = (uint32_t)lo;
}

// sorted member order -> contiguous copy of the (windowed) rows, so that the update streams
__global__ void km_gather_sorted_kernel(BfIndexDev ix, const uint64_t *__restrict__ sorted, uint64_t n,
                                        float *__restrict__ out) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * ix.dim) return;
    const uint64_t m = e / ix.dim;
    const uint32_t j = (uint32_t)(e - m * ix.dim);
    out[e] = ix.rows[(uint64_t)(uint32_t)sorted[m] * ix.stride + j];
}

// One block per cluster.  The f64 sum of every (cluster, dimension) runs over the cluster's
// members in ascending datapoint order (keys are sorted by (cluster, index)) -- a sequential
// chain by definition; the member rows were gathered into member order by the whole chip
// (km_gather_sorted_kernel) and the block stages tiles of them in LDS with all 256 threads, so
// the chain reads LDS instead of waiting for one random HBM access per add.
constexpr uint32_t kKmTileFloats = 8192;   // 32 KB of staged row values
__global__ __launch_bounds__(256) void km_update_kernel(BfIndexDev ix, const float *__restrict__ grows,
                                                        const uint32_t *__restrict__ offsets,
                                                        float *__restrict__ centers, uint32_t k_stride,
                                                        const uint32_t *__restrict__ skip, uint32_t skip_stride) {
    // blockIdx.y = the column window (one per subspace in the batched codebook training; the primitives launch one):
    // window y reads the columns from y * dim on, offsets + y * k_stride (positions into `grows` as a whole) and writes
    // centers + y * k_stride * dim; it is skipped when skip[y * skip_stride] is set.
    __shared__ float s_x[kKmTileFloats];
    if (skip && skip[blockIdx.y * skip_stride]) return;   // (block-uniform)
    ix.rows += (size_t)blockIdx.y * ix.dim;
    offsets += (size_t)blockIdx.y * k_stride;
    centers += (size_t)blockIdx.y * k_stride * ix.dim;
    const uint32_t c = blockIdx.x, tid = threadIdx.x, dim = ix.dim;
    const uint32_t b = offsets[c], e = offsets[c + 1];
    if (e == b) {   // empty cluster: data[c % n]  (kmeans.rs:405-408)
        for (uint32_t j = tid; j < dim; j += blockDim.x)
            centers[(size_t)c * dim + j] = ix.rows[(uint64_t)(c % ix.n) * ix.stride + j];
        return;
    }
    if (dim <= 64) {
        // Narrow rows (the per-subspace codebooks: 4..16 dims, 16..256 clusters): wave 0 runs the
        // chains while waves 1-3 stage the NEXT tile, so the chain never waits for a staging phase
        // (with one buffer the 4 summing threads idled through every copy: 2.1 ms per call at 62 k
        // members).
        const uint32_t half = kKmTileFloats / 2, tm = half / dim;   // members per half-tile
        auto stage = [&](uint32_t m0, uint32_t buf, uint32_t t0, uint32_t nt) {
            const uint32_t nm = min(tm, e - m0);
            for (uint32_t f = t0; f < nm * dim; f += nt) s_x[buf * half + f] = grows[(uint64_t)m0 * dim + f];
        };
        stage(b, 0, tid, blockDim.x);
        __syncthreads();
        double sum = 0.0;
        uint32_t buf = 0;
        for (uint32_t m0 = b; m0 < e; m0 += tm, buf ^= 1u) {
            const uint32_t nm = min(tm, e - m0);
            if (tid >= 64) {
                if (m0 + tm < e) stage(m0 + tm, buf ^ 1u, tid - 64, blockDim.x - 64);
            } else if (tid < dim) {
                const float *sx = s_x + buf * half;
                for (uint32_t mm = 0; mm < nm; ++mm) sum += (double)sx[mm * dim + tid];
            }
            __syncthreads();
        }
        if (tid < dim) centers[(size_t)c * dim + tid] = (float)(sum / (double)(e - b));
        return;
    }
    // dimensions are processed in slabs of <= 256 (one chain per thread)
    for (uint32_t j0 = 0; j0 < dim; j0 += 256) {
        const uint32_t dw = min(256u, dim - j0);          // slab width
        const uint32_t tm = kKmTileFloats / dw;           // members per tile
        double sum = 0.0;
        for (uint32_t m0 = b; m0 < e; m0 += tm) {
            const uint32_t nm = min(tm, e - m0);
            __syncthreads();
            for (uint32_t f = tid; f < nm * dw; f += blockDim.x) {
                const uint32_t mm = f / dw, jj = f - mm * dw;
                s_x[f] = grows[(uint64_t)(m0 + mm) * dim + j0 + jj];   // rows gathered in member order
            }
            __syncthreads();
            if (tid < dw)
                for (uint32_t mm = 0; mm < nm; ++mm) sum += (double)s_x[mm * dw + tid];
        }
        if (tid < dw) centers[(size_t)c * dim + j0 + tid] = (float)(sum / (double)(e - b));
    }
}

static inline uint64_t km_splitmix(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static BfIndexDev km_view(const BfIndexDev &ix, uint32_t col_offset, uint32_t sub_dim) {
    BfIndexDev v = ix;
    v.rows = ix.rows + col_offset;
    v.dim = sub_dim;
    return v;
}

static int km_launch_assign(const BfIndexDev &v, const float *d_centers, uint32_t k, uint32_t *d_assign,
                            float *d_dist, bool avx, hipStream_t st) {
    const uint32_t dimp = (v.dim + 3u) & ~3u;
    const dim3 grid((uint32_t)ceil_div_u64(v.n, 256));
    if (avx) {
        const size_t lds = (size_t)kAvxTC * dimp * sizeof(float);
        SCANN_TRY(launch(assign_nearest_avx_kernel, grid, dim3(256), lds, st, v, d_centers, k, d_assign, d_dist));
    } else {
        SCANN_TRY(launch_assign_nearest(v.dim, grid, st, v, d_centers, k, d_assign, d_dist));
    }
    return SCANN_HIP_OK;
}

uint64_t km_seed_stream_next(uint64_t &s) { return km_splitmix(s); }

// ---- batched launches of the kernels above (build.hip: every subspace of a codebook in one launch) ----
int km_sums_batched(const float *d_vals, uint64_t n, uint32_t lists, double *d_partials, uint32_t *d_min_pos,
                    uint32_t min_pos_stride, const uint32_t *d_skip, uint32_t skip_stride, hipStream_t st) {
    const uint32_t nb = (uint32_t)ceil_div_u64(n, 256);
    return launch(km_sum_f64_kernel, dim3(nb, lists), dim3(256), 0, st, d_vals, n, d_partials, d_min_pos, min_pos_stride,
                  d_skip, skip_stride);
}

int km_totals_batched(const double *d_partials, uint64_t n, uint32_t lists, const float *d_min_d, const double *d_u_tab,
                      const uint32_t *d_fallback_tab, double *d_totals, uint32_t total_stride, uint32_t *d_picks,
                      uint32_t pick_stride, hipStream_t st) {
    const uint32_t nb = (uint32_t)ceil_div_u64(n, 256);
    return launch(km_total_pick_kernel, dim3(lists), dim3(256), 0, st, d_partials, nb, d_min_d, n, 0.0, 0u, d_u_tab,
                  d_fallback_tab, d_totals, total_stride, d_picks, pick_stride);
}

int km_sequential_sums_batched(const float *d_vals, uint64_t n, uint32_t lists, double *d_totals, uint32_t total_stride,
                               const uint32_t *d_need, uint32_t need_stride, hipStream_t st) {
    return launch(km_sum_f64_sequential_kernel, dim3(lists), dim3(256), 0, st, d_vals, n, d_totals, total_stride, d_need,
                  need_stride);
}

int km_update_batched(const BfIndexDev &window0, const float *d_grows, const uint32_t *d_offsets, float *d_centers,
                      uint32_t k, uint32_t k_stride, uint32_t windows, const uint32_t *d_skip, uint32_t skip_stride,
                      hipStream_t st) {
    return launch(km_update_kernel, dim3(k, windows), dim3(256), 0, st, window0, d_grows, d_offsets, d_centers, k_stride,
                  d_skip, skip_stride);
}

// The test of bf_kmeans_lloyd_device's inertia (below), for one list: every term is a non-negative multiple of
// g = ulp(smallest positive term); if total <= 2^53 * g every partial sum of every order is exactly representable, so
// the tree sum IS the sum in datapoint order.
bool km_tree_sum_is_exact(double total, uint32_t min_pos_bits) {
    if (min_pos_bits == 0xFFFFFFFFu) return true;   // all terms are zero
    if (!(total == total && total < INFINITY)) return false;
    float mp;
    std::memcpy(&mp, &min_pos_bits, 4);
    int e = 0;
    (void)std::frexp(mp, &e);                    // mp = f * 2^e, f in [0.5, 1)
    const int ge = std::max(e - 24, -149);       // ulp exponent (denormals: 2^-149)
    return total <= std::ldexp(1.0, ge + 53);
}

// The seeding with everything on the device: d_centers_out [k][sub_dim], complete on return.
int bf_kmeans_init_pp_device(const BfIndexDev &ix, uint32_t col_offset, uint32_t sub_dim, uint32_t k, uint64_t seed,
                             uint32_t simd_threshold, float *d_centers_out, KmScratch &sc, hipStream_t st) {
    const int avx = sub_dim >= simd_threshold ? 1 : 0;   // kmeans.rs:419-431
    const BfIndexDev v = km_view(ix, col_offset, sub_dim);
    const uint64_t n = v.n;
    if (n == 0 || k == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "empty dataset / no clusters");
    const uint32_t nb = (uint32_t)ceil_div_u64(n, 256);
    SCANN_TRY(sc.dmin.ensure(n * 4));
    SCANN_TRY(sc.dpart.ensure((size_t)nb * 8));
    SCANN_TRY(sc.dtotal.ensure(16));
    SCANN_TRY(sc.dpicks.ensure((size_t)k * 4));
    uint64_t s = seed;
    const uint32_t first = (uint32_t)(km_splitmix(s) % n);   // kmeans.rs:305-306
    SCANN_HIP_CHECK(hipMemcpyAsync(sc.dpicks.p, &first, 4, hipMemcpyHostToDevice, st));
    for (uint32_t c = 1; c <= k; ++c) {
        uint32_t *sel = sc.dpicks.as<uint32_t>() + (c - 1);
        SCANN_TRY(launch(km_mind_update_kernel, dim3(nb), dim3(256), 0, st, v, sel, c == 1 ? 1 : 0, avx,
                         sc.dmin.as<float>()));
        if (c == k) break;
        SCANN_TRY(launch(km_sum_f64_kernel, dim3(nb), dim3(256), 0, st, sc.dmin.as<float>(), n,
                         sc.dpart.as<double>(), (uint32_t *)nullptr, 0u, (const uint32_t *)nullptr, 0u));
        const double u = (double)(km_splitmix(s) >> 11) * (1.0 / 9007199254740992.0);
        const uint32_t fallback = (uint32_t)(km_splitmix(s) % n);
        SCANN_TRY(launch(km_total_pick_kernel, dim3(1), dim3(256), 0, st, sc.dpart.as<double>(), nb,
                         sc.dmin.as<float>(), n, u, fallback, (const double *)nullptr, (const uint32_t *)nullptr,
                         sc.dtotal.as<double>(), 0u, sc.dpicks.as<uint32_t>() + c, 0u));
    }
    SCANN_TRY(launch(km_gather_rows_kernel, dim3(ceil_div_u32(k * sub_dim, 256)), dim3(256), 0, st, v,
                     sc.dpicks.as<uint32_t>(), k, d_centers_out));
    SCANN_HIP_CHECK(hipStreamSynchronize(st));   // (the first pick was uploaded from this frame)
    return SCANN_HIP_OK;
}

int bf_kmeans_init_pp_host(const BfIndexDev &ix, uint32_t col_offset, uint32_t sub_dim, uint32_t k,
                           uint64_t seed, uint32_t simd_threshold, float *centers_out, hipStream_t st) {
    if (ix.n == 0 || k == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "empty dataset / no clusters");
    KmScratch sc;
    DevBuf dcent;
    SCANN_TRY(dcent.ensure((size_t)k * sub_dim * 4));
    SCANN_TRY(bf_kmeans_init_pp_device(ix, col_offset, sub_dim, k, seed, simd_threshold, dcent.as<float>(), sc, st));
    SCANN_HIP_CHECK(hipMemcpyAsync(centers_out, dcent.p, (size_t)k * sub_dim * 4, hipMemcpyDeviceToHost, st));
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    return SCANN_HIP_OK;
}

// keys (cluster << 32 | index) of an assignment, radix-sorted into sc.dsorted: every cluster's members in ascending
// datapoint index; sc.doff [k + 1] = where each cluster starts.  Enqueue only.
int bf_kmeans_csr_device(const uint32_t *d_assign, uint64_t n, uint32_t k, KmScratch &sc, hipStream_t st) {
    const uint32_t nb = (uint32_t)ceil_div_u64(n, 256);
    SCANN_TRY(sc.dkeys.ensure(n * 8));
    SCANN_TRY(sc.dsorted.ensure(n * 8));
    SCANN_TRY(sc.doff.ensure((size_t)(k + 1) * 4));
    size_t tmp_bytes = 0;
    SCANN_HIP_CHECK(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, sc.dkeys.as<uint64_t>(),
                                                      sc.dsorted.as<uint64_t>(), (int)n, 0, 64, st));
    SCANN_TRY(sc.dtmp.ensure(tmp_bytes));
    tmp_bytes = sc.dtmp.bytes;
    int key_bits = 33;   // 32 index bits + the bits of the cluster id
    while (key_bits < 64 && (1ull << (key_bits - 32)) < k) ++key_bits;
    SCANN_TRY(launch(km_make_keys_kernel, dim3(nb), dim3(256), 0, st, d_assign, n, sc.dkeys.as<uint64_t>()));
    SCANN_HIP_CHECK(hipcub::DeviceRadixSort::SortKeys(sc.dtmp.p, tmp_bytes, sc.dkeys.as<uint64_t>(),
                                                      sc.dsorted.as<uint64_t>(), (int)n, 0, key_bits, st));
    SCANN_TRY(launch(km_offsets_kernel, dim3(ceil_div_u32(k + 1, 256)), dim3(256), 0, st, sc.dsorted.as<uint64_t>(), n, k,
                     sc.doff.as<uint32_t>()));
    return SCANN_HIP_OK;
}

// The Lloyd loop with centres [k][sub_dim] and the assignment [n] on the device, both updated in place.
// final_assign: the assignment (and inertia) of the final centres (kmeans.rs:248-255); without it d_assign holds the
// assignment the last update was made from, which is all a codebook needs (only the centres are kept).
int bf_kmeans_lloyd_device(const BfIndexDev &ix, uint32_t col_offset, uint32_t sub_dim, float *d_centers, uint32_t k,
                           uint32_t max_iterations, double convergence_threshold, uint32_t simd_threshold,
                           uint32_t *d_assign, bool final_assign, KmScratch &sc, double *out_inertia,
                           uint32_t *out_iterations, int *out_converged, hipStream_t st) {
    const BfIndexDev v = km_view(ix, col_offset, sub_dim);
    const bool avx = sub_dim >= simd_threshold;   // kmeans.rs:419-431
    const uint64_t n = v.n;
    if (n == 0 || k == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "Cannot cluster empty dataset");
    const uint32_t nb = (uint32_t)ceil_div_u64(n, 256);
    SCANN_TRY(sc.ddist.ensure(n * 4));
    SCANN_TRY(sc.dpart.ensure((size_t)nb * 8));
    SCANN_TRY(sc.dtotal.ensure(16));
    SCANN_TRY(sc.dgrows.ensure(n * sub_dim * 4));

    // dtotal: [0] f64 total, [1] (as u32) bit pattern of the smallest positive term
    auto assign_and_inertia = [&](double *inertia) -> int {
        SCANN_TRY(km_launch_assign(v, d_centers, k, d_assign, sc.ddist.as<float>(), avx, st));
        uint32_t *d_minpos = reinterpret_cast<uint32_t *>(sc.dtotal.as<double>() + 1);
        SCANN_HIP_CHECK(hipMemsetAsync(d_minpos, 0xFF, 4, st));
        SCANN_TRY(launch(km_sum_f64_kernel, dim3(nb), dim3(256), 0, st, sc.ddist.as<float>(), n,
                         sc.dpart.as<double>(), d_minpos, 0u, (const uint32_t *)nullptr, 0u));
        SCANN_TRY(launch(km_total_pick_kernel, dim3(1), dim3(256), 0, st, sc.dpart.as<double>(), nb,
                         (const float *)nullptr, n, 0.0, 0u, (const double *)nullptr, (const uint32_t *)nullptr,
                         sc.dtotal.as<double>(), 0u, (uint32_t *)nullptr, 0u));
        struct { double total; uint32_t minpos; uint32_t pad; } h;
        SCANN_HIP_CHECK(hipMemcpyAsync(&h, sc.dtotal.p, 16, hipMemcpyDeviceToHost, st));
        SCANN_HIP_CHECK(hipStreamSynchronize(st));
        // The reference adds the terms in datapoint order (kmeans.rs:376); the tree sum stands when it is that sum.
        if (!km_tree_sum_is_exact(h.total, h.minpos)) {
            SCANN_TRY(launch(km_sum_f64_sequential_kernel, dim3(1), dim3(256), 0, st, sc.ddist.as<float>(), n,
                             sc.dtotal.as<double>(), 0u, (const uint32_t *)nullptr, 0u));
            SCANN_HIP_CHECK(hipMemcpyAsync(&h.total, sc.dtotal.p, 8, hipMemcpyDeviceToHost, st));
            SCANN_HIP_CHECK(hipStreamSynchronize(st));
        }
        *inertia = h.total;
        return SCANN_HIP_OK;
    };

    double prev = INFINITY, inertia = 0.0;
    uint32_t iters = 0;
    int converged = 0;
    for (uint32_t it = 0; it < max_iterations; ++it) {   // kmeans.rs:226-246
        iters = it + 1;
        SCANN_TRY(assign_and_inertia(&inertia));
        const double rel = std::fabs(prev - inertia) / (prev + 1e-10);
        if (rel < convergence_threshold) {
            converged = 1;
            break;
        }
        prev = inertia;
        // update_centers: members of every cluster in ascending datapoint order
        SCANN_TRY(bf_kmeans_csr_device(d_assign, n, k, sc, st));
        SCANN_TRY(launch(km_gather_sorted_kernel, dim3((uint32_t)ceil_div_u64(n * sub_dim, 256)), dim3(256), 0,
                         st, v, sc.dsorted.as<uint64_t>(), n, sc.dgrows.as<float>()));
        SCANN_TRY(launch(km_update_kernel, dim3(k), dim3(256), 0, st, v, sc.dgrows.as<float>(),
                         sc.doff.as<uint32_t>(), d_centers, 0u, (const uint32_t *)nullptr, 0u));
    }
    // final assignment for accurate sizes / inertia (kmeans.rs:248-255)
    if (final_assign) SCANN_TRY(assign_and_inertia(&inertia));
    if (out_inertia) *out_inertia = inertia;
    if (out_iterations) *out_iterations = iters;
    if (out_converged) *out_converged = converged;
    return SCANN_HIP_OK;
}

int bf_kmeans_lloyd_host(const BfIndexDev &ix, uint32_t col_offset, uint32_t sub_dim, float *centers,
                         uint32_t k, uint32_t max_iterations, double convergence_threshold,
                         uint32_t simd_threshold, uint32_t *out_assign, uint32_t *out_sizes, double *out_inertia,
                         uint32_t *out_iterations, int *out_converged, hipStream_t st) {
    const uint64_t n = ix.n;
    if (n == 0 || k == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "Cannot cluster empty dataset");
    KmScratch sc;
    DevBuf dcent, dassign;
    SCANN_TRY(upload(dcent, centers, (size_t)k * sub_dim * 4));
    SCANN_TRY(dassign.ensure(n * 4));
    SCANN_TRY(bf_kmeans_lloyd_device(ix, col_offset, sub_dim, dcent.as<float>(), k, max_iterations, convergence_threshold,
                                     simd_threshold, dassign.as<uint32_t>(), true, sc, out_inertia, out_iterations,
                                     out_converged, st));
    SCANN_HIP_CHECK(hipMemcpyAsync(centers, dcent.p, (size_t)k * sub_dim * 4, hipMemcpyDeviceToHost, st));
    if (out_assign || out_sizes) {
        std::vector<uint32_t> tmp;
        uint32_t *dst = out_assign;
        if (!dst) {
            tmp.resize(n);
            dst = tmp.data();
        }
        SCANN_HIP_CHECK(hipMemcpyAsync(dst, dassign.p, n * 4, hipMemcpyDeviceToHost, st));
        SCANN_HIP_CHECK(hipStreamSynchronize(st));
        if (out_sizes) {
            for (uint32_t c = 0; c < k; ++c) out_sizes[c] = 0;
            for (uint64_t i = 0; i < n; ++i) ++out_sizes[dst[i]];
        }
    }
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    return SCANN_HIP_OK;
}

}  // namespace scann

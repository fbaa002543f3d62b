// bf_bin.hip -- brute force over bit rows (SCANN_HIP_ROWS_BIN1) by Hamming distance, DESIGN.md 3.3b-ii.
//
// DistanceMeasure::Hamming (distance_measures/mod.rs:49-50, one_to_one.rs:618-632) counts the positions whose values
// differ.  On rows stored one bit per element that is popcount(x XOR q): the batch's f32 queries are packed once
// (bit j = q[j] != 0), every pass then XORs and counts 32 elements per instruction pair, or, for batches of 64 queries
// and more, multiplies +-1 bytes on the integer matrix cores.  The counts are integers
// below 2^24, so the f32 distance is exact and every kernel path returns the same bits.  What follows the scores
// (threshold, candidate lists, selection, radius sort) is bf.hip's.
#include "bf.h"

#include "launch.h"

namespace scann {

size_t bf_bin_query_bytes(const BfIndexDev &ix, uint32_t nq) { return (size_t)nq * (ix.stride / 32u) * sizeof(uint32_t); }

// One wave per query, 64 elements per step: a lane tests q[64 c + lane], the ballot is words 2 c and 2 c + 1.  Lanes at
// or past dim vote 0, so the pad bits dim .. stride - 1 of the packed query are clear.  NaN != 0 is true: a NaN is a 1.
__global__ __launch_bounds__(256) void bf_pack_query_bits_kernel(const float *__restrict__ queries, uint32_t nq,
                                                                 uint32_t dim, uint32_t q_stride, uint32_t words,
                                                                 uint32_t *__restrict__ qbits) {
    const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (q >= nq) return;   // wave-uniform
    const float *src = queries + (size_t)q * q_stride;
    uint32_t *dst = qbits + (size_t)q * words;
    for (uint32_t c = 0; 2u * c < words; ++c) {
        const uint32_t e = 64u * c + lane;
        const float v = e < dim ? src[e] : 0.0f;
        const uint64_t b = __ballot(v != 0.0f);
        if (lane == 0) dst[2u * c] = (uint32_t)b;
        if (lane == 1 && 2u * c + 1u < words) dst[2u * c + 1u] = (uint32_t)(b >> 32);
    }
}


// One row per lane, QT queries per block row.  The row travels in chunks of CH words through VGPRs (CH = 32, or 8 for
// rows of up to 256 bits, which would otherwise count 24 words of zeros; VEC: CH / 4 16-byte loads in flight, else
// 4-byte loads); the same chunk of the QT packed queries sits in LDS as [word][QT], so
// the words of four queries for one row word are one wave-uniform 16-byte broadcast read.  Per (row word, query):
// v_xor_b32, then v_bcnt_u32_b32 with the query's accumulator as its addend.  The QT accumulators stay in registers
// across the chunks of a wide row.  Only words below ceil(dim / 32) are read from LDS or counted, and the chunk that
// holds the last of them is masked once (row pad bits may be set; the packed queries' are clear).
// Lanes past the last row compute on the last row and emit nothing: every lane reaches every barrier.
// The filter pass's bounds wait in LDS, one read per block instead of QT global loads in every lane's emit.
template <int QT, bool VEC, int CH>
__global__ __launch_bounds__(256) void bf_hamming_kernel(BfIndexDev ix, BfPass p) {
    static_assert(QT == 2 || QT % 4 == 0, "queries are read from LDS two or four at a time");
    __shared__ __attribute__((aligned(16))) uint32_t qs[CH * QT];   // [word of the chunk][QT]
    __shared__ uint64_t s_thr[QT];   // the queries' bounds: read once, not one dependent global load per query at the emit
    if (p.filter && threadIdx.x < (uint32_t)QT && blockIdx.y * QT + threadIdx.x < p.nq)
        s_thr[threadIdx.x] = p.thr[blockIdx.y * QT + threadIdx.x];   // (visible after the first chunk's barrier)
    const uint32_t words = ix.stride >> 5, nw = (ix.dim + 31u) >> 5;       // stored / scored words of a row
    const uint32_t full = ix.dim >> 5, tail = (1u << (ix.dim & 31u)) - 1u;  // whole words; mask of the partial one
    const uint32_t q0 = blockIdx.y * QT;
    const uint32_t vrow = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = vrow < p.nrows;
    const uint32_t *row = static_cast<const uint32_t *>(ix.qrows) +
                          (size_t)bf_real_row(p, valid ? vrow : p.nrows - 1u) * words;
    uint32_t acc[QT];
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) acc[qi] = 0;
    for (uint32_t w0 = 0; w0 < nw; w0 += CH) {
        const bool last = w0 + CH > full;   // the chunk with the partial word or words past the scored ones
        uint32_t r[CH];
        if constexpr (VEC) {   // (words % 4 == 0: a 16-byte load that starts below nw ends inside the row)
#pragma unroll
            for (int i = 0; i < CH / 4; ++i) {
                uint4 v = make_uint4(0, 0, 0, 0);
                if (!last || w0 + 4u * i < nw) v = *reinterpret_cast<const uint4 *>(row + w0 + 4 * i);
                r[4 * i] = v.x, r[4 * i + 1] = v.y, r[4 * i + 2] = v.z, r[4 * i + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < CH; ++i) r[i] = (!last || w0 + i < nw) ? row[w0 + i] : 0u;
        }
        if (last) {
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const uint32_t wi = w0 + i;
                r[i] &= wi < full ? 0xFFFFFFFFu : (wi == full ? tail : 0u);
            }
        }
        if (w0) __syncthreads();   // every lane has left the previous chunk's query words
        for (uint32_t i = threadIdx.x; i < (uint32_t)(CH * QT); i += blockDim.x) {
            const uint32_t wi = i / QT, qi = i % QT;   // consecutive lanes: consecutive LDS words (no bank conflict)
            qs[wi * QT + qi] = (q0 + qi < p.nq && w0 + wi < nw) ? p.qbits[(size_t)(q0 + qi) * words + w0 + wi] : 0u;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            if constexpr (QT == 2) {
                const uint2 qv = *reinterpret_cast<const uint2 *>(qs + i * QT);
                acc[0] += (uint32_t)__popc(r[i] ^ qv.x);
                acc[1] += (uint32_t)__popc(r[i] ^ qv.y);
            } else {
#pragma unroll
                for (int g = 0; g < QT / 4; ++g) {
                    const uint4 qv = *reinterpret_cast<const uint4 *>(qs + i * QT + 4 * g);
                    acc[4 * g] += (uint32_t)__popc(r[i] ^ qv.x);
                    acc[4 * g + 1] += (uint32_t)__popc(r[i] ^ qv.y);
                    acc[4 * g + 2] += (uint32_t)__popc(r[i] ^ qv.z);
                    acc[4 * g + 3] += (uint32_t)__popc(r[i] ^ qv.w);
                }
            }
        }
    }
    if (!valid) return;
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) {
        if (q0 + qi >= p.nq) break;
        uint64_t T = 0;
        float Tf = 0.0f;
        if (p.filter) {
            T = s_thr[qi];
            Tf = bf_thr_float(T);
        }
        bf_emit(p, q0 + qi, vrow, (float)acc[qi], Tf, T);   // < 2^24: exact
    }
}

int bf_bin_pack_queries(const BfIndexDev &ix, const float *d_queries, uint32_t nq, uint32_t q_stride, uint32_t *d_qbits,
                        hipStream_t st) {
    if (nq == 0) return SCANN_HIP_OK;
    return launch(bf_pack_query_bits_kernel, dim3(ceil_div_u32(nq, 4)), dim3(256), 0, st, d_queries, nq, ix.dim, q_stride,
                  ix.stride / 32u, d_qbits);
}

// ---- the batch pass on the integer matrix cores ----------------------------------------------------------------------
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// the low four bits of n -> four 0/1 bytes (bit j lands on bit 8 j: the four shifted copies never overlap)
__device__ __forceinline__ uint32_t bin_nib_01(uint32_t n) { return ((n & 15u) * 0x00204081u) & 0x01010101u; }
// sixteen bits -> sixteen int8 of +1 (bit set) / -1 (clear): 0/1 bytes times 0xFE, complemented
__device__ __forceinline__ v4i bin_half_pm1(uint32_t b) {
    return v4i{(int)~(bin_nib_01(b) * 0xFEu), (int)~(bin_nib_01(b >> 4) * 0xFEu), (int)~(bin_nib_01(b >> 8) * 0xFEu),
               (int)~(bin_nib_01(b >> 12) * 0xFEu)};
}
// sixteen bits -> sixteen byte masks 0xFF / 0x00
__device__ __forceinline__ v4i bin_half_mask(uint32_t b) {
    return v4i{(int)(bin_nib_01(b) * 0xFFu), (int)(bin_nib_01(b >> 4) * 0xFFu), (int)(bin_nib_01(b >> 8) * 0xFFu),
               (int)(bin_nib_01(b >> 12) * 0xFFu)};
}

constexpr uint32_t kBmRows = 128, kBmWords = 8;   // rows of a block's tile; row words (k-steps of 32 bits) per LDS stage

// v_mfma_i32_32x32x32_i8 with both operands as +-1 bytes: sum_j x_j q_j = dim - 2 Hamming over the scored bits, an exact
// i32, so distance = (dim - dot) / 2 and no popcount of the row or the query is needed.  Query bytes at or past dim are
// 0, which also masks the rows' pad bits.  Block = 4 waves x 32 queries over one tile of 128 rows.  A stage is 8 words
// of the 128 rows: each thread loads one 16-byte word of one row, expands it to 128 int8 in registers and writes them
// to LDS (row r, 16-byte chunk c at r * 256 + 16 (c ^ (r & 15)): the 32 rows of a fragment read fall on 16 chunk
// columns); every wave then reads its A fragments from LDS, expands its own query bits in registers (16 bits per lane
// and k-step) and issues 4 MFMAs per k-step, one per 32-row sub-tile.  A[i = lane & 31][k = 16 h + j] = row i, bit
// 32 t + 16 h + j; B[k][n = lane & 31] = query n, the same bit.  The epilogue is bf_emit, as in bf_hamming_kernel.
__global__ __launch_bounds__(256) void bf_hamming_mfma_kernel(BfIndexDev ix, BfPass p) {
    __shared__ __attribute__((aligned(16))) unsigned char xs[kBmRows * kBmWords * 32];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, h = lane >> 5, li = lane & 31u;
    const uint32_t words = ix.stride >> 5, nw = (ix.dim + 31u) >> 5, full = ix.dim >> 5, tail = (1u << (ix.dim & 31u)) - 1u;
    const uint32_t row0 = blockIdx.x * kBmRows;
    const uint32_t q = blockIdx.y * 128u + wave * 32u + li;
    const bool qvalid = q < p.nq;
    const uint32_t *qw = p.qbits + (size_t)min(q, p.nq - 1u) * words;
    const uint32_t srow = tid >> 1, squad = tid & 1u;   // this thread's share of a stage: words 4 squad .. + 3 of row srow
    const uint32_t *src = static_cast<const uint32_t *>(ix.qrows) +
                          (size_t)bf_real_row(p, min(row0 + srow, p.nrows - 1u)) * words + 4u * squad;
    v16i acc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[s] = v16i{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t w0 = 0; w0 < nw; w0 += kBmWords) {
        uint4 pre = make_uint4(0, 0, 0, 0);   // (stride % 128 == 0: a 16-byte word that starts below nw ends in the row)
        if (w0 + 4u * squad < nw) pre = *reinterpret_cast<const uint4 *>(src + w0);
        uint4 qa = *reinterpret_cast<const uint4 *>(qw + w0), qb = make_uint4(0, 0, 0, 0);
        if (w0 + 4u < nw) qb = *reinterpret_cast<const uint4 *>(qw + w0 + 4);
        if (w0) __syncthreads();   // every wave has left the previous stage
        const uint32_t wv[4] = {pre.x, pre.y, pre.z, pre.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t c = 2u * (4u * squad + j), sw = srow & 15u;
            *reinterpret_cast<v4i *>(xs + srow * 256u + 16u * (c ^ sw)) = bin_half_pm1(wv[j]);
            *reinterpret_cast<v4i *>(xs + srow * 256u + 16u * ((c + 1u) ^ sw)) = bin_half_pm1(wv[j] >> 16);
        }
        __syncthreads();
        const uint32_t qv[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
#pragma unroll
        for (int t = 0; t < (int)kBmWords; ++t) {
            if (w0 + t >= nw) break;   // uniform
            v4i b = bin_half_pm1(qv[t] >> (16u * h));
            if (w0 + t >= full) b &= bin_half_mask(tail >> (16u * h));   // the partial word: bytes at or past dim are 0
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const v4i a = *reinterpret_cast<const v4i *>(xs + (32u * s + li) * 256u + 16u * ((2u * t + h) ^ (li & 15u)));
                acc[s] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc[s], 0, 0, 0);
            }
        }
    }
    if (!qvalid) return;
    uint64_t T = 0;
    float Tf = 0.0f;
    if (p.filter) {
        T = p.thr[q];
        Tf = bf_thr_float(T);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t vrow = row0 + 32u * s + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (vrow < p.nrows) bf_emit(p, q, vrow, (float)(((int)ix.dim - acc[s][r]) >> 1), Tf, T);
        }
}

// queries per block row: 2 and 8 keep a search of one to a few queries at the rate the rows arrive; from 17 queries
// on a row word is loaded once for 32 of them (64 VALU instructions behind a 4-byte load)
static int bin_qt(uint32_t nq) { return nq <= 2 ? 2 : (nq <= 16 ? 8 : 32); }

// 16-byte loads: rows of whole 16-byte words on an aligned base
static bool bin_vec(const BfIndexDev &ix) { return (ix.stride & 127u) == 0 && (reinterpret_cast<uintptr_t>(ix.qrows) & 15u) == 0; }

// Smallest batch that takes the matrix-core pass, from the timings of DESIGN.md 3.3b-ii: a block row of 128 queries
// costs the pass the same whether 64 or 128 of them exist, which at 64 queries still beats the popcount pass on rows of
// 256 and 1024 bits (0.39 against 0.50 ms) and loses to it at 4096 bits (0.75 against 0.63 ms; at 128 queries 0.78
// against 1.16 ms).  Rows wider than 1024 bits therefore wait for a full block row.
#ifndef SCANN_BF_BIN_MFMA_MIN_QUERIES
#define SCANN_BF_BIN_MFMA_MIN_QUERIES 64
#endif
static bool bin_mfma(const BfIndexDev &ix, uint32_t nq) {
    return bin_vec(ix) && nq >= (uint64_t)SCANN_BF_BIN_MFMA_MIN_QUERIES * (ix.dim <= 1024 ? 1u : 2u);
}

const char *bf_bin_kernel_name(const BfIndexDev &ix, uint32_t nq) {
    return bin_mfma(ix, nq) ? "bf_hamming_mfma_kernel" : "bf_hamming_kernel";
}

int bf_bin_pass(const BfIndexDev &ix, const BfPass &p, hipStream_t st) {
    if (ix.fmt != SCANN_HIP_ROWS_BIN1 || ix.measure != SCANN_HIP_HAMMING || (ix.stride & 31u) || !p.qbits)
        return fail(SCANN_HIP_INTERNAL, "bit-row pass on a handle or a pass it cannot read");
    if (p.nq == 0 || p.nrows == 0) return SCANN_HIP_OK;
    if (bin_mfma(ix, p.nq))
        return launch(bf_hamming_mfma_kernel, dim3(ceil_div_u32(p.nrows, kBmRows), ceil_div_u32(p.nq, 128)), dim3(256), 0, st,
                      ix, p);
    const bool vec = bin_vec(ix);
    return with_value<2, 8, 32>(bin_qt(p.nq), [&](auto qt) {
        return with_value<8, 32>(ix.dim <= 256 ? 8 : 32, [&](auto ch) {
            const dim3 grid(ceil_div_u32(p.nrows, 256), ceil_div_u32(p.nq, (uint32_t)qt()));
            return vec ? launch((bf_hamming_kernel<qt(), true, ch()>), grid, dim3(256), 0, st, ix, p)
                       : launch((bf_hamming_kernel<qt(), false, ch()>), grid, dim3(256), 0, st, ix, p);
        });
    });
}

}  // namespace scann

// mmr.hip -- the MMR stage behind a search: MmrDiversifier::apply (restricts/crowding.rs:217-267) over the
// [nq][depth] rows a search with k = depth left in the workspace, with
//   sim(a, b) = -DistanceMeasure::distance(row[a], row[b])
// under the handle's measure, in the arithmetic of exact_pair_thread (pair.h; bitwise symmetric in its two rows).
//
// The rule: entry 0 of the row is selected first.  Every later round scores each entry not yet selected, in row
// order, as  score = lambda * (-dist) - (1 - lambda) * max_sim  (two f32 products and one f32 subtraction, each
// rounded: -ffp-contract=off), where max_sim is the f32::max fold of sim(entry, s) over the selected entries starting
// from f32::MIN (fmaxf drops a NaN operand as Rust's max does; a -inf similarity leaves f32::MIN).  The winner is the
// first entry whose score is strictly greater than every earlier one, the running best starting at f32::MIN; if no
// score exceeds f32::MIN (NaN, -inf, <= MIN) the lowest remaining position is taken (the reference's best_idx = 0).
//
// One 256-thread workgroup per query.  In LDS: the row's idx / dist, a max_sim slot and a selected flag per entry
// (13 bytes each, depth <= 2048) and the last selected row (dim floats).  Per round
//   1. the last selected row is copied to LDS;
//   2. every thread folds its entries' max_sim against THAT row only (a running max: nothing is recomputed against
//      earlier selections) -- the candidate's row comes from global memory, the k re-reads of a query's depth rows
//      are L2 traffic after the first round -- and forms their scores;
//   3. the workgroup reduces to the winner by (score, then lowest position): scores that do not exceed f32::MIN enter
//      the reduction AS f32::MIN, so that "nobody exceeded f32::MIN" is the same reduction's tie on position, not a
//      second pass.  Cross-lane shuffles inside a wave, one LDS step across the four waves.
// Entries are written in selection order with the plain search's distance bits.
#include <algorithm>
#include <cmath>
#include <string>

#include "launch.h"
#include "mmr.h"
#include "pair.h"

namespace scann {

namespace {

constexpr uint32_t kMmrInvalid = 0xFFFFFFFFu;
constexpr uint32_t kMmrThreads = 256;
constexpr float kF32Min = -3.40282347e+38f;   // f32::MIN

// true if (as, ap) wins over (bs, bp): the greater score, then the lower position (no score is NaN here)
__device__ __forceinline__ bool mmr_better(float as, uint32_t ap, float bs, uint32_t bp) {
    return as > bs || (as == bs && ap < bp);
}

template <int MEASURE>
__global__ __launch_bounds__(kMmrThreads) void mmr_kernel(const uint32_t *__restrict__ rows_idx,
                                                          const float *__restrict__ rows_dist,
                                                          const uint32_t *__restrict__ rows_cnt, uint32_t depth,
                                                          const float *__restrict__ data, uint64_t n, uint32_t dim,
                                                          uint32_t stride, uint32_t k, float lambda,
                                                          uint32_t *__restrict__ out_idx, float *__restrict__ out_dist,
                                                          uint32_t *__restrict__ out_cnt) {
    extern __shared__ __attribute__((aligned(16))) float s_row[];    // [dim rounded up to 4]: the last selected row
    uint32_t *s_idx = reinterpret_cast<uint32_t *>(s_row + ((dim + 3u) & ~3u));   // [depth]
    float *s_dist = reinterpret_cast<float *>(s_idx + depth);                     // [depth]
    float *s_ms = s_dist + depth;                                                 // [depth] max_sim
    uint8_t *s_sel = reinterpret_cast<uint8_t *>(s_ms + depth);                   // [depth] selected flag
    __shared__ float s_ws[kMmrThreads / 64];
    __shared__ uint32_t s_wp[kMmrThreads / 64];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t *ri = rows_idx + (size_t)q * depth;
    const float *rd = rows_dist + (size_t)q * depth;
    uint32_t *oi = out_idx + (size_t)q * k;
    float *od = out_dist + (size_t)q * k;
    const uint32_t cnt = min(rows_cnt[q], depth);   // a short row is walked to its count: no sentinel is looked up
    const uint32_t nsel = min(k, cnt);
    const float oml = 1.0f - lambda;

    for (uint32_t i = tid; i < cnt; i += kMmrThreads) {
        s_idx[i] = ri[i];
        s_dist[i] = rd[i];
        s_ms[i] = kF32Min;
        s_sel[i] = 0;
    }
    __syncthreads();
    if (nsel > 0 && tid == 0) {   // the first item: best relevance
        oi[0] = s_idx[0];
        od[0] = s_dist[0];
        s_sel[0] = 1;
    }
    uint32_t last = 0;
    for (uint32_t r = 1; r < nsel; ++r) {
        const uint32_t li = s_idx[last];
        const bool lok = (uint64_t)li < n;
        for (uint32_t j = tid; j < dim; j += kMmrThreads) s_row[j] = lok ? data[(size_t)li * stride + j] : 0.0f;
        __syncthreads();   // (also publishes s_sel[last])
        float bs = kF32Min;
        uint32_t bp = kMmrInvalid;
        for (uint32_t i = tid; i < cnt; i += kMmrThreads) {
            if (s_sel[i]) continue;
            float ms = s_ms[i];
            const uint32_t ci = s_idx[i];
            if (lok && (uint64_t)ci < n) {
                const float sim = -exact_pair_thread(MEASURE, dim, s_row, data + (size_t)ci * stride);
                ms = fmaxf(ms, sim);
                s_ms[i] = ms;
            }
            const float rel = -s_dist[i];
            const float score = lambda * rel - oml * ms;
            const float sc = score > kF32Min ? score : kF32Min;   // NaN, -inf, <= MIN: only its position competes
            if (bp == kMmrInvalid || sc > bs) {                   // ascending positions: the first of equals stays
                bs = sc;
                bp = i;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float os = __shfl_xor(bs, off);
            const uint32_t op = __shfl_xor(bp, off);
            if (mmr_better(os, op, bs, bp)) {
                bs = os;
                bp = op;
            }
        }
        if ((tid & 63u) == 0) {
            s_ws[tid >> 6] = bs;
            s_wp[tid >> 6] = bp;
        }
        __syncthreads();
        bs = s_ws[0];
        bp = s_wp[0];
#pragma unroll
        for (uint32_t w = 1; w < kMmrThreads / 64; ++w)
            if (mmr_better(s_ws[w], s_wp[w], bs, bp)) {
                bs = s_ws[w];
                bp = s_wp[w];
            }
        // r < nsel <= cnt: an entry remains, so bp is a position of the row
        if (tid == 0) {
            oi[r] = s_idx[bp];
            od[r] = s_dist[bp];
            s_sel[bp] = 1;
        }
        last = bp;
    }
    for (uint32_t i = nsel + tid; i < k; i += kMmrThreads) {
        oi[i] = kMmrInvalid;
        od[i] = INFINITY;
    }
    if (tid == 0) out_cnt[q] = nsel;
}

}  // namespace

int mmr_launch(const uint32_t *rows_idx, const float *rows_dist, const uint32_t *rows_cnt, uint32_t nq, uint32_t depth,
               const float *data, uint64_t n, uint32_t dim, uint32_t stride, int measure, uint32_t k, float lambda,
               uint32_t *out_idx, float *out_dist, uint32_t *out_cnt, hipStream_t st) {
    if (nq == 0) return SCANN_HIP_OK;
    if (depth == 0 || depth > kMmrMaxDepth)
        return fail(SCANN_HIP_UNIMPLEMENTED, "MMR depth " + std::to_string(depth) + " exceeds " + std::to_string(kMmrMaxDepth));
    if (k > depth) return fail(SCANN_HIP_INVALID_ARGUMENT, "MMR: depth < k");
    if (!(lambda >= 0.0f && lambda <= 1.0f)) return fail(SCANN_HIP_INVALID_ARGUMENT, "MMR: lambda outside [0, 1]");
    if (!data && n > 0) return fail(SCANN_HIP_FAILED_PRECONDITION, "MMR: the handle holds no f32 rows");
    const size_t lds = (size_t)((dim + 3u) & ~3u) * 4 + (size_t)depth * 13;
    return with_measure(measure, [&](auto M) {
        return launch(mmr_kernel<decltype(M)::value>, dim3(nq), dim3(kMmrThreads), lds, st, rows_idx, rows_dist, rows_cnt,
                      depth, data, n, dim, stride, k, lambda, out_idx, out_dist, out_cnt);
    });
}

}  // namespace scann

// sparse_dev.h -- what the two sparse scans share (sparse.hip: every CSR entry past a query panel; sparse_inv.hip:
// row-blocked posting lists): the handle, the measures' epilogue, the append-and-bitonic selection in
// LDS, and the entry points of sparse_inv.hip that sparse.hip's driver calls.  Device code: for .hip units only.
#pragma once
#include <mutex>

#include "common.h"
#include "sparse.h"

struct scann_hip_sparse_index {
    int device = 0;
    uint64_t n = 0, nnz = 0;
    uint32_t dimensionality = 0;
    int measure = SCANN_HIP_DOT_PRODUCT;
    scann::DevBuf d_off, d_dims, d_vals, d_norm, d_len;
    // row-blocked postings (scann_hip_sparse_build_postings): block b's directory is entries [blk_dir[b], blk_dir[b + 1])
    // of dir_dim (ascending dimensions) and dir_start (the list's first posting; dir_start[entries] = nnz); the postings
    // are two planes, the row inside the block and the value, ascending by row inside a list
    bool inv = false;
    uint32_t inv_blocks = 0;
    scann::DevBuf inv_blk_dir, inv_dir_dim, inv_dir_start, inv_rows, inv_vals;
    uint64_t inv_bytes = 0, inv_chunks = 0, inv_visited = 0;   // (the last two: of the last posting-list search)
    // searches: one stream and grow-only buffers, one call at a time
    std::mutex mu;
    hipStream_t stream = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    bool timed = false, stats = false;
    uint64_t plan[5] = {0, 0, 0, 0, 0};
    scann::DevBuf q_off, q_dims, q_vals, q_norm, tiles, allow, partial, out_idx, out_dist, out_count, dist, d_stats;
    ~scann_hip_sparse_index() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace scann {

// The queries of a search as sparse.hip's driver uploaded them, the filter, and where the scan's results go.
struct SparseInvArgs {
    const uint64_t *q_off;
    const uint32_t *q_dims;
    const float *q_vals;
    const float *q_norm;
    uint32_t nq;
    const uint64_t *allow;
    uint32_t allow_bits;
    uint32_t k, chunk_blocks, chunks;
    uint64_t *partial;            // [nq][chunks][k]
    float *out;                   // the distances entry: [nq][n]; null for a search
    unsigned long long *stats;    // [0] postings visited
};

// sparse_inv.hip: the posting-list scan of a handle that has postings, enqueued on the handle's stream
int sparse_inv_scan(scann_hip_sparse_index *ix, const SparseInvArgs &a);

__device__ __forceinline__ float sparse_distance(int measure, float acc, uint32_t xlen, float xn2, uint32_t qlen, float qn2) {
    switch (measure) {
        case SCANN_HIP_COSINE: {
            const float nq = sqrtf(qn2), nx = sqrtf(xn2);
            const float sim = (nq == 0.0f || nx == 0.0f) ? 0.0f : acc / (nq * nx);
            return 1.0f - sim;
        }
        case SCANN_HIP_SPARSE_JACCARD: {
            if (qlen == 0 && xlen == 0) return 0.0f;
            const uint32_t c = (uint32_t)acc;
            return 1.0f - (float)c / (float)((uint64_t)qlen + xlen - c);
        }
        case SCANN_HIP_SPARSE_DICE: {
            if (qlen == 0 && xlen == 0) return 0.0f;
            return 1.0f - (2.0f * (float)(uint32_t)acc) / (float)((uint64_t)qlen + xlen);
        }
        case SCANN_HIP_SPARSE_NONZERO_INTERSECT: return (float)(-(int32_t)acc);
        default: return -acc;
    }
}

// sparse.hip: the merge of a search's chunk partials ([nq][chunks][k] keys, chunks * k <= kSparseMergeKeys) into the final
// rows, enqueued on `stream`; the stacked-quantizer scan (stacked.hip) ends in it too
int sparse_merge(const uint64_t *partial, uint32_t nq, uint32_t chunks, uint32_t k, uint32_t *out_idx, float *out_dist,
                 uint32_t *out_count, hipStream_t stream);

// NBUF buffers of 2^cap_log keys each, sorted ascending side by side: one barrier per pass for all of them.  THREADS: the
// workgroup's size.
template <uint32_t NBUF, uint32_t THREADS = kSparseThreads>
__device__ void sparse_sort_buffers(uint64_t *buf, uint32_t cap_log) {
    const uint32_t half_log = cap_log - 1, pairs = NBUF << half_log;
    for (uint32_t lk = 1; lk <= cap_log; ++lk) {
        for (int lj = (int)lk - 1; lj >= 0; --lj) {
            for (uint32_t i = threadIdx.x; i < pairs; i += THREADS) {
                const uint32_t b = i >> half_log, ii = i & ((1u << half_log) - 1);
                const uint32_t lo = ((ii >> lj) << (lj + 1)) | (ii & ((1u << lj) - 1)), hi = lo + (1u << lj);
                uint64_t *p = buf + ((size_t)b << cap_log);
                const uint64_t x = p[lo], y = p[hi];
                const bool up = ((lo >> lk) & 1u) == 0;
                if ((x > y) == up) {
                    p[lo] = y;
                    p[hi] = x;
                }
            }
            __syncthreads();
        }
    }
}

// pads every buffer past its count, sorts, cuts to k and moves the thresholds.  Every thread of the workgroup calls.
template <uint32_t NBUF, uint32_t THREADS = kSparseThreads>
__device__ void sparse_compact(uint64_t *buf, uint32_t cap_log, uint32_t k, uint32_t *cnt, uint64_t *thr) {
    for (uint32_t i = threadIdx.x; i < (NBUF << cap_log); i += THREADS)
        if ((i & ((1u << cap_log) - 1)) >= cnt[i >> cap_log]) buf[i] = SCANN_KEY_MAX;
    __syncthreads();
    sparse_sort_buffers<NBUF, THREADS>(buf, cap_log);
    if (threadIdx.x < NBUF) {
        const uint32_t c = min(cnt[threadIdx.x], k);
        cnt[threadIdx.x] = c;
        if (c == k) thr[threadIdx.x] = buf[((size_t)threadIdx.x << cap_log) + k - 1];
    }
    __syncthreads();
}

}  // namespace scann

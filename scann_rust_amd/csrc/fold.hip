// fold.hip -- the CSR / code half of scann_hip_fold_mutable (scann_hip.h "fold"): the old index's leaves, less the
// removed rows, merged with the delta rows into new leaf offsets, ids and packed codes, every leaf in ascending new
// datapoint index.  Nothing here re-assigns or re-encodes a base row.
//
// A CSR position p of the old index survives when the row leaf_ids[p] is live.  The new datapoint index of base row r
// is new_index(r) = (live base rows below r) + (delta ids below r's external id): export_live's destination, defined for
// removed rows too and monotone in r.  With leaves strictly ascending in datapoint index (checked), new_index is
// monotone along a leaf, so a leaf's survivors keep their relative order and the delta rows of the leaf are merged
// between them by binary search -- no sort, and no workgroup owns a leaf: the index is cut into chunks of
// kMutFoldChunk CSR positions whatever the leaf boundaries, so a flat hasher's single leaf is shared by n / chunk
// workgroups like any other.
//
// Kernels:
//   fold_count_kernel         one workgroup per chunk: survivor bitmap over CSR positions (one ballot per wave and 64
//                             positions), survivors per chunk, the ascending / range check into the flag word
//   fold_scan_kernel          exclusive scan in place (one workgroup): chunk counts, the delta's per-leaf histogram
//   fold_delta_rank_kernel    per delta row (ascending id): its leaf and its rank among the delta rows of that leaf
//                             (tokens of the rows before it stream through LDS; at most 65 536 rows), histogram
//   fold_delta_list_kernel    the delta rows grouped by leaf, ascending inside a leaf
//   fold_offsets_kernel       new_off[l] = survivors below leaf l + delta rows of the leaves below l
//   fold_scatter_base_kernel  one workgroup per chunk: survivor -> new_off[l] + survivors of l before it + delta rows
//                             of l with a smaller new index; ids remapped, code words copied through an LDS list of
//                             destinations so that reads are contiguous
//   fold_scatter_delta_kernel delta row -> new_off[l] + its rank + survivors of l with a smaller new index; its byte
//                             codes packed into words
#include "fold.h"
#include "launch.h"
#include "mutable.h"

namespace scann {

namespace {

constexpr uint32_t kFoldThreads = 256;
constexpr uint32_t kFoldPasses = kMutFoldChunk / kFoldThreads;
constexpr uint32_t kFoldWords = kMutFoldChunk / 64;   // survivor-bitmap words per chunk
constexpr uint32_t kFoldNone = 0xFFFFFFFFu;
static_assert(kMutFoldChunk % kFoldThreads == 0 && kFoldThreads % 64 == 0, "a wave covers one bitmap word");

// first index in [lo, hi) with a[index] >= v (hi if none)
__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t *a, uint32_t lo, uint32_t hi, uint32_t v) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the leaf that holds CSR position p (p < leaf_off[L]): the last l with leaf_off[l] <= p, so empty leaves are skipped
__device__ __forceinline__ uint32_t leaf_of_position(const uint32_t *leaf_off, uint32_t L, uint32_t p) {
    uint32_t lo = 0, hi = L + 1;   // first index with leaf_off[index] > p
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (leaf_off[mid] <= p) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// survivors in CSR positions below p (p <= n)
__device__ __forceinline__ uint32_t survivors_before(const FoldArgs &a, uint64_t p) {
    const uint64_t c = p / kMutFoldChunk, g = p >> 6;
    uint32_t s = a.cpref[c];
    for (uint64_t w = c * kFoldWords; w < g; ++w) s += (uint32_t)__popcll(a.sbits[w]);
    if (p & 63u) s += (uint32_t)__popcll(a.sbits[g] & ((1ull << (p & 63u)) - 1ull));
    return s;
}

// new datapoint index of base row r (r < n), live or removed
__device__ __forceinline__ uint32_t new_index(const FoldArgs &a, uint32_t r) {
    const uint64_t word = a.live[r >> 6];
    const uint32_t rank = a.live_prefix[r >> 6] + (uint32_t)__popcll(word & ((1ull << (r & 63u)) - 1ull));
    const uint32_t ext = a.base_ids ? a.base_ids[r] : r;
    return rank + lower_bound_u32(a.sorted_ids, 0, a.nd, ext);
}

__global__ __launch_bounds__(kFoldThreads) void fold_count_kernel(FoldArgs a) {
    __shared__ uint32_t s_cnt[kFoldThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t count = 0, bad = 0;
    for (uint32_t pass = 0; pass < kFoldPasses; ++pass) {
        const uint64_t p = (uint64_t)blockIdx.x * kMutFoldChunk + pass * kFoldThreads + tid;
        bool alive = false;
        if (p < a.n) {
            const uint32_t r = a.leaf_ids ? a.leaf_ids[p] : (uint32_t)p;
            if (r >= a.n) {
                bad |= 2u;
            } else {
                alive = (a.live[r >> 6] >> (r & 63u)) & 1ull;
                if (a.leaf_ids && p > 0 && a.leaf_ids[p - 1] >= r) {   // allowed only where a leaf starts at p
                    const uint32_t idx = lower_bound_u32(a.leaf_off, 0, a.L + 1, (uint32_t)p);
                    if (idx > a.L || a.leaf_off[idx] != (uint32_t)p) bad |= 1u;
                }
            }
        }
        const unsigned long long m = __ballot(alive);
        if (lane == 0) a.sbits[p >> 6] = m;   // (the scratch covers whole chunks: words past n are written as 0)
        count += (uint32_t)__popcll(m);
    }
    if (lane == 0) s_cnt[wave] = count;
    __syncthreads();
    if (tid == 0) {
        uint32_t tot = 0;
        for (uint32_t w = 0; w < kFoldThreads / 64; ++w) tot += s_cnt[w];
        a.cpref[blockIdx.x] = tot;
    }
    if (bad) atomicOr(a.flag, bad);
}

// v[0..len) -> its exclusive prefix in place, v[len] = the total; one workgroup of 1024 threads
__global__ __launch_bounds__(1024) void fold_scan_kernel(uint32_t *v, uint64_t len) {
    __shared__ uint32_t s_w[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t carry = 0;
    for (uint64_t base = 0; base < len; base += 1024) {
        const uint64_t i = base + tid;
        const uint32_t c = i < len ? v[i] : 0u;
        uint32_t incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
            if ((int)lane >= o) incl += up;
        }
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        uint32_t wbase = 0, tot = 0;
        for (uint32_t w = 0; w < 16; ++w) {
            if (w < wave) wbase += s_w[w];
            tot += s_w[w];
        }
        if (i < len) v[i] = carry + wbase + incl - c;
        carry += tot;
        __syncthreads();
    }
    if (tid == 0) v[len] = carry;
}

__global__ __launch_bounds__(kFoldThreads) void fold_delta_rank_kernel(FoldArgs a) {
    __shared__ uint32_t s_tok[kFoldThreads];
    const uint32_t tid = threadIdx.x, i = blockIdx.x * kFoldThreads + tid;
    const bool act = i < a.nd;
    uint32_t l = 0, rank = i;
    if (a.tok_slot) {   // (kernel-uniform)
        if (act) l = a.tok_slot[a.order[i]];
        rank = 0;
        for (uint32_t t = 0; t <= blockIdx.x; ++t) {
            const uint32_t x = t * kFoldThreads + tid;
            s_tok[tid] = x < a.nd ? a.tok_slot[a.order[x]] : kFoldNone;
            __syncthreads();
            const uint32_t lim = t < blockIdx.x ? kFoldThreads : tid;   // the rows before row i
            for (uint32_t y = 0; y < lim; ++y) rank += s_tok[y] == l ? 1u : 0u;
            __syncthreads();
        }
    }
    if (!act) return;
    if (l >= a.L) {   // (the assignment kernel never answers this)
        atomicOr(a.flag, 2u);
        l = 0;
    }
    a.dtok[i] = l;
    a.drank[i] = rank;
    atomicAdd(&a.doff[l], 1u);
}

__global__ void fold_delta_list_kernel(FoldArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.nd) return;
    const uint32_t at = a.doff[a.dtok[i]] + a.drank[i];
    if (at < a.nd) a.dlist[at] = i;
}

__global__ void fold_offsets_kernel(FoldArgs a) {
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l > a.L) return;
    const uint32_t sb = survivors_before(a, a.leaf_off[l]);
    a.sbase[l] = sb;
    a.new_off[l] = sb + a.doff[l];
    if (l == a.L) a.new_off[a.L + 1] = *a.flag;
}

__global__ __launch_bounds__(kFoldThreads) void fold_scatter_base_kernel(FoldArgs a) {
    __shared__ uint32_t s_dest[kFoldThreads];
    const uint32_t tid = threadIdx.x;
    for (uint32_t pass = 0; pass < kFoldPasses; ++pass) {
        const uint64_t p0 = (uint64_t)blockIdx.x * kMutFoldChunk + pass * kFoldThreads;
        if (p0 >= a.n) break;   // (block-uniform)
        const uint64_t p = p0 + tid;
        uint32_t dest = kFoldNone;
        if (p < a.n) {
            const uint32_t r = a.leaf_ids ? a.leaf_ids[p] : (uint32_t)p;
            if (r < a.n && ((a.live[r >> 6] >> (r & 63u)) & 1ull)) {
                const uint32_t l = leaf_of_position(a.leaf_off, a.L, (uint32_t)p);
                const uint32_t before = survivors_before(a, p) - a.sbase[l];
                const uint32_t j = new_index(a, r);
                uint32_t lo = a.doff[l], hi = a.doff[l + 1];   // delta rows of the leaf with a smaller new index
                const uint32_t first = lo;
                while (lo < hi) {
                    const uint32_t mid = lo + ((hi - lo) >> 1);
                    if (a.dj[a.dlist[mid]] < j) lo = mid + 1;
                    else hi = mid;
                }
                const uint64_t d = (uint64_t)a.new_off[l] + before + (lo - first);
                if (d < a.n_new) {
                    dest = (uint32_t)d;
                    if (a.new_ids) a.new_ids[d] = j;
                }
            }
        }
        s_dest[tid] = dest;
        __syncthreads();
        for (uint32_t e = tid; e < kFoldThreads * a.nw; e += kFoldThreads) {
            const uint32_t q = e / a.nw, w = e - q * a.nw;
            const uint32_t d = s_dest[q];
            if (d != kFoldNone) a.new_codes[(size_t)d * a.nw + w] = a.codes[(size_t)(p0 + q) * a.nw + w];
        }
        __syncthreads();
    }
}

__global__ void fold_scatter_delta_kernel(FoldArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.nd) return;
    const uint32_t l = a.dtok[i], j = a.dj[i];
    uint32_t lo = a.leaf_off[l], hi = a.leaf_off[l + 1];   // first position of the leaf whose row does not come before j
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint32_t r = a.leaf_ids ? a.leaf_ids[mid] : mid;
        if (r < a.n && new_index(a, r) < j) lo = mid + 1;
        else hi = mid;
    }
    const uint64_t d = (uint64_t)a.new_off[l] + a.drank[i] + (survivors_before(a, lo) - a.sbase[l]);
    if (d >= a.n_new) return;
    if (a.new_ids) a.new_ids[d] = j;
    const uint8_t *c = a.code8 + (size_t)a.order[i] * a.S;
    const uint32_t per = a.bits == 4 ? 8u : 4u;   // subspaces per word
    for (uint32_t w = 0; w < a.nw; ++w) {
        uint32_t word = 0;
        for (uint32_t s = 0; s < per; ++s) {
            const uint32_t v = c[w * per + s];
            word |= a.bits == 4 ? (v & 15u) << (4 * s) : v << (8 * s);
        }
        a.new_codes[(size_t)d * a.nw + w] = word;
    }
}

}  // namespace

int fold_clear(const FoldArgs &a, hipStream_t st) {
    SCANN_HIP_CHECK(hipMemsetAsync(a.doff, 0, ((size_t)a.L + 1) * 4, st));
    SCANN_HIP_CHECK(hipMemsetAsync(a.flag, 0, 4, st));
    return SCANN_HIP_OK;
}

int fold_count(const FoldArgs &a, hipStream_t st) {
    const uint64_t chunks = ceil_div_u64(a.n, kMutFoldChunk);
    if (chunks == 0 || chunks > 0x7FFFFFFFull) return fail(SCANN_HIP_INTERNAL, "fold: bad chunk count");
    SCANN_TRY(launch(fold_count_kernel, dim3((uint32_t)chunks), dim3(kFoldThreads), 0, st, a));
    SCANN_TRY(launch(fold_scan_kernel, dim3(1), dim3(1024), 0, st, a.cpref, chunks));
    const uint32_t dgrid = ceil_div_u32(a.nd, kFoldThreads);
    if (a.nd) SCANN_TRY(launch(fold_delta_rank_kernel, dim3(dgrid), dim3(kFoldThreads), 0, st, a));
    SCANN_TRY(launch(fold_scan_kernel, dim3(1), dim3(1024), 0, st, a.doff, (uint64_t)a.L));
    if (a.nd) SCANN_TRY(launch(fold_delta_list_kernel, dim3(dgrid), dim3(kFoldThreads), 0, st, a));
    return launch(fold_offsets_kernel, dim3(ceil_div_u32(a.L + 1, 256)), dim3(256), 0, st, a);
}

int fold_scatter(const FoldArgs &a, hipStream_t st) {
    const uint64_t chunks = ceil_div_u64(a.n, kMutFoldChunk);
    SCANN_TRY(launch(fold_scatter_base_kernel, dim3((uint32_t)chunks), dim3(kFoldThreads), 0, st, a));
    if (a.nd)
        SCANN_TRY(launch(fold_scatter_delta_kernel, dim3(ceil_div_u32(a.nd, kFoldThreads)), dim3(kFoldThreads), 0, st, a));
    return SCANN_HIP_OK;
}

}  // namespace scann

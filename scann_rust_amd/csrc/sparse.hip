// sparse.hip -- sparse brute force: rows in CSR on the device, a batch of sparse queries scored
// against all of them.  SparseDataset + BruteForceSearcher of the reference, pair by pair through dot_product_sparse, the
// sparse branch of cosine_similarity, jaccard_distance_sparse, dice_distance_sparse and non_zero_intersect_distance
// (distance_measures/one_to_one.rs:412-436, 473-490; distance_measures/sparse.rs).
//
//   sparse_prepare_kernel   one thread per row: the checks of scann_hip_sparse_create, the row's length and its
//                           sequential f32 squared norm (datapoint.rs:146-151).
//   sparse_scan_kernel      grid (query tiles, row chunks), 16 waves.
//     A  panel    the tile's queries (at most 16, lengths summing to at most 1024) become an LDS panel[slot][16] of
//                 f32, one slot per distinct dimension of the tile, found through an open-addressing map
//                 (u32 key, u16 slot, home = dim % 2048, linear probing, atomicCAS inserts).
//     B  scan     a wave takes four consecutive rows at a time and streams their CSR elements 64 per fetch, across
//                 the row boundaries.  Every lane probes the map for its element (a miss, the common case, ends
//                 there).  The hits stay in their lanes' registers; lane (r, j) walks the hit lanes of row r in
//                 ascending lane order -- ascending dimension -- fetching (slot, value) by ds_bpermute and adding
//                 panel[slot][j] * value to the one accumulator of (row r, query j).  One chain per pair, no atomics.
//     C  select   the measure's epilogue, the allow bitmap, and per query of the tile an LDS append buffer with a
//                 running threshold, sorted and cut to k whenever a further round could overflow it; the k best keys of
//                 the chunk go to partial[query][chunk][k].
//   sparse_merge_kernel     one workgroup per query: sorts the chunk partials in LDS, writes the final rows.
// A handle that has postings (scann_hip_sparse_build_postings) keeps this driver and the merge and swaps the scan for
// sparse_inv.hip's; what the two scans share (the handle, the epilogue, the LDS selection) is in sparse_dev.h.
#include <memory>
#include <vector>

#include "comm.h"   // ctx_device
#include "launch.h"
#include "sparse_dev.h"

namespace scann {
namespace {

constexpr uint32_t kPrepThreads = 256, kMergeThreads = 256;
constexpr uint32_t kMapMask = kSparseMap - 1;

struct SparseScanArgs {
    // rows
    const uint64_t *row_off;
    const uint32_t *dims;
    const float *vals;
    const float *row_norm;
    const uint32_t *row_len;
    uint32_t n, chunk_rows;
    // queries
    const uint64_t *q_off;
    const uint32_t *q_dims;
    const float *q_vals;
    const float *q_norm;
    const uint32_t *tile_start;
    int measure;
    // selection
    const uint64_t *allow;
    uint32_t allow_bits;
    uint32_t k, cap_log, chunks;
    uint64_t *partial;            // [nq][chunks][k]
    float *out;                   // the distances entry: [nq][n]
    unsigned long long *stats;    // [0] elements probed, [1] probes, [2] hits
};

__device__ __forceinline__ bool finite_bits(float v) { return (__builtin_bit_cast(uint32_t, v) & 0x7F800000u) != 0x7F800000u; }

__global__ __launch_bounds__(kPrepThreads) void sparse_prepare_kernel(const uint64_t *__restrict__ off, const uint32_t *__restrict__ dims,
                                                                      const float *__restrict__ vals, uint32_t n, uint64_t nnz,
                                                                      uint32_t dimensionality, float *__restrict__ norm,
                                                                      uint32_t *__restrict__ len, uint32_t *bad) {
    const uint64_t row = (uint64_t)blockIdx.x * kPrepThreads + threadIdx.x;
    if (row >= n) return;
    const uint64_t o0 = off[row], o1 = off[row + 1];
    float s = 0.0f;
    // a strictly ascending list of u32 below 2^32 - 1 is shorter than 2^32: longer rows are refused unread
    bool ok = o0 <= o1 && o1 <= nnz && o1 - o0 <= 0xFFFFFFFFull;
    if (ok) {
        uint32_t prev = 0;
        for (uint64_t e = o0; e < o1; ++e) {
            const uint32_t d = dims[e];
            const float v = vals[e];
            if (d >= dimensionality || (e > o0 && d <= prev) || !finite_bits(v)) {
                ok = false;
                break;
            }
            prev = d;
            s += v * v;
        }
    }
    norm[row] = s;
    len[row] = ok ? (uint32_t)(o1 - o0) : 0u;
    if (!ok) atomicOr(bad, 1u);
}

// the value a stored entry contributes: itself (DotProduct, Cosine), 1 for being stored (Jaccard, Dice), 1 for being
// non-zero (NonZeroIntersect) -- products of these, summed in f32, are the sum or the exact count (<= 1024 < 2^24)
__device__ __forceinline__ float sparse_term(int mode, float v) { return mode == 0 ? v : mode == 1 ? 1.0f : (v != 0.0f ? 1.0f : 0.0f); }

// slot of dimension d (one is always free: the map is at most half full); false on a miss.  *probes counts key reads.
__device__ __forceinline__ bool sparse_probe(const uint32_t *keys, uint32_t d, uint32_t *pos, uint32_t *probes) {
    uint32_t h = d & kMapMask;
    for (;;) {
        const uint32_t key = keys[h];
        ++*probes;
        if (key == d) {
            *pos = h;
            return true;
        }
        if (key == kSparseEmpty) return false;
        h = (h + 1) & kMapMask;
    }
}

__device__ __forceinline__ uint64_t low_mask(uint32_t bits) { return bits >= 64 ? ~0ull : (1ull << bits) - 1ull; }
// lanes of a fetch that starts at element `base` which lie before element `o`
__device__ __forceinline__ uint32_t lanes_before(uint64_t o, uint64_t base) { return o <= base ? 0u : (o - base >= 64 ? 64u : (uint32_t)(o - base)); }

template <bool SELECT, bool STATS>
__global__ __launch_bounds__(kSparseThreads) void sparse_scan_kernel(const SparseScanArgs a) {
    extern __shared__ __align__(16) unsigned char sparse_lds[];
    float *panel = reinterpret_cast<float *>(sparse_lds);                                   // [kSparseSlots][kSparseQT]
    uint32_t *keys = reinterpret_cast<uint32_t *>(panel + kSparseSlots * kSparseQT);        // [kSparseMap]
    uint16_t *slots = reinterpret_cast<uint16_t *>(keys + kSparseMap);                      // [kSparseMap]
    uint64_t *buf = reinterpret_cast<uint64_t *>(slots + kSparseMap);                       // [kSparseQT][1 << cap_log]
    __shared__ uint32_t s_cnt[kSparseQT];
    __shared__ uint64_t s_thr[kSparseQT];
    __shared__ uint32_t s_nslots;

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t r = lane / kSparseQT, j = lane % kSparseQT;   // this lane's row of the four in flight, its query of the tile
    const uint32_t tile = blockIdx.x, chunk = blockIdx.y;
    const uint32_t q0 = a.tile_start[tile], tnq = a.tile_start[tile + 1] - q0;
    const int mode = (a.measure == SCANN_HIP_SPARSE_JACCARD || a.measure == SCANN_HIP_SPARSE_DICE) ? 1
                     : a.measure == SCANN_HIP_SPARSE_NONZERO_INTERSECT                               ? 2
                                                                                                     : 0;
    uint32_t probes = 0;   // (counted only under STATS)

    // ---- A: the panel -----------------------------------------------------------------------------------
    {
        float4 *p4 = reinterpret_cast<float4 *>(panel);
        for (uint32_t i = tid; i < kSparseSlots * kSparseQT / 4; i += kSparseThreads) p4[i] = float4{0.0f, 0.0f, 0.0f, 0.0f};
        for (uint32_t i = tid; i < kSparseMap; i += kSparseThreads) keys[i] = kSparseEmpty;
        if (tid < kSparseQT) {
            s_cnt[tid] = 0;
            s_thr[tid] = SCANN_KEY_MAX;
        }
        if (tid == 0) s_nslots = 0;
        __syncthreads();
        const uint64_t e0 = a.q_off[q0], e1 = a.q_off[q0 + tnq];   // (at most kSparseSlots elements: the planner's rule)
        for (uint64_t e = e0 + tid; e < e1; e += kSparseThreads) {
            const uint32_t d = a.q_dims[e];
            uint32_t h = d & kMapMask;
            for (;;) {
                const uint32_t prev = atomicCAS(&keys[h], kSparseEmpty, d);
                if (prev == kSparseEmpty || prev == d) break;
                h = (h + 1) & kMapMask;
            }
        }
        __syncthreads();
        for (uint32_t i = tid; i < kSparseMap; i += kSparseThreads)
            if (keys[i] != kSparseEmpty) slots[i] = (uint16_t)atomicAdd(&s_nslots, 1u);
        __syncthreads();
        for (uint32_t jq = 0; jq < tnq; ++jq) {
            for (uint64_t e = a.q_off[q0 + jq] + tid; e < a.q_off[q0 + jq + 1]; e += kSparseThreads) {
                uint32_t pos = 0, unused = 0;
                if (sparse_probe(keys, a.q_dims[e], &pos, &unused)) panel[(uint32_t)slots[pos] * kSparseQT + jq] = sparse_term(mode, a.q_vals[e]);
            }
        }
        __syncthreads();
    }

    // ---- B, C: the chunk's rows, kSparseRoundRows per round ------------------------------------------------
    const bool qvalid = j < tnq;
    const uint32_t q = q0 + (qvalid ? j : 0u);
    const uint32_t qlen = (uint32_t)(a.q_off[q + 1] - a.q_off[q]);
    const float qn2 = a.q_norm[q];
    const uint32_t cap_log = a.cap_log;
    const uint64_t c0 = (uint64_t)chunk * a.chunk_rows;
    const uint64_t c1 = c0 + a.chunk_rows < a.n ? c0 + a.chunk_rows : a.n;
    const uint32_t rounds = (uint32_t)((c1 - c0 + kSparseRoundRows - 1) / kSparseRoundRows);
    unsigned long long n_el = 0, n_hit = 0;

    for (uint32_t round = 0; round < rounds; ++round) {
        for (uint32_t g = 0; g < kSparseGroups; ++g) {
            const uint64_t g0 = c0 + (uint64_t)round * kSparseRoundRows + (wave * kSparseGroups + g) * kSparseRowsInFlight;
            if (g0 >= c1) continue;   // (the whole wave)
            const uint64_t row = g0 + r;
            const uint64_t g1 = g0 + kSparseRowsInFlight < c1 ? g0 + kSparseRowsInFlight : c1;
            // rows past the chunk are empty ranges at the group's end
            const uint64_t o_lo = a.row_off[row < g1 ? row : g1], o_hi = a.row_off[row + 1 < g1 ? row + 1 : g1];
            const uint64_t gs = a.row_off[g0], ge = a.row_off[g1];
            float acc = 0.0f;
            uint32_t d_next = kSparseEmpty;
            float v_next = 0.0f;
            if (gs + lane < ge) {
                d_next = a.dims[gs + lane];
                if (mode != 1) v_next = a.vals[gs + lane];
            }
            for (uint64_t base = gs; base < ge; base += 64) {
                const uint32_t d = d_next;
                const float v = v_next;
                d_next = kSparseEmpty;
                if (base + 64 + lane < ge) {   // the next fetch is in flight while this one is probed
                    d_next = a.dims[base + 64 + lane];
                    if (mode != 1) v_next = a.vals[base + 64 + lane];
                }
                uint32_t pos = 0;
#ifdef SCANN_SPARSE_SKIP_PROBE   // (tools/time_sparse.py's variant builds: wrong answers, the stream alone)
                const bool hit = false;
                acc += d == 0x12345u ? v : 0.0f;
#else
                const bool hit = d != kSparseEmpty && sparse_probe(keys, d, &pos, &probes);
#endif
                const uint32_t slot = hit ? (uint32_t)slots[pos] : 0u;   // (slot 0 is readable whoever asks)
                const float term = sparse_term(mode, v);
                if (STATS) {
                    n_el += d != kSparseEmpty ? 1u : 0u;
                    n_hit += hit ? 1u : 0u;
                }
#ifdef SCANN_SPARSE_SKIP_WALK   // (variant build: stream and probes, every hit used once by its own lane, no walk)
                acc += hit ? term * (float)slot : 0.0f;
#else
                // the hit lanes of this lane's row, lowest first: ascending dimension
                uint64_t m = __ballot(hit) & low_mask(lanes_before(o_hi, base)) & ~low_mask(lanes_before(o_lo, base));
                while (__any(m != 0ull)) {   // (uniform: every lane takes part in the exchange)
                    const bool act = m != 0ull;
                    const int src = act ? __builtin_ctzll(m) : 0;
                    m &= m - 1ull;
                    const uint32_t s = (uint32_t)__shfl((int)slot, src);
                    const float x = __shfl(term, src);
                    const float p = panel[s * kSparseQT + j];
                    if (act) acc += p * x;
                }
#endif
            }
            if (row < g1 && qvalid) {
                const uint32_t rw = (uint32_t)row;
                const float dist = sparse_distance(a.measure, acc, a.row_len[rw], a.row_norm[rw], qlen, qn2);
                if (!SELECT) {
                    a.out[(size_t)q * a.n + rw] = dist;
                } else if (!a.allow || (rw < a.allow_bits && ((a.allow[rw >> 6] >> (rw & 63u)) & 1ull))) {
                    const uint64_t key = make_key(dist, rw);
                    // (the buffer has room: it held at most cap - kSparseRoundRows keys when the round began)
                    if (key < s_thr[j]) buf[((size_t)j << cap_log) + atomicAdd(&s_cnt[j], 1u)] = key;
                }
            }
        }
        if (SELECT) {
            __syncthreads();   // the round's appends are done
            // one decision for the workgroup: the counts are read before the second barrier, the next round's appends
            // come after it, so no thread can see a count another has already moved
            const int full = __syncthreads_or(tid < kSparseQT && s_cnt[tid] > (1u << cap_log) - kSparseRoundRows);
            if (full) sparse_compact<kSparseQT>(buf, cap_log, a.k, s_cnt, s_thr);
        }
    }
    if (SELECT) {
        __syncthreads();
        sparse_compact<kSparseQT>(buf, cap_log, a.k, s_cnt, s_thr);
        for (uint32_t i = tid; i < tnq * a.k; i += kSparseThreads) {
            const uint32_t jq = i / a.k, ii = i % a.k;
            a.partial[((size_t)(q0 + jq) * a.chunks + chunk) * a.k + ii] = buf[((size_t)jq << cap_log) + ii];
        }
    }
    if (STATS) {
        unsigned long long pr = probes;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            pr += shfl_xor_t<uint64_t>(pr, o);
            n_el += shfl_xor_t<uint64_t>(n_el, o);
            n_hit += shfl_xor_t<uint64_t>(n_hit, o);
        }
        if (lane == 0) {
            atomicAdd(&a.stats[0], n_el);
            atomicAdd(&a.stats[1], pr);
            atomicAdd(&a.stats[2], n_hit);
        }
    }
}

// one workgroup per query: the chunks' k best keys, sorted; the first k are the answer
__global__ __launch_bounds__(kMergeThreads) void sparse_merge_kernel(const uint64_t *__restrict__ partial, uint32_t total, uint32_t npad,
                                                                     uint32_t k, uint32_t *__restrict__ out_idx,
                                                                     float *__restrict__ out_dist, uint32_t *__restrict__ out_count) {
    extern __shared__ __align__(16) unsigned char sparse_lds[];
    uint64_t *keys = reinterpret_cast<uint64_t *>(sparse_lds);
    const uint32_t q = blockIdx.x;
    for (uint32_t i = threadIdx.x; i < npad; i += kMergeThreads) keys[i] = i < total ? partial[(size_t)q * total + i] : SCANN_KEY_MAX;
    __syncthreads();
    bitonic_sort_lds(keys, npad);
    for (uint32_t i = threadIdx.x; i < k; i += kMergeThreads) {
        const uint64_t key = keys[i];
        out_idx[(size_t)q * k + i] = (uint32_t)key;                       // (SCANN_KEY_MAX: 0xFFFFFFFF, +NaN)
        out_dist[(size_t)q * k + i] = ordered_to_f32((uint32_t)(key >> 32));
        if (key != SCANN_KEY_MAX && (i + 1 == k || keys[i + 1] == SCANN_KEY_MAX)) out_count[q] = i + 1;
    }
    if (threadIdx.x == 0 && keys[0] == SCANN_KEY_MAX) out_count[q] = 0;
}

}  // namespace

int sparse_merge(const uint64_t *partial, uint32_t nq, uint32_t chunks, uint32_t k, uint32_t *out_idx, float *out_dist,
                 uint32_t *out_count, hipStream_t stream) {
    const uint32_t total = chunks * k, npad = next_pow2_u32(total);
    return launch(sparse_merge_kernel, dim3(nq), dim3(kMergeThreads), (size_t)npad * 8, stream, partial, total, npad, k, out_idx, out_dist,
                  out_count);
}

}  // namespace scann

using namespace scann;

namespace {

// queries checked, planned and uploaded; the scan launched (with k: the selection and the merge); results copied back
int sparse_run(scann_hip_sparse_index *ix, const uint64_t *q_offsets, const uint32_t *q_dims, const float *q_vals, uint32_t nq,
               uint32_t k, const uint64_t *allow, uint64_t allow_bits, uint32_t *out_idx, float *out_dist, uint32_t *out_count,
               float *out) {
    const bool select = out == nullptr;
    if (!q_offsets) return fail(SCANN_HIP_INVALID_ARGUMENT, "q_offsets is null");
    const uint64_t qnnz = q_offsets[nq] - q_offsets[0];
    if (q_offsets[nq] < q_offsets[0] || (qnnz && (!q_dims || !q_vals))) return fail(SCANN_HIP_INVALID_ARGUMENT, "null query dims/values");
    std::vector<float> norms;
    const char *why = "";
    if (sparse_check_queries(q_offsets, q_dims, q_vals, nq, ix->dimensionality, &norms, &why) != SCANN_HIP_OK)
        return fail(SCANN_HIP_INVALID_ARGUMENT, why);
    std::vector<uint32_t> starts;
    if (sparse_plan_tiles(q_offsets, nq, &starts) != SCANN_HIP_OK)
        return fail(SCANN_HIP_UNIMPLEMENTED, "a query has more entries than SCANN_HIP_SPARSE_TILE_SLOTS");
    std::lock_guard<std::mutex> lock(ix->mu);
    ix->timed = false;
    for (uint64_t &p : ix->plan) p = 0;
    ix->inv_chunks = ix->inv_visited = 0;
    if (select) {   // what a search that launches nothing leaves: no rows, the halves of the all-ones key
        for (uint32_t i = 0; i < nq; ++i) out_count[i] = 0;
        for (size_t i = 0; i < (size_t)nq * k; ++i) {
            out_idx[i] = 0xFFFFFFFFu;
            out_dist[i] = ordered_to_f32(0xFFFFFFFFu);
        }
    }
    if (ix->n == 0 || nq == 0) return SCANN_HIP_OK;
    const uint32_t n = (uint32_t)ix->n, ntiles = (uint32_t)starts.size() - 1;
    const bool inv = ix->inv;   // the posting-list route (sparse_inv.hip): chunks are whole blocks of rows
    uint32_t chunk_rows = 0, chunks = 0;
    if (inv) sparse_inv_chunks(ix->inv_blocks, select ? kSparseMergeKeys / k : 65535u, &chunk_rows, &chunks);
    else sparse_chunks(n, select ? kSparseMergeKeys / k : 65535u, &chunk_rows, &chunks);
    if (allow_bits > n) allow_bits = n;
    std::vector<uint64_t> rel((size_t)nq + 1);
    for (uint32_t i = 0; i <= nq; ++i) rel[i] = q_offsets[i] - q_offsets[0];

    SCANN_HIP_CHECK(hipSetDevice(ix->device));
    hipStream_t st = ix->stream;
    SCANN_TRY(ix->q_off.ensure(rel.size() * 8));
    SCANN_TRY(ix->q_dims.ensure(qnnz * 4));
    SCANN_TRY(ix->q_vals.ensure(qnnz * 4));
    SCANN_TRY(ix->q_norm.ensure((size_t)nq * 4));
    SCANN_TRY(ix->tiles.ensure(starts.size() * 4));
    SCANN_TRY(ix->d_stats.ensure(24));
    SCANN_HIP_CHECK(hipMemcpyAsync(ix->q_off.p, rel.data(), rel.size() * 8, hipMemcpyHostToDevice, st));
    if (qnnz) {
        SCANN_HIP_CHECK(hipMemcpyAsync(ix->q_dims.p, q_dims, qnnz * 4, hipMemcpyHostToDevice, st));
        SCANN_HIP_CHECK(hipMemcpyAsync(ix->q_vals.p, q_vals, qnnz * 4, hipMemcpyHostToDevice, st));
    }
    SCANN_HIP_CHECK(hipMemcpyAsync(ix->q_norm.p, norms.data(), (size_t)nq * 4, hipMemcpyHostToDevice, st));
    SCANN_HIP_CHECK(hipMemcpyAsync(ix->tiles.p, starts.data(), starts.size() * 4, hipMemcpyHostToDevice, st));
    const size_t allow_words = allow ? (size_t)((allow_bits + 63) / 64) : 0;
    if (allow) {
        SCANN_TRY(ix->allow.ensure(allow_words * 8));
        if (allow_words) SCANN_HIP_CHECK(hipMemcpyAsync(ix->allow.p, allow, allow_words * 8, hipMemcpyHostToDevice, st));
    }
    SCANN_HIP_CHECK(hipMemsetAsync(ix->d_stats.p, 0, 24, st));
    if (select) {
        SCANN_TRY(ix->partial.ensure((size_t)nq * chunks * k * 8));
        SCANN_TRY(ix->out_idx.ensure((size_t)nq * k * 4));
        SCANN_TRY(ix->out_dist.ensure((size_t)nq * k * 4));
        SCANN_TRY(ix->out_count.ensure((size_t)nq * 4));
    } else {
        SCANN_TRY(ix->dist.ensure((size_t)nq * n * 4));
    }
    SCANN_HIP_CHECK(hipStreamSynchronize(st));   // the pageable copies have left the host vectors

    SparseScanArgs a{};
    a.row_off = ix->d_off.as<uint64_t>();
    a.dims = ix->d_dims.as<uint32_t>();
    a.vals = ix->d_vals.as<float>();
    a.row_norm = ix->d_norm.as<float>();
    a.row_len = ix->d_len.as<uint32_t>();
    a.n = n;
    a.chunk_rows = chunk_rows;
    a.q_off = ix->q_off.as<uint64_t>();
    a.q_dims = ix->q_dims.as<uint32_t>();
    a.q_vals = ix->q_vals.as<float>();
    a.q_norm = ix->q_norm.as<float>();
    a.tile_start = ix->tiles.as<uint32_t>();
    a.measure = ix->measure;
    a.allow = allow ? ix->allow.as<uint64_t>() : nullptr;
    a.allow_bits = (uint32_t)allow_bits;
    a.k = k;
    a.chunks = chunks;
    a.partial = ix->partial.as<uint64_t>();
    a.out = ix->dist.as<float>();
    a.stats = ix->d_stats.as<unsigned long long>();
    uint32_t cap_log = 0;
    while ((1u << cap_log) < sparse_select_cap(k)) ++cap_log;
    a.cap_log = cap_log;

    const dim3 grid(ntiles, chunks), block(kSparseThreads);
    const size_t lds = sparse_scan_lds(k, select);
    SCANN_HIP_CHECK(hipEventRecord(ix->ev[0], st));
    if (inv) {
        SparseInvArgs v{};
        v.q_off = a.q_off;
        v.q_dims = a.q_dims;
        v.q_vals = a.q_vals;
        v.q_norm = a.q_norm;
        v.nq = nq;
        v.allow = a.allow;
        v.allow_bits = a.allow_bits;
        v.k = k;
        v.chunk_blocks = chunk_rows;
        v.chunks = chunks;
        v.partial = a.partial;
        v.out = select ? nullptr : a.out;
        v.stats = ix->stats ? a.stats : nullptr;
        SCANN_TRY(sparse_inv_scan(ix, v));
    } else if (select) {
        if (ix->stats) SCANN_TRY(launch(sparse_scan_kernel<true, true>, grid, block, lds, st, a));
        else SCANN_TRY(launch(sparse_scan_kernel<true, false>, grid, block, lds, st, a));
    } else {
        if (ix->stats) SCANN_TRY(launch(sparse_scan_kernel<false, true>, grid, block, lds, st, a));
        else SCANN_TRY(launch(sparse_scan_kernel<false, false>, grid, block, lds, st, a));
    }
    SCANN_HIP_CHECK(hipEventRecord(ix->ev[1], st));
    if (select) {
        SCANN_TRY(sparse_merge(ix->partial.as<uint64_t>(), nq, chunks, k, ix->out_idx.as<uint32_t>(), ix->out_dist.as<float>(),
                               ix->out_count.as<uint32_t>(), st));
    }
    SCANN_HIP_CHECK(hipEventRecord(ix->ev[2], st));
    if (select) {
        SCANN_HIP_CHECK(hipMemcpyAsync(out_idx, ix->out_idx.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost, st));
        SCANN_HIP_CHECK(hipMemcpyAsync(out_dist, ix->out_dist.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost, st));
        SCANN_HIP_CHECK(hipMemcpyAsync(out_count, ix->out_count.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    } else {
        SCANN_HIP_CHECK(hipMemcpyAsync(out, ix->dist.p, (size_t)nq * n * 4, hipMemcpyDeviceToHost, st));
    }
    uint64_t stats[3] = {0, 0, 0};
    if (ix->stats) SCANN_HIP_CHECK(hipMemcpyAsync(stats, ix->d_stats.p, 24, hipMemcpyDeviceToHost, st));
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    ix->timed = true;
    if (inv) {   // (the plan stays all zero: it describes exhaustive scans)
        ix->inv_chunks = chunks;
        ix->inv_visited = stats[0];
        return SCANN_HIP_OK;
    }
    ix->plan[0] = ntiles;
    ix->plan[1] = chunks;
    ix->plan[2] = stats[0];
    ix->plan[3] = stats[1];
    ix->plan[4] = stats[2];
    return SCANN_HIP_OK;
}

}  // namespace

extern "C" {

int scann_hip_sparse_create(scann_hip_ctx *ctx, const uint64_t *row_offsets, const uint32_t *dims, const float *vals, uint64_t n,
                            uint32_t dimensionality, int measure, scann_hip_sparse_index **out) {
    if (!out) return fail(SCANN_HIP_INVALID_ARGUMENT, "out is null");
    *out = nullptr;
    if (!ctx) return fail(SCANN_HIP_INVALID_ARGUMENT, "context is null");
    switch (measure) {
        case SCANN_HIP_DOT_PRODUCT:
        case SCANN_HIP_COSINE:
        case SCANN_HIP_SPARSE_JACCARD:
        case SCANN_HIP_SPARSE_DICE:
        case SCANN_HIP_SPARSE_NONZERO_INTERSECT: break;
        case SCANN_HIP_SQUARED_L2:
        case SCANN_HIP_L2:
        case SCANN_HIP_L1:
            return fail(SCANN_HIP_UNIMPLEMENTED, "sparse SquaredL2 / L2 / L1 sum over the union of the index lists: not built");
        default: return fail(SCANN_HIP_INVALID_ARGUMENT, "unknown measure");
    }
    if (n >= 0xFFFFFFFFull) return fail(SCANN_HIP_OUT_OF_RANGE, "n must be below 2^32 - 1");
    if (n && !row_offsets) return fail(SCANN_HIP_INVALID_ARGUMENT, "row_offsets is null");
    if (n && row_offsets[0] != 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "row_offsets[0] must be 0");
    const uint64_t nnz = n ? row_offsets[n] : 0;
    if (nnz && (!dims || !vals)) return fail(SCANN_HIP_INVALID_ARGUMENT, "null dims/vals with stored entries");
    std::unique_ptr<scann_hip_sparse_index> ix(new scann_hip_sparse_index());
    ix->device = ctx_device(ctx);
    ix->n = n;
    ix->nnz = nnz;
    ix->dimensionality = dimensionality;
    ix->measure = measure;
    SCANN_HIP_CHECK(hipSetDevice(ix->device));
    SCANN_HIP_CHECK(hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking));
    for (hipEvent_t &e : ix->ev) SCANN_HIP_CHECK(hipEventCreate(&e));
    if (n) {
        SCANN_TRY(upload(ix->d_off, row_offsets, (n + 1) * 8));
        SCANN_TRY(upload(ix->d_dims, dims, nnz * 4));
        SCANN_TRY(upload(ix->d_vals, vals, nnz * 4));
        SCANN_TRY(ix->d_norm.ensure(n * 4));
        SCANN_TRY(ix->d_len.ensure(n * 4));
        DevBuf bad;
        const uint32_t zero = 0;
        SCANN_TRY(upload(bad, &zero, 4));
        SCANN_TRY(launch(sparse_prepare_kernel, dim3((uint32_t)ceil_div_u64(n, kPrepThreads)), dim3(kPrepThreads), 0, ix->stream,
                         ix->d_off.as<uint64_t>(), ix->d_dims.as<uint32_t>(), ix->d_vals.as<float>(), (uint32_t)n, nnz, dimensionality,
                         ix->d_norm.as<float>(), ix->d_len.as<uint32_t>(), bad.as<uint32_t>()));
        uint32_t flag = 0;
        SCANN_HIP_CHECK(hipMemcpyAsync(&flag, bad.p, 4, hipMemcpyDeviceToHost, ix->stream));
        SCANN_HIP_CHECK(hipStreamSynchronize(ix->stream));
        if (flag)
            return fail(SCANN_HIP_INVALID_ARGUMENT,
                        "sparse rows: offsets must be monotone, dims strictly ascending and below the dimensionality, values finite");
    }
    *out = ix.release();
    return SCANN_HIP_OK;
}

void scann_hip_sparse_destroy(scann_hip_sparse_index *index) {
    if (!index) return;
    (void)hipSetDevice(index->device);
    delete index;
}

uint64_t scann_hip_sparse_size(const scann_hip_sparse_index *index) { return index ? index->n : 0; }

uint64_t scann_hip_sparse_device_bytes(const scann_hip_sparse_index *index) {
    if (!index || !index->n) return 0;
    return index->d_off.bytes + index->d_dims.bytes + index->d_vals.bytes + index->d_norm.bytes + index->d_len.bytes + index->inv_bytes;
}

int scann_hip_sparse_search_batched(scann_hip_sparse_index *index, const uint64_t *q_offsets, const uint32_t *q_dims, const float *q_vals,
                                    uint32_t nq, uint32_t k, const uint64_t *allow_bitmap, uint64_t allow_bitmap_bits, uint32_t *out_idx,
                                    float *out_dist, uint32_t *out_count) {
    if (!index) return fail(SCANN_HIP_INVALID_ARGUMENT, "index is null");
    if (k == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "k must be at least 1");
    if (k > kSparseMaxK) return fail(SCANN_HIP_UNIMPLEMENTED, "k above SCANN_HIP_SPARSE_MAX_K");
    if (nq && (!out_idx || !out_dist || !out_count)) return fail(SCANN_HIP_INVALID_ARGUMENT, "null output pointer");
    return sparse_run(index, q_offsets, q_dims, q_vals, nq, k, allow_bitmap, allow_bitmap_bits, out_idx, out_dist, out_count, nullptr);
}

int scann_hip_sparse_distances(scann_hip_sparse_index *index, const uint64_t *q_offsets, const uint32_t *q_dims, const float *q_vals,
                               uint32_t nq, float *out) {
    if (!index) return fail(SCANN_HIP_INVALID_ARGUMENT, "index is null");
    if (!out) return fail(SCANN_HIP_INVALID_ARGUMENT, "out is null");
    return sparse_run(index, q_offsets, q_dims, q_vals, nq, 1, nullptr, 0, nullptr, nullptr, nullptr, out);
}

void scann_hip_sparse_last_kernel_ms(scann_hip_sparse_index *index, float *out_ms) {
    if (!out_ms) return;
    out_ms[0] = out_ms[1] = 0.0f;
    if (!index) return;
    std::lock_guard<std::mutex> lock(index->mu);
    if (!index->timed) return;
    if (hipEventElapsedTime(&out_ms[0], index->ev[0], index->ev[1]) != hipSuccess ||
        hipEventElapsedTime(&out_ms[1], index->ev[1], index->ev[2]) != hipSuccess) {
        clear_last_hip_error();
        out_ms[0] = out_ms[1] = 0.0f;
    }
}

void scann_hip_sparse_enable_stats(scann_hip_sparse_index *index, int enable) {
    if (!index) return;
    std::lock_guard<std::mutex> lock(index->mu);
    index->stats = enable != 0;
}

void scann_hip_sparse_last_plan(scann_hip_sparse_index *index, uint64_t *out) {
    if (!out) return;
    for (int i = 0; i < 5; ++i) out[i] = 0;
    if (!index) return;
    std::lock_guard<std::mutex> lock(index->mu);
    for (int i = 0; i < 5; ++i) out[i] = index->plan[i];
}

}  // extern "C"

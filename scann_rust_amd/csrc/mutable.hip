// mutable.hip -- mutable indexes (scann_hip.h "mutable indexes"; mutator/mod.rs): an immutable base handle, a
// resident live bitmap over its rows, a dense delta segment of added / changed rows, and the search that merges them.
//
// Kernels:
//   live_clear_kernel          clears the live bits of a batch of base rows (atomicAnd on 32-bit halves of the words)
//   delta_write_kernel         scatters a batch of staged rows (and their external ids) into delta slots
//   live_and_user_*_kernel     combined[j] = live[j] & user[id of j]: word-wise AND (identity ids) or a gather through
//                              base_ids, one ballot per 64 base rows
//   delta_scan_kernel          one workgroup per (tile of kMutTile delta rows, group of queries): the group's queries are
//                              staged in LDS once, every thread scores kMutTile / 256 rows per query with
//                              exact_pair_thread (pair.h: the reference's per-pair arithmetic), keys (ordered distance,
//                              EXTERNAL id) are sorted in LDS and the first min(k, kMutTile) written: [nq][tiles][kt]
//                              partial lists, never an [nq][n_delta] matrix.  A row the user bitmap disallows never
//                              becomes a key.
//   mutable_merge_kernel       one workgroup per query: the base list (indices mapped to external ids) and the delta
//                              partial lists stream through an LDS buffer that is re-sorted per chunk, the k best
//                              staying at its front; out_count = valid keys among the first k
//   live_prefix_kernel, gather_live_kernel, scatter_delta_kernel   export_live: exclusive popcount prefix per bitmap
//                              word (one workgroup), live base rows gathered to their final position (rank among live
//                              base rows + delta ids below), delta rows scattered between them
#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "allow.h"
#include "bf.h"
#include "comm.h"
#include "fold.h"
#include "launch.h"
#include "mutable.h"
#include "pair.h"
#include "txh.h"

namespace scann {

namespace {

constexpr uint32_t kMutInvalid = 0xFFFFFFFFu;
constexpr uint32_t kMutThreads = 256;
constexpr uint32_t kMutRowsPerThread = kMutTile / kMutThreads;
constexpr uint32_t kMutMergeCap = 2048;   // keys of the merge buffer unless 2 * next_pow2(k) is larger

__global__ void live_clear_kernel(uint32_t *live32, const uint32_t *rows, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = rows[i];   // (validated on the host: r < n_base)
    atomicAnd(&live32[r >> 5], ~(1u << (r & 31u)));
}

// slots[e] == kMutInvalid: element e is superseded by a later element of the same batch
__global__ void delta_write_kernel(float4 *delta, uint32_t *delta_ids, uint32_t stride4, uint32_t capacity,
                                   const float4 *src, const uint32_t *slots, const uint32_t *ids, uint32_t n) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t e = (uint32_t)(t / stride4), c = (uint32_t)(t % stride4);
    if (e >= n) return;
    const uint32_t slot = slots[e];
    if (slot >= capacity) return;
    delta[(size_t)slot * stride4 + c] = src[(size_t)e * stride4 + c];
    if (c == 0) delta_ids[slot] = ids[e];
}

__global__ void live_and_user_words_kernel(const uint64_t *live, uint64_t words, const uint64_t *user, uint64_t user_bits,
                                           uint64_t *out) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= words) return;
    uint64_t u = 0;
    if (w * 64 < user_bits) {
        u = user[w];
        const uint64_t rest = user_bits - w * 64;   // bits at or past the capacity are ignored
        if (rest < 64) u &= (1ull << rest) - 1ull;
    }
    out[w] = live[w] & u;
}

__global__ __launch_bounds__(kMutThreads) void live_and_user_gather_kernel(const uint64_t *live, uint64_t n_base,
                                                                           const uint32_t *base_ids, const uint64_t *user,
                                                                           uint64_t user_bits, uint64_t *out) {
    const uint64_t j = (uint64_t)blockIdx.x * kMutThreads + threadIdx.x;
    bool a = false;
    if (j < n_base) {
        const uint64_t ext = base_ids[j];
        a = ext < user_bits && ((user[ext >> 6] >> (ext & 63u)) & 1ull);
    }
    const unsigned long long m = __ballot(a);
    if ((threadIdx.x & 63u) == 0 && j < n_base) out[j >> 6] = live[j >> 6] & m;
}

template <int MEASURE>
__global__ __launch_bounds__(kMutThreads) void delta_scan_kernel(const float *__restrict__ delta,
                                                                 const uint32_t *__restrict__ delta_ids, uint32_t n_delta,
                                                                 uint32_t dim, uint32_t stride,
                                                                 const float *__restrict__ queries, uint32_t nq,
                                                                 uint32_t q_stride, uint32_t qt,
                                                                 const uint64_t *__restrict__ user, uint64_t user_bits,
                                                                 int filtered, uint32_t kt, uint32_t tiles,
                                                                 uint64_t *__restrict__ pkeys) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
    uint64_t *s_keys = reinterpret_cast<uint64_t *>(s_mem);                      // [kMutTile]
    float *s_q = reinterpret_cast<float *>(s_mem + (size_t)kMutTile * 8);        // [qt][dimp]
    const uint32_t tid = threadIdx.x, tile = blockIdx.x, q0 = blockIdx.y * qt;
    const uint32_t dimp = (dim + 3u) & ~3u;
    const uint32_t nqt = min(qt, nq - q0);
    for (uint32_t i = tid; i < nqt * dimp; i += kMutThreads) {
        const uint32_t qq = i / dimp, c = i % dimp;
        s_q[i] = c < dim ? queries[(size_t)(q0 + qq) * q_stride + c] : 0.0f;
    }
    const uint32_t row0 = tile * kMutTile;
    const uint32_t in_tile = min(kMutTile, n_delta - row0);   // (tile < tiles: >= 1)
    uint32_t sort_n = 2;
    while (sort_n < in_tile) sort_n <<= 1;
    uint32_t id[kMutRowsPerThread];
#pragma unroll
    for (uint32_t r = 0; r < kMutRowsPerThread; ++r) {
        const uint32_t slot = row0 + tid + r * kMutThreads;
        id[r] = kMutInvalid;   // not a row, or not allowed: never a key
        if (slot < n_delta) {
            const uint32_t e = delta_ids[slot];
            const bool ok = !filtered || ((uint64_t)e < user_bits && ((user[e >> 6] >> (e & 63u)) & 1ull));
            if (ok) id[r] = e;
        }
    }
    __syncthreads();
    for (uint32_t qq = 0; qq < nqt; ++qq) {
#pragma unroll
        for (uint32_t r = 0; r < kMutRowsPerThread; ++r) {
            const uint32_t pos = tid + r * kMutThreads;
            if (pos >= sort_n) continue;
            uint64_t key = SCANN_KEY_MAX;
            if (id[r] != kMutInvalid) {
                const float d = exact_pair_thread(MEASURE, dim, s_q + (size_t)qq * dimp, delta + (size_t)(row0 + pos) * stride);
                key = make_key(d, id[r]);
            }
            s_keys[pos] = key;
        }
        __syncthreads();
        bitonic_sort_lds(s_keys, sort_n);
        uint64_t *out = pkeys + ((size_t)(q0 + qq) * tiles + tile) * kt;
        for (uint32_t i = tid; i < kt; i += kMutThreads) out[i] = i < sort_n ? s_keys[i] : SCANN_KEY_MAX;
        __syncthreads();
    }
}

// keep: slots at the front that survive a round (next_pow2(k)); buf: keys of the LDS buffer (a power of two)
__global__ __launch_bounds__(kMutThreads) void mutable_merge_kernel(const uint32_t *__restrict__ b_idx,
                                                                    const float *__restrict__ b_dist,
                                                                    const uint32_t *__restrict__ b_cnt, uint32_t kb,
                                                                    const uint32_t *__restrict__ base_ids, uint64_t n_base,
                                                                    const uint64_t *__restrict__ pkeys, uint32_t n_part,
                                                                    uint32_t k, uint32_t keep, uint32_t buf,
                                                                    uint32_t *__restrict__ out_idx,
                                                                    float *__restrict__ out_dist,
                                                                    uint32_t *__restrict__ out_cnt) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
    uint64_t *s = reinterpret_cast<uint64_t *>(s_mem);   // [buf]
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t total = kb + n_part;
    const uint32_t bc = b_cnt ? min(b_cnt[q], kb) : 0u;
    auto cand = [&](uint32_t c) -> uint64_t {
        if (c < kb) {
            if (c >= bc) return SCANN_KEY_MAX;
            const uint32_t bi = b_idx[(size_t)q * kb + c];
            if ((uint64_t)bi >= n_base) return SCANN_KEY_MAX;
            return make_key(b_dist[(size_t)q * kb + c], base_ids ? base_ids[bi] : bi);
        }
        if (c < total) return pkeys[(size_t)q * n_part + (c - kb)];
        return SCANN_KEY_MAX;
    };
    for (uint32_t i = tid; i < buf; i += kMutThreads) s[i] = cand(i);
    __syncthreads();
    bitonic_sort_lds(s, buf);
    for (uint32_t next = buf; next < total; next += buf - keep) {   // (buf > keep whenever total > buf)
        for (uint32_t i = tid; i < buf - keep; i += kMutThreads) s[keep + i] = cand(next + i);
        __syncthreads();
        bitonic_sort_lds(s, buf);
    }
    // an absent key (SCANN_KEY_MAX) sorts behind every real one: the valid keys of the first k form a prefix
    for (uint32_t i = tid; i < k; i += kMutThreads) {
        const uint64_t key = i < buf ? s[i] : SCANN_KEY_MAX;
        const bool valid = (uint32_t)key != kMutInvalid;
        out_idx[(size_t)q * k + i] = valid ? (uint32_t)key : kMutInvalid;
        out_dist[(size_t)q * k + i] = valid ? ordered_to_f32((uint32_t)(key >> 32)) : INFINITY;
        if (valid) {
            const uint64_t nx = (i + 1 < k && i + 1 < buf) ? s[i + 1] : SCANN_KEY_MAX;
            if (i + 1 == k || (uint32_t)nx == kMutInvalid) out_cnt[q] = i + 1;
        } else if (i == 0) {
            out_cnt[q] = 0;
        }
    }
}

// exclusive prefix of the words' popcounts; one workgroup of 1024 threads
__global__ __launch_bounds__(1024) void live_prefix_kernel(const uint64_t *live, uint64_t words, uint32_t *prefix) {
    __shared__ uint32_t s_w[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t carry = 0;
    for (uint64_t base = 0; base < words; base += 1024) {
        const uint64_t w = base + tid;
        const uint32_t c = w < words ? (uint32_t)__popcll(live[w]) : 0u;
        uint32_t incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
            if ((int)lane >= o) incl += up;
        }
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        uint32_t wbase = 0, tot = 0;
        for (uint32_t i = 0; i < 16; ++i) {
            if (i < wave) wbase += s_w[i];
            tot += s_w[i];
        }
        if (w < words) prefix[w] = carry + wbase + incl - c;
        carry += tot;
        __syncthreads();
    }
}

// one thread per (base row, 4-float chunk of the output row); sorted_delta_ids ascending
__global__ void gather_live_kernel(const float *__restrict__ rows, uint32_t dim, uint32_t in_stride, uint32_t stride4,
                                   const uint64_t *__restrict__ live, const uint32_t *__restrict__ prefix, uint64_t n_base,
                                   const uint32_t *__restrict__ base_ids, const uint32_t *__restrict__ sorted_delta_ids,
                                   uint32_t n_delta, float4 *__restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t j = t / stride4;
    const uint32_t c = (uint32_t)(t % stride4);
    if (j >= n_base) return;
    const uint64_t word = live[j >> 6];
    if (!((word >> (j & 63u)) & 1ull)) return;
    const uint32_t rank = prefix[j >> 6] + (uint32_t)__popcll(word & ((1ull << (j & 63u)) - 1ull));
    const uint32_t ext = base_ids ? base_ids[j] : (uint32_t)j;
    uint32_t lo = 0, hi = n_delta;   // delta ids below ext
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sorted_delta_ids[mid] < ext) lo = mid + 1;
        else hi = mid;
    }
    const float *src = rows + (size_t)j * in_stride;
    float4 v;
    v.x = 4 * c + 0 < dim ? src[4 * c + 0] : 0.0f;
    v.y = 4 * c + 1 < dim ? src[4 * c + 1] : 0.0f;
    v.z = 4 * c + 2 < dim ? src[4 * c + 2] : 0.0f;
    v.w = 4 * c + 3 < dim ? src[4 * c + 3] : 0.0f;
    out[(size_t)(rank + lo) * stride4 + c] = v;
}

__global__ void scatter_delta_kernel(const float4 *__restrict__ delta, uint32_t stride4, const uint32_t *__restrict__ dest,
                                     uint32_t n_delta, float4 *__restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t s = (uint32_t)(t / stride4), c = (uint32_t)(t % stride4);
    if (s >= n_delta) return;
    out[(size_t)dest[s] * stride4 + c] = delta[(size_t)s * stride4 + c];
}

}  // namespace

}  // namespace scann

using namespace scann;

struct scann_hip_mutable {
    scann_hip_ctx *ctx = nullptr;
    scann_hip_index *base = nullptr;
    BaseView bv;
    std::mutex mu;
    hipStream_t st = nullptr;
    uint32_t dim = 0, stride = 0, capacity = 0;
    uint64_t n_base = 0, live_base = 0;
    // external ids of the base rows: identity until a rebase passes a list (strictly ascending)
    bool identity = true;
    std::vector<uint32_t> base_ids;
    DevBuf d_base_ids;
    std::vector<uint64_t> live;   // host mirror of d_live
    DevBuf d_live;
    // delta segment: rows [capacity][stride], ids [capacity]; slots [0, n_delta) are live
    DevBuf d_delta, d_delta_ids;
    std::vector<uint32_t> delta_ids;
    // ids that are not plain base rows: the delta slot, or kRemoved for a removed id that has no base row.  A base row
    // whose id is absent here is live or removed by its bit.
    static constexpr uint32_t kRemoved = 0xFFFFFFFFu;
    std::unordered_map<uint32_t, uint32_t> over;
    uint32_t next_index = 0;
    uint64_t pending = 0;
    DevBuf st_rows, st_a, st_b;   // staging of one mutation batch
    DevBuf q, user, comb, b_idx, b_dist, b_cnt, pkeys, o_idx, o_dist, o_cnt;   // search
    DevBuf x_prefix, x_sorted, x_dest, x_out;                                   // export
    bool timing = false;
    hipEvent_t ev[6] = {};
    bool ran[3] = {false, false, false};
    hipEvent_t fev[6] = {};    // fold: created by the first fold
    float fold_ms[5] = {};     // stages of the last fold (scann_hip_fold_mutable_stage_ms)

    uint32_t n_delta() const { return (uint32_t)delta_ids.size(); }
    static constexpr uint64_t kNoRow = ~0ull;
    uint64_t base_row(uint32_t id) const {
        if (identity) return id < n_base ? id : kNoRow;
        auto it = std::lower_bound(base_ids.begin(), base_ids.end(), id);
        return it != base_ids.end() && *it == id ? (uint64_t)(it - base_ids.begin()) : kNoRow;
    }
    bool bit(uint64_t r) const { return (live[r >> 6] >> (r & 63u)) & 1ull; }
    bool known(uint32_t id) const { return over.count(id) || base_row(id) != kNoRow; }
    bool in_delta(uint32_t id, uint32_t *slot) const {
        auto it = over.find(id);
        if (it == over.end() || it->second == kRemoved) return false;
        if (slot) *slot = it->second;
        return true;
    }
};

namespace {

int check_base(const scann_hip_index *base, BaseView *bv) {
    SCANN_TRY(index_base_view(base, bv));
    if (bv->brute_force) {
        if (bv->quantized) return fail(SCANN_HIP_UNIMPLEMENTED, "mutable index over quantized brute-force rows is not built");
        return SCANN_HIP_OK;
    }
    if (bv->partitioned) return fail(SCANN_HIP_UNIMPLEMENTED, "mutable index over SearchMode::Partitioned is not built");
    if (bv->sharded) return fail(SCANN_HIP_UNIMPLEMENTED, "mutable index over a shard (leaf_sizes_global) is not built");
    if (bv->quantized) return fail(SCANN_HIP_UNIMPLEMENTED, "mutable index over quantized rows is not built");
    if (bv->projected) return fail(SCANN_HIP_UNIMPLEMENTED, "mutable index over a base that searches through a projection is not built");
    if (!bv->rows) return fail(SCANN_HIP_UNIMPLEMENTED, "mutable index needs a base that stores its rows");
    if (bv->rows_csr) return fail(SCANN_HIP_UNIMPLEMENTED, "mutable index needs rows stored by datapoint index");
    return SCANN_HIP_OK;
}

int set_dev(const scann_hip_mutable *m) {
    SCANN_HIP_CHECK(hipSetDevice(ctx_device(m->ctx)));
    return SCANN_HIP_OK;
}

// every base row live, empty delta
int reset_state(scann_hip_mutable *m) {
    const uint64_t words = (m->n_base + 63) / 64;
    m->live.assign(words, ~0ull);
    if (m->n_base & 63u) m->live[words - 1] = (1ull << (m->n_base & 63u)) - 1ull;
    m->live_base = m->n_base;
    SCANN_TRY(upload(m->d_live, m->live.data(), words * 8));
    m->delta_ids.clear();
    m->over.clear();
    m->pending = 0;
    return SCANN_HIP_OK;
}

// staging of a batch of n elements, allocated BEFORE the host state is touched: an allocation failure leaves the handle
// as it was (the ensure calls of write_rows / clear_bits then find the buffers in place)
int reserve_batch(scann_hip_mutable *m, uint32_t n, bool rows) {
    if (rows) {
        SCANN_TRY(m->st_rows.ensure((size_t)n * m->stride * 4));
        SCANN_TRY(m->st_b.ensure((size_t)n * 8));
    }
    return m->st_a.ensure((size_t)n * 4);
}

int clear_bits(scann_hip_mutable *m, const std::vector<uint32_t> &rows) {
    if (rows.empty()) return SCANN_HIP_OK;
    const uint32_t n = (uint32_t)rows.size();
    SCANN_TRY(m->st_a.ensure((size_t)n * 4));
    SCANN_HIP_CHECK(hipMemcpyAsync(m->st_a.p, rows.data(), (size_t)n * 4, hipMemcpyHostToDevice, m->st));
    return launch(live_clear_kernel, dim3(ceil_div_u32(n, 256)), dim3(256), 0, m->st, m->d_live.as<uint32_t>(),
                  m->st_a.as<uint32_t>(), n);
}

// rows[e] -> delta slot slots[e] under id ids[e]; of several elements with one slot the last is written
int write_rows(scann_hip_mutable *m, const float *rows, uint32_t n, uint32_t row_stride, std::vector<uint32_t> &slots,
               const std::vector<uint32_t> &ids, std::vector<float> &stage) {
    std::unordered_map<uint32_t, uint32_t> last;
    for (uint32_t e = 0; e < n; ++e) last[slots[e]] = e;
    for (uint32_t e = 0; e < n; ++e)
        if (last[slots[e]] != e) slots[e] = kMutInvalid;
    stage.assign((size_t)n * m->stride, 0.0f);
    for (uint32_t e = 0; e < n; ++e)
        std::memcpy(&stage[(size_t)e * m->stride], rows + (size_t)e * row_stride, (size_t)m->dim * 4);
    SCANN_TRY(m->st_rows.ensure(stage.size() * 4));
    SCANN_TRY(m->st_b.ensure((size_t)n * 8));
    uint32_t *d_slots = m->st_b.as<uint32_t>(), *d_ids = d_slots + n;
    SCANN_HIP_CHECK(hipMemcpyAsync(m->st_rows.p, stage.data(), stage.size() * 4, hipMemcpyHostToDevice, m->st));
    SCANN_HIP_CHECK(hipMemcpyAsync(d_slots, slots.data(), (size_t)n * 4, hipMemcpyHostToDevice, m->st));
    SCANN_HIP_CHECK(hipMemcpyAsync(d_ids, ids.data(), (size_t)n * 4, hipMemcpyHostToDevice, m->st));
    const uint32_t stride4 = m->stride / 4;
    const uint64_t threads = (uint64_t)n * stride4;
    return launch(delta_write_kernel, dim3((uint32_t)ceil_div_u64(threads, 256)), dim3(256), 0, m->st,
                  m->d_delta.as<float4>(), m->d_delta_ids.as<uint32_t>(), stride4, m->capacity, m->st_rows.as<float4>(),
                  d_slots, d_ids, n);
}

int sync(scann_hip_mutable *m) {
    SCANN_HIP_CHECK(hipStreamSynchronize(m->st));
    return SCANN_HIP_OK;
}

// stages 2 and 3 on the handle's stream: the delta partial lists, then the merge with the base rows in m->b_*
// (have_base) into m->o_*
int delta_and_merge(scann_hip_mutable *m, uint32_t nq, uint32_t q_stride, uint32_t k, uint32_t kb, bool have_base,
                    bool filtered, uint64_t user_bits) {
    const uint32_t nd = m->n_delta();
    const uint32_t tiles = ceil_div_u32(nd, kMutTile), kt = std::min(k, kMutTile);
    const uint32_t n_part = tiles * kt;
    m->ran[1] = false;
    if (nd > 0) {
        SCANN_TRY(m->pkeys.ensure((size_t)nq * n_part * 8));
        const uint32_t dimp = (m->dim + 3u) & ~3u;
        const size_t q_budget = 48 * 1024;
        uint32_t qt = (uint32_t)std::min<size_t>(8, q_budget / ((size_t)dimp * 4));
        if (qt == 0) qt = 1;
        qt = std::min(qt, nq);
        const size_t lds = (size_t)kMutTile * 8 + (size_t)qt * dimp * 4;
        if (ceil_div_u32(nq, qt) > 65535u)
            return fail(SCANN_HIP_UNIMPLEMENTED, "mutable search: more than " + std::to_string(65535u * qt) + " queries per call");
        if (m->timing) SCANN_HIP_CHECK(hipEventRecord(m->ev[2], m->st));
        SCANN_TRY(with_measure(m->bv.measure, [&](auto M) {
            return launch(delta_scan_kernel<decltype(M)::value>, dim3(tiles, ceil_div_u32(nq, qt)), dim3(kMutThreads), lds,
                          m->st, m->d_delta.as<float>(), m->d_delta_ids.as<uint32_t>(), nd, m->dim, m->stride,
                          m->q.as<float>(), nq, q_stride, qt, m->user.as<uint64_t>(), user_bits, filtered ? 1 : 0, kt,
                          tiles, m->pkeys.as<uint64_t>());
        }));
        if (m->timing) SCANN_HIP_CHECK(hipEventRecord(m->ev[3], m->st));
        m->ran[1] = m->timing;
    }
    SCANN_TRY(m->o_idx.ensure((size_t)nq * k * 4));
    SCANN_TRY(m->o_dist.ensure((size_t)nq * k * 4));
    SCANN_TRY(m->o_cnt.ensure((size_t)nq * 4));
    const uint32_t kbm = have_base ? kb : 0u;
    const uint32_t total = kbm + n_part;
    const uint32_t keep = next_pow2_u32(std::max(k, 1u));
    const uint32_t cap = std::max(2 * keep, kMutMergeCap);
    const uint32_t buf = std::min(next_pow2_u32(std::max(total, 2u)), cap);
    if (m->timing) SCANN_HIP_CHECK(hipEventRecord(m->ev[4], m->st));
    SCANN_TRY(launch(mutable_merge_kernel, dim3(nq), dim3(kMutThreads), (size_t)buf * 8, m->st, m->b_idx.as<uint32_t>(),
                     m->b_dist.as<float>(), have_base ? m->b_cnt.as<uint32_t>() : (const uint32_t *)nullptr, kbm,
                     m->identity ? (const uint32_t *)nullptr : m->d_base_ids.as<uint32_t>(), m->n_base,
                     m->pkeys.as<uint64_t>(), n_part, k, keep, buf, m->o_idx.as<uint32_t>(), m->o_dist.as<float>(),
                     m->o_cnt.as<uint32_t>()));
    if (m->timing) SCANN_HIP_CHECK(hipEventRecord(m->ev[5], m->st));
    m->ran[2] = m->timing;
    return SCANN_HIP_OK;
}

// The live rows in ascending external id (export_live's and fold's order): order / sorted = the delta slots / ids in
// ascending id, dest[slot] = final position of a delta row, out_ids[position] = id (live base ids and delta ids merged).
struct LiveOrder {
    std::vector<uint32_t> order, sorted, dest;
};

void plan_live_order(const scann_hip_mutable *m, LiveOrder *lo, uint32_t *out_ids) {
    const uint32_t nd = m->n_delta();
    std::vector<uint32_t> &order = lo->order, &sorted = lo->sorted, &dest = lo->dest;
    order.resize(nd);
    sorted.resize(nd);
    dest.assign(std::max(nd, 1u), 0u);
    for (uint32_t s = 0; s < nd; ++s) order[s] = s;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return m->delta_ids[a] < m->delta_ids[b]; });
    for (uint32_t i = 0; i < nd; ++i) sorted[i] = m->delta_ids[order[i]];
    uint64_t pos = 0;
    uint32_t di = 0;
    for (uint64_t j = 0; j < m->n_base; ++j) {
        if ((j & 63u) == 0 && m->live[j >> 6] == 0) {   // (a word of removed rows)
            j += 63;
            continue;
        }
        if (!m->bit(j)) continue;
        const uint32_t ext = m->identity ? (uint32_t)j : m->base_ids[j];
        while (di < nd && sorted[di] < ext) {
            dest[order[di]] = (uint32_t)pos;
            out_ids[pos++] = sorted[di++];
        }
        out_ids[pos++] = ext;
    }
    while (di < nd) {
        dest[order[di]] = (uint32_t)pos;
        out_ids[pos++] = sorted[di++];
    }
}

// What gather_live_rows reads, allocated and uploaded on the handle's stream: the sorted delta ids (x_sorted) and the
// delta rows' destinations (x_dest); room for the word-prefix of the live bitmap (x_prefix).
int gather_prepare(scann_hip_mutable *m, const LiveOrder &lo) {
    const uint32_t nd = m->n_delta();
    const uint64_t words = (m->n_base + 63) / 64;
    SCANN_TRY(m->x_prefix.ensure(std::max<uint64_t>(words, 1) * 4));
    SCANN_TRY(m->x_sorted.ensure(std::max<size_t>(nd, 1) * 4));
    SCANN_TRY(m->x_dest.ensure(std::max<size_t>(nd, 1) * 4));
    if (nd) {
        SCANN_HIP_CHECK(hipMemcpyAsync(m->x_sorted.p, lo.sorted.data(), (size_t)nd * 4, hipMemcpyHostToDevice, m->st));
        SCANN_HIP_CHECK(hipMemcpyAsync(m->x_dest.p, lo.dest.data(), (size_t)nd * 4, hipMemcpyHostToDevice, m->st));
    }
    return SCANN_HIP_OK;
}

// The live rows in that order into out ([live rows][stride] floats, device memory), on the handle's stream, after
// gather_prepare: kernel launches only.  The word-prefix of the live bitmap (x_prefix) and the sorted delta ids
// (x_sorted) stay on the device for the caller.
int gather_live_rows(scann_hip_mutable *m, float4 *out) {
    const uint32_t nd = m->n_delta();
    const hipStream_t st = m->st;
    const uint32_t stride4 = m->stride / 4;
    const uint64_t words = (m->n_base + 63) / 64;
    if (words)
        SCANN_TRY(launch(live_prefix_kernel, dim3(1), dim3(1024), 0, st, m->d_live.as<uint64_t>(), words,
                         m->x_prefix.as<uint32_t>()));
    if (m->live_base > 0) {
        const uint64_t threads = m->n_base * stride4;
        SCANN_TRY(launch(gather_live_kernel, dim3((uint32_t)ceil_div_u64(threads, 256)), dim3(256), 0, st, m->bv.rows, m->dim,
                         m->bv.stride, stride4, m->d_live.as<uint64_t>(), m->x_prefix.as<uint32_t>(), m->n_base,
                         m->identity ? (const uint32_t *)nullptr : m->d_base_ids.as<uint32_t>(), m->x_sorted.as<uint32_t>(),
                         nd, out));
    }
    if (nd) {
        const uint64_t threads = (uint64_t)nd * stride4;
        SCANN_TRY(launch(scatter_delta_kernel, dim3((uint32_t)ceil_div_u64(threads, 256)), dim3(256), 0, st,
                         m->d_delta.as<float4>(), stride4, m->x_dest.as<uint32_t>(), nd, out));
    }
    return SCANN_HIP_OK;
}

void fill_rows_empty(uint32_t nq, uint32_t k, uint32_t *out_idx, float *out_dist, uint32_t *out_count) {
    for (size_t i = 0; i < (size_t)nq * k; ++i) {
        out_idx[i] = kMutInvalid;
        out_dist[i] = INFINITY;
    }
    for (uint32_t i = 0; i < nq; ++i) out_count[i] = 0;
}

int download_rows(scann_hip_mutable *m, const DevBuf &i, const DevBuf &d, const DevBuf &c, uint32_t nq, uint32_t k,
                  uint32_t *out_idx, float *out_dist, uint32_t *out_count) {
    const size_t ob = (size_t)nq * k * 4;
    SCANN_HIP_CHECK(hipMemcpyAsync(out_idx, i.p, ob, hipMemcpyDeviceToHost, m->st));
    SCANN_HIP_CHECK(hipMemcpyAsync(out_dist, d.p, ob, hipMemcpyDeviceToHost, m->st));
    SCANN_HIP_CHECK(hipMemcpyAsync(out_count, c.p, (size_t)nq * 4, hipMemcpyDeviceToHost, m->st));
    return SCANN_HIP_OK;
}

// scann_hip_mutable_rebase under the handle's mutex.  Everything that can fail for want of memory comes first: a
// failure leaves the handle as it was.
int rebase_locked(scann_hip_mutable *m, scann_hip_index *new_base, const uint32_t *base_ids, uint64_t n) {
    BaseView bv;
    SCANN_TRY(check_base(new_base, &bv));
    if (bv.dim != m->dim) return fail(SCANN_HIP_INVALID_ARGUMENT, "rebase: the new base has another dimensionality");
    if (n != bv.n) return fail(SCANN_HIP_INVALID_ARGUMENT, "rebase: n differs from the new base's size");
    if (n >= 0xFFFFFFFFull) return fail(SCANN_HIP_OUT_OF_RANGE, "base has too many rows for u32 ids");
    if (base_ids)
        for (uint64_t j = 0; j < n; ++j)
            if (base_ids[j] == kMutInvalid || (j > 0 && base_ids[j] <= base_ids[j - 1]))
                return fail(SCANN_HIP_INVALID_ARGUMENT, "rebase: base_ids must be strictly ascending");
    SCANN_TRY(set_dev(m));
    SCANN_TRY(sync(m));
    DevBuf new_ids, new_live;
    if (base_ids) SCANN_TRY(upload(new_ids, base_ids, n * 4));
    SCANN_TRY(new_live.ensure((n + 63) / 64 * 8));
    m->d_live.take(new_live);
    m->base = new_base;
    m->bv = bv;
    m->n_base = n;
    m->identity = base_ids == nullptr;
    m->base_ids.clear();
    uint64_t past = n;   // one past the largest id in use
    if (base_ids) {
        m->base_ids.assign(base_ids, base_ids + n);
        m->d_base_ids.take(new_ids);
        past = n ? (uint64_t)base_ids[n - 1] + 1 : 0;
    }
    if (past > m->next_index) m->next_index = (uint32_t)past;
    return reset_state(m);
}

}  // namespace

extern "C" {

int scann_hip_mutable_create(scann_hip_ctx *ctx, scann_hip_index *base, uint32_t capacity, scann_hip_mutable **out) {
    if (!ctx || !base || !out) return fail(SCANN_HIP_INVALID_ARGUMENT, "null ctx/base/out");
    BaseView bv;
    SCANN_TRY(check_base(base, &bv));
    if (capacity == 0 || capacity > kMutMaxCapacity)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "delta capacity must be in [1, " + std::to_string(kMutMaxCapacity) + "]");
    if (bv.n >= 0xFFFFFFFFull) return fail(SCANN_HIP_OUT_OF_RANGE, "base has too many rows for u32 ids");
    std::unique_ptr<scann_hip_mutable> m(new scann_hip_mutable());
    m->ctx = ctx;
    m->base = base;
    m->bv = bv;
    m->dim = bv.dim;
    m->stride = scann_hip_compute_stride(bv.dim);
    m->capacity = capacity;
    m->n_base = bv.n;
    m->next_index = (uint32_t)bv.n;
    SCANN_TRY(set_dev(m.get()));
    SCANN_HIP_CHECK(hipStreamCreateWithFlags(&m->st, hipStreamNonBlocking));
    for (auto &e : m->ev) SCANN_HIP_CHECK(hipEventCreate(&e));
    SCANN_TRY(m->d_delta.ensure((size_t)capacity * m->stride * 4));
    SCANN_TRY(m->d_delta_ids.ensure((size_t)capacity * 4));
    SCANN_TRY(reset_state(m.get()));
    *out = m.release();
    return SCANN_HIP_OK;
}

void scann_hip_mutable_destroy(scann_hip_mutable *m) {
    if (!m) return;
    (void)hipSetDevice(ctx_device(m->ctx));
    if (m->st) {
        (void)hipStreamSynchronize(m->st);
        (void)hipStreamDestroy(m->st);
    }
    for (auto &e : m->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto &e : m->fev)
        if (e) (void)hipEventDestroy(e);
    delete m;
}

int scann_hip_mutable_add(scann_hip_mutable *m, const float *rows, uint32_t n, uint32_t row_stride, uint32_t dim,
                          uint32_t *out_ids) {
    if (!m) return fail(SCANN_HIP_INVALID_ARGUMENT, "handle is null");
    if (n == 0) return SCANN_HIP_OK;
    if (!rows || !out_ids) return fail(SCANN_HIP_INVALID_ARGUMENT, "null rows/out_ids");
    std::lock_guard<std::mutex> lock(m->mu);
    if (dim != m->dim || row_stride < dim)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "Dimension mismatch: expected " + std::to_string(m->dim) + ", got " + std::to_string(dim));
    if ((uint64_t)m->n_delta() + n > m->capacity)
        return fail(SCANN_HIP_RESOURCE_EXHAUSTED, "delta segment is full (capacity " + std::to_string(m->capacity) + "): export and rebase");
    if ((uint64_t)m->next_index + n > 0xFFFFFFFFull) return fail(SCANN_HIP_OUT_OF_RANGE, "out of u32 ids");
    SCANN_TRY(set_dev(m));
    SCANN_TRY(reserve_batch(m, n, true));
    std::vector<uint32_t> slots(n), ids(n);
    for (uint32_t i = 0; i < n; ++i) {
        ids[i] = m->next_index + i;
        slots[i] = m->n_delta() + i;
    }
    std::vector<float> stage;
    SCANN_TRY(write_rows(m, rows, n, row_stride, slots, ids, stage));
    for (uint32_t i = 0; i < n; ++i) {
        m->over[ids[i]] = m->n_delta();
        m->delta_ids.push_back(ids[i]);
        out_ids[i] = ids[i];
    }
    m->next_index += n;
    m->pending += n;
    return sync(m);
}

int scann_hip_mutable_remove(scann_hip_mutable *m, const uint32_t *ids, uint32_t n) {
    if (!m) return fail(SCANN_HIP_INVALID_ARGUMENT, "handle is null");
    if (n == 0) return SCANN_HIP_OK;
    if (!ids) return fail(SCANN_HIP_INVALID_ARGUMENT, "ids is null");
    std::lock_guard<std::mutex> lock(m->mu);
    for (uint32_t i = 0; i < n; ++i)
        if (!m->known(ids[i])) return fail(SCANN_HIP_NOT_FOUND, "Index " + std::to_string(ids[i]) + " not found");
    SCANN_TRY(set_dev(m));
    SCANN_TRY(reserve_batch(m, n, false));
    std::vector<uint32_t> cleared;
    bool delta_changed = false;
    const size_t row_bytes = (size_t)m->stride * 4;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t id = ids[i];
        uint32_t slot;
        const uint64_t r = m->base_row(id);
        if (m->in_delta(id, &slot)) {   // swap-remove: the last row moves into the hole
            const uint32_t last = m->n_delta() - 1;
            if (slot != last) {
                SCANN_HIP_CHECK(hipMemcpyAsync(m->d_delta.as<char>() + (size_t)slot * row_bytes,
                                               m->d_delta.as<char>() + (size_t)last * row_bytes, row_bytes,
                                               hipMemcpyDeviceToDevice, m->st));
                m->delta_ids[slot] = m->delta_ids[last];
                m->over[m->delta_ids[slot]] = slot;
            }
            m->delta_ids.pop_back();
            delta_changed = true;
            if (r != scann_hip_mutable::kNoRow) m->over.erase(id);   // (its bit is already clear)
            else m->over[id] = scann_hip_mutable::kRemoved;
        } else if (r != scann_hip_mutable::kNoRow && m->bit(r)) {
            m->live[r >> 6] &= ~(1ull << (r & 63u));
            --m->live_base;
            cleared.push_back((uint32_t)r);
        }   // else: already removed, absorbed
        ++m->pending;
    }
    SCANN_TRY(clear_bits(m, cleared));
    if (delta_changed && m->n_delta())
        SCANN_HIP_CHECK(hipMemcpyAsync(m->d_delta_ids.p, m->delta_ids.data(), (size_t)m->n_delta() * 4,
                                       hipMemcpyHostToDevice, m->st));
    return sync(m);
}

int scann_hip_mutable_update(scann_hip_mutable *m, const uint32_t *ids, const float *rows, uint32_t n,
                             uint32_t row_stride, uint32_t dim) {
    if (!m) return fail(SCANN_HIP_INVALID_ARGUMENT, "handle is null");
    if (n == 0) return SCANN_HIP_OK;
    if (!ids || !rows) return fail(SCANN_HIP_INVALID_ARGUMENT, "null ids/rows");
    std::lock_guard<std::mutex> lock(m->mu);
    if (dim != m->dim || row_stride < dim)   // (mod.rs:334-340: the dimension is compared before the id is looked up)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "Dimension mismatch: expected " + std::to_string(m->dim) + ", got " + std::to_string(dim));
    for (uint32_t i = 0; i < n; ++i)
        if (!m->known(ids[i])) return fail(SCANN_HIP_NOT_FOUND, "Index " + std::to_string(ids[i]) + " not found");
    std::unordered_set<uint32_t> fresh;
    for (uint32_t i = 0; i < n; ++i)
        if (!m->in_delta(ids[i], nullptr)) fresh.insert(ids[i]);
    if ((uint64_t)m->n_delta() + fresh.size() > m->capacity)
        return fail(SCANN_HIP_RESOURCE_EXHAUSTED, "delta segment is full (capacity " + std::to_string(m->capacity) + "): export and rebase");
    SCANN_TRY(set_dev(m));
    SCANN_TRY(reserve_batch(m, n, true));
    std::vector<uint32_t> slots(n), idv(ids, ids + n), cleared;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t id = ids[i];
        uint32_t slot;
        if (!m->in_delta(id, &slot)) {
            const uint64_t r = m->base_row(id);
            if (r != scann_hip_mutable::kNoRow && m->bit(r)) {
                m->live[r >> 6] &= ~(1ull << (r & 63u));
                --m->live_base;
                cleared.push_back((uint32_t)r);
            }
            slot = m->n_delta();
            m->delta_ids.push_back(id);
            m->over[id] = slot;
        }
        slots[i] = slot;
    }
    m->pending += n;
    std::vector<float> stage;
    SCANN_TRY(write_rows(m, rows, n, row_stride, slots, idv, stage));
    SCANN_TRY(clear_bits(m, cleared));
    return sync(m);
}

int scann_hip_mutable_get(scann_hip_mutable *m, uint32_t id, float *out_row) {
    if (!m || !out_row) return fail(SCANN_HIP_INVALID_ARGUMENT, "null handle/out_row");
    std::lock_guard<std::mutex> lock(m->mu);
    SCANN_TRY(set_dev(m));
    uint32_t slot;
    const float *src = nullptr;
    if (m->in_delta(id, &slot)) {
        src = m->d_delta.as<float>() + (size_t)slot * m->stride;
    } else {
        const uint64_t r = m->base_row(id);
        if (r != scann_hip_mutable::kNoRow && !m->over.count(id) && m->bit(r)) src = m->bv.rows + (size_t)r * m->bv.stride;
    }
    if (!src) return fail(SCANN_HIP_NOT_FOUND, "Index " + std::to_string(id) + " not found");
    SCANN_HIP_CHECK(hipMemcpyAsync(out_row, src, (size_t)m->dim * 4, hipMemcpyDeviceToHost, m->st));
    return sync(m);
}

int scann_hip_mutable_exists(scann_hip_mutable *m, uint32_t id) {
    if (!m) return 0;
    std::lock_guard<std::mutex> lock(m->mu);
    if (m->in_delta(id, nullptr)) return 1;
    const uint64_t r = m->base_row(id);
    return r != scann_hip_mutable::kNoRow && !m->over.count(id) && m->bit(r) ? 1 : 0;
}

uint64_t scann_hip_mutable_size(scann_hip_mutable *m) {
    if (!m) return 0;
    std::lock_guard<std::mutex> lock(m->mu);
    return m->live_base + m->n_delta();
}

uint64_t scann_hip_mutable_pending(scann_hip_mutable *m) {
    if (!m) return 0;
    std::lock_guard<std::mutex> lock(m->mu);
    return m->pending;
}

int scann_hip_mutable_needs_rebuild(scann_hip_mutable *m, uint64_t threshold) {
    if (!m) return 0;
    std::lock_guard<std::mutex> lock(m->mu);
    return m->pending >= threshold ? 1 : 0;
}

void scann_hip_mutable_enable_timing(scann_hip_mutable *m, int enable) {
    if (!m) return;
    std::lock_guard<std::mutex> lock(m->mu);
    m->timing = enable != 0;
    m->ran[0] = m->ran[1] = m->ran[2] = false;
}

int scann_hip_mutable_last_stage_ms(scann_hip_mutable *m, float *out_ms3) {
    if (!m || !out_ms3) return fail(SCANN_HIP_INVALID_ARGUMENT, "null handle/out");
    std::lock_guard<std::mutex> lock(m->mu);
    SCANN_TRY(set_dev(m));
    for (int s = 0; s < 3; ++s) {
        out_ms3[s] = 0.0f;
        if (!m->ran[s]) continue;
        SCANN_HIP_CHECK(hipEventSynchronize(m->ev[2 * s + 1]));
        SCANN_HIP_CHECK(hipEventElapsedTime(&out_ms3[s], m->ev[2 * s], m->ev[2 * s + 1]));
    }
    return SCANN_HIP_OK;
}

int scann_hip_mutable_search(scann_hip_mutable *m, const float *queries, uint32_t nq, uint32_t q_stride, uint32_t q_dim,
                             uint32_t k, const scann_hip_search_opts *opts, uint32_t *out_idx, float *out_dist,
                             uint32_t *out_count) {
    if (!m) return fail(SCANN_HIP_INVALID_ARGUMENT, "handle is null");
    if (nq == 0) return SCANN_HIP_OK;
    if (!queries || !out_count || (k > 0 && (!out_idx || !out_dist)))
        return fail(SCANN_HIP_INVALID_ARGUMENT, "null query/output pointer");
    std::lock_guard<std::mutex> lock(m->mu);
    if (q_dim != m->dim)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "Query dimensionality " + std::to_string(q_dim) +
                                                    " does not match dataset dimensionality " + std::to_string(m->dim));
    if (q_stride < q_dim) return fail(SCANN_HIP_INVALID_ARGUMENT, "q_stride < q_dim");
    if (k > kMutMaxK) return fail(SCANN_HIP_INVALID_ARGUMENT, "k exceeds " + std::to_string(kMutMaxK));
    scann_hip_search_opts o;
    scann_hip_search_opts_default(&o);
    if (opts) o = *opts;
    SCANN_TRY(refuse_allow_stride(&o, "mutable indexes"));
    if (!m->bv.brute_force) {
        if (!o.exact_reorder)
            return fail(SCANN_HIP_UNIMPLEMENTED, "mutable search needs exact_reorder = 1 (approximate and exact distances cannot be merged)");
        if (o.tokens || o.token_dists || o.cand_idx || o.cand_dist || o.cand_count)
            return fail(SCANN_HIP_UNIMPLEMENTED, "per-stage outputs behind a mutable search are not built");
    }
    if (k == 0) {
        fill_rows_empty(nq, 0, out_idx, out_dist, out_count);
        return SCANN_HIP_OK;
    }
    const uint32_t nd = m->n_delta();
    m->ran[0] = m->ran[1] = m->ran[2] = false;
    // no mutation at all: the plain search of the base, straight into the caller's arrays
    if (nd == 0 && m->live_base == m->n_base && m->identity)
        return scann_hip_search_batched(m->base, queries, nq, q_stride, q_dim, k, opts, out_idx, out_dist, out_count);

    SCANN_TRY(set_dev(m));
    const bool filtered = o.allow_bitmap != nullptr;
    const uint64_t user_bits = filtered ? o.allow_bitmap_bits : 0;
    const hipStream_t st = m->st;
    SCANN_TRY(m->q.ensure((size_t)nq * q_stride * 4));
    SCANN_HIP_CHECK(hipMemcpyAsync(m->q.p, queries, (size_t)nq * q_stride * 4, hipMemcpyHostToDevice, st));
    if (filtered) {
        const size_t words = (size_t)((user_bits + 63) / 64);
        SCANN_TRY(m->user.ensure(std::max<size_t>(words, 1) * 8));
        if (words) SCANN_HIP_CHECK(hipMemcpyAsync(m->user.p, o.allow_bitmap, words * 8, hipMemcpyHostToDevice, st));
    }
    // ---- stage 1: the base pass
    const uint32_t kb = m->bv.brute_force ? (uint32_t)std::min<uint64_t>(k, m->n_base) : k;
    const bool run_base = m->live_base > 0 && kb > 0;
    const uint64_t base_words = (m->n_base + 63) / 64;
    const uint64_t *d_bitmap = nullptr;
    scann_hip_search_opts ob = o;
    if (run_base) {
        if (filtered) {
            SCANN_TRY(m->comb.ensure(base_words * 8));
            if (m->identity)
                SCANN_TRY(launch(live_and_user_words_kernel, dim3((uint32_t)ceil_div_u64(base_words, 256)), dim3(256), 0, st,
                                 m->d_live.as<uint64_t>(), base_words, m->user.as<uint64_t>(), user_bits,
                                 m->comb.as<uint64_t>()));
            else
                SCANN_TRY(launch(live_and_user_gather_kernel, dim3((uint32_t)ceil_div_u64(m->n_base, kMutThreads)),
                                 dim3(kMutThreads), 0, st, m->d_live.as<uint64_t>(), m->n_base,
                                 m->d_base_ids.as<uint32_t>(), m->user.as<uint64_t>(), user_bits, m->comb.as<uint64_t>()));
            d_bitmap = m->comb.as<uint64_t>();
        } else if (m->live_base < m->n_base) {
            d_bitmap = m->d_live.as<uint64_t>();
        }
        ob.allow_bitmap = d_bitmap;
        ob.allow_bitmap_bits = d_bitmap ? m->n_base : 0;
        SCANN_TRY(m->b_idx.ensure((size_t)nq * kb * 4));
        SCANN_TRY(m->b_dist.ensure((size_t)nq * kb * 4));
        SCANN_TRY(m->b_cnt.ensure((size_t)nq * 4));
        if (m->timing) SCANN_HIP_CHECK(hipEventRecord(m->ev[0], st));
        int s = scann_hip_search_batched_device(m->base, m->q.as<float>(), nq, q_stride, kb, &ob, m->b_idx.as<uint32_t>(),
                                                m->b_dist.as<float>(), m->b_cnt.as<uint32_t>(), st);
        if (s != SCANN_HIP_OK) {
            (void)hipStreamSynchronize(st);   // (the uploads read the caller's memory)
            return s;
        }
        if (m->timing) SCANN_HIP_CHECK(hipEventRecord(m->ev[1], st));
        m->ran[0] = m->timing;
    }
    if (!run_base && nd == 0) {
        SCANN_TRY(sync(m));
        fill_rows_empty(nq, k, out_idx, out_dist, out_count);
        return SCANN_HIP_OK;
    }
    // ---- stages 2 and 3 (skipped when the base rows ARE the answer: empty delta, identity ids, same pitch)
    const bool direct = run_base && nd == 0 && m->identity && kb == k;
    int s = SCANN_HIP_OK;
    if (direct) {
        s = download_rows(m, m->b_idx, m->b_dist, m->b_cnt, nq, k, out_idx, out_dist, out_count);
    } else {
        s = delta_and_merge(m, nq, q_stride, k, kb, run_base, filtered, user_bits);
        if (s == SCANN_HIP_OK) s = download_rows(m, m->o_idx, m->o_dist, m->o_cnt, nq, k, out_idx, out_dist, out_count);
    }
    if (s != SCANN_HIP_OK) {
        (void)hipStreamSynchronize(st);
        return s;
    }
    // ---- the one synchronisation, and the base's verdict on its enqueue-only pass
    if (!run_base) return sync(m);
    s = scann_hip_index_last_device_status(m->base, st);
    if (s != SCANN_HIP_ABORTED && s != SCANN_HIP_RESOURCE_EXHAUSTED) return s;
    // a sampled bound that missed or a candidate buffer that overflowed under the bitmap: the base's host entry point
    // answers the base pass (with its repeats), then stages 2 and 3 again
    std::vector<uint64_t> hb;
    scann_hip_search_opts oh = o;
    if (d_bitmap) {
        if (filtered) {
            hb.resize(base_words);
            SCANN_HIP_CHECK(hipMemcpy(hb.data(), m->comb.p, base_words * 8, hipMemcpyDeviceToHost));
        } else {
            hb = m->live;
        }
        oh.allow_bitmap = hb.data();
        oh.allow_bitmap_bits = m->n_base;
    }
    std::vector<uint32_t> hi((size_t)nq * kb), hc(nq);
    std::vector<float> hd((size_t)nq * kb);
    SCANN_TRY(scann_hip_search_batched(m->base, queries, nq, q_stride, q_dim, kb, &oh, hi.data(), hd.data(), hc.data()));
    SCANN_TRY(set_dev(m));
    SCANN_HIP_CHECK(hipMemcpyAsync(m->b_idx.p, hi.data(), hi.size() * 4, hipMemcpyHostToDevice, st));
    SCANN_HIP_CHECK(hipMemcpyAsync(m->b_dist.p, hd.data(), hd.size() * 4, hipMemcpyHostToDevice, st));
    SCANN_HIP_CHECK(hipMemcpyAsync(m->b_cnt.p, hc.data(), hc.size() * 4, hipMemcpyHostToDevice, st));
    s = delta_and_merge(m, nq, q_stride, k, kb, true, filtered, user_bits);
    if (s == SCANN_HIP_OK) s = download_rows(m, m->o_idx, m->o_dist, m->o_cnt, nq, k, out_idx, out_dist, out_count);
    const int s2 = sync(m);
    return s != SCANN_HIP_OK ? s : s2;
}

int scann_hip_mutable_export_live(scann_hip_mutable *m, float *out_rows, uint32_t *out_ids, uint64_t capacity_rows,
                                  uint64_t *out_n) {
    if (!m || !out_n) return fail(SCANN_HIP_INVALID_ARGUMENT, "null handle/out_n");
    std::lock_guard<std::mutex> lock(m->mu);
    const uint32_t nd = m->n_delta();
    const uint64_t n_live = m->live_base + nd;
    *out_n = n_live;
    if (capacity_rows < n_live) return fail(SCANN_HIP_RESOURCE_EXHAUSTED, "export_live: capacity_rows is below the live count");
    if (n_live == 0) return SCANN_HIP_OK;
    if (!out_rows || !out_ids) return fail(SCANN_HIP_INVALID_ARGUMENT, "null out_rows/out_ids");
    SCANN_TRY(set_dev(m));
    LiveOrder lo;
    plan_live_order(m, &lo, out_ids);
    const hipStream_t st = m->st;
    SCANN_TRY(m->x_out.ensure((size_t)n_live * m->stride * 4));
    SCANN_TRY(gather_prepare(m, lo));
    SCANN_TRY(gather_live_rows(m, m->x_out.as<float4>()));
    SCANN_HIP_CHECK(hipMemcpyAsync(out_rows, m->x_out.p, (size_t)n_live * m->stride * 4, hipMemcpyDeviceToHost, st));
    SCANN_TRY(sync(m));
    m->x_out.release();   // (as large as the index: not kept)
    return SCANN_HIP_OK;
}

int scann_hip_mutable_rebase(scann_hip_mutable *m, scann_hip_index *new_base, const uint32_t *base_ids, uint64_t n) {
    if (!m || !new_base) return fail(SCANN_HIP_INVALID_ARGUMENT, "null handle/new_base");
    std::lock_guard<std::mutex> lock(m->mu);
    return rebase_locked(m, new_base, base_ids, n);
}

int scann_hip_fold_mutable_stage_ms(scann_hip_mutable *m, float *out_ms5) {
    if (!m || !out_ms5) return fail(SCANN_HIP_INVALID_ARGUMENT, "null handle/out");
    std::lock_guard<std::mutex> lock(m->mu);
    for (int s = 0; s < 5; ++s) out_ms5[s] = m->fold_ms[s];
    return SCANN_HIP_OK;
}

int scann_hip_fold_mutable(scann_hip_mutable *m, scann_hip_index **out_new_base, uint32_t *out_base_ids,
                           uint64_t capacity_rows, uint64_t *out_n) {
    if (!m || !out_new_base || !out_n) return fail(SCANN_HIP_INVALID_ARGUMENT, "null handle/out_new_base/out_n");
    std::lock_guard<std::mutex> lock(m->mu);
    const uint32_t nd = m->n_delta();
    const uint64_t n_live = m->live_base + nd;
    *out_n = n_live;
    if (out_base_ids && capacity_rows < n_live)
        return fail(SCANN_HIP_RESOURCE_EXHAUSTED, "fold: capacity_rows is below the live count");
    if (n_live == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "Cannot build from empty dataset");
    FoldView fv;
    if (!m->bv.brute_force) {
        SCANN_TRY(index_fold_view(m->base, &fv));
        if (fv.n_local != fv.n_rows || fv.n_local != m->n_base)
            return fail(SCANN_HIP_FAILED_PRECONDITION, "fold: the base must index every row it stores (n_local == n_rows)");
    }
    SCANN_TRY(set_dev(m));
    const hipStream_t st = m->st;
    for (auto &e : m->fev)
        if (!e) SCANN_HIP_CHECK(hipEventCreate(&e));
    std::vector<uint32_t> ids(n_live);
    LiveOrder lo;
    plan_live_order(m, &lo, ids.data());
    DevBuf rows, codes, leaf_off, leaf_ids;   // the new index's arrays: freed here unless a handle takes them
    DevBuf tok, code8, order, dj, scratch;
    std::vector<uint32_t> off;
    const bool tree = !m->bv.brute_force;
    const uint32_t L = fv.L;
    FoldArgs a;
    // ---- every allocation and every copy from the host comes first: between two of the events below the stream holds
    // kernels only, so an event span is device time
    SCANN_TRY(rows.ensure((size_t)n_live * m->stride * 4));
    SCANN_TRY(gather_prepare(m, lo));
    if (tree) {
        SCANN_TRY(code8.ensure((size_t)std::max(nd, 1u) * fv.S));
        if (!fv.ah) SCANN_TRY(tok.ensure((size_t)std::max(nd, 1u) * 4));
        std::vector<uint32_t> djv(std::max(nd, 1u));
        for (uint32_t i = 0; i < nd; ++i) djv[i] = lo.dest[lo.order[i]];
        SCANN_TRY(upload(order, lo.order.data(), (size_t)nd * 4));
        SCANN_TRY(upload(dj, djv.data(), (size_t)nd * 4));
        SCANN_TRY(codes.ensure((size_t)n_live * fv.nw * 4));
        SCANN_TRY(leaf_off.ensure(((size_t)L + 1) * 4));
        if (!fv.ah) SCANN_TRY(leaf_ids.ensure((size_t)n_live * 4));
        const uint64_t chunks = ceil_div_u64(m->n_base, kMutFoldChunk);
        // scratch, every part a multiple of 8 bytes: sbits | cpref | sbase | doff | new_off | dtok | drank | dlist | flag
        auto r8 = [](uint64_t b) { return (b + 7) & ~7ull; };
        const uint64_t b_sbits = chunks * (kMutFoldChunk / 64) * 8, b_cpref = r8((chunks + 1) * 4), b_l = r8(((uint64_t)L + 2) * 4),
                       b_d = r8((uint64_t)std::max(nd, 1u) * 4);
        SCANN_TRY(scratch.ensure(b_sbits + b_cpref + 3 * b_l + 3 * b_d + 8));
        char *sp = scratch.as<char>();
        a.leaf_off = fv.leaf_off; a.leaf_ids = fv.leaf_ids; a.codes = fv.codes;
        a.L = L; a.nw = fv.nw; a.S = fv.S; a.bits = fv.K <= 16 ? 4u : 8u; a.n = m->n_base;
        a.live = m->d_live.as<uint64_t>(); a.live_prefix = m->x_prefix.as<uint32_t>();
        a.base_ids = m->identity ? nullptr : m->d_base_ids.as<uint32_t>();
        a.nd = nd; a.sorted_ids = m->x_sorted.as<uint32_t>(); a.order = order.as<uint32_t>(); a.dj = dj.as<uint32_t>();
        a.tok_slot = fv.ah ? nullptr : tok.as<uint32_t>(); a.code8 = code8.as<uint8_t>();
        a.sbits = reinterpret_cast<uint64_t *>(sp); sp += b_sbits;
        a.cpref = reinterpret_cast<uint32_t *>(sp); sp += b_cpref;
        a.sbase = reinterpret_cast<uint32_t *>(sp); sp += b_l;
        a.doff = reinterpret_cast<uint32_t *>(sp); sp += b_l;
        a.new_off = reinterpret_cast<uint32_t *>(sp); sp += b_l;
        a.dtok = reinterpret_cast<uint32_t *>(sp); sp += b_d;
        a.drank = reinterpret_cast<uint32_t *>(sp); sp += b_d;
        a.dlist = reinterpret_cast<uint32_t *>(sp); sp += b_d;
        a.flag = reinterpret_cast<uint32_t *>(sp);
        a.new_ids = fv.ah ? nullptr : leaf_ids.as<uint32_t>();
        a.new_codes = codes.as<uint32_t>();
        a.n_new = n_live;
        SCANN_TRY(fold_clear(a, st));
    }
    // ---- rows: export_live's kernels, writing to the new index's own buffer (they leave the bitmap's word prefix and
    // the sorted delta ids on the device for the passes below)
    SCANN_HIP_CHECK(hipEventRecord(m->fev[0], st));
    SCANN_TRY(gather_live_rows(m, rows.as<float4>()));
    SCANN_HIP_CHECK(hipEventRecord(m->fev[1], st));
    if (tree) {
        // ---- delta rows: leaf and code, by the partitioner's and the codebook's own kernels (delta slot order)
        if (nd) {
            if (!fv.ah) {
                BfIndexDev dv{};
                dv.rows = m->d_delta.as<float>();
                dv.n = nd;
                dv.dim = m->dim;
                dv.stride = m->stride;
                SCANN_TRY(bf_assign_nearest_device(dv, fv.centers, L, tok.as<uint32_t>(), nullptr, st));
            }
            const bool res = !fv.ah && fv.use_residuals;
            SCANN_TRY(launch_encode(fv.codebook, fv.S, fv.K, fv.dsub, m->d_delta.as<float>(), nd, m->stride,
                                    res ? fv.centers : nullptr, res ? tok.as<uint32_t>() : nullptr, code8.as<uint8_t>(), st));
        }
        SCANN_HIP_CHECK(hipEventRecord(m->fev[2], st));
        // ---- pass 1: counts, scans, new offsets
        SCANN_TRY(fold_count(a, st));
        SCANN_HIP_CHECK(hipEventRecord(m->fev[3], st));
        // ---- the offsets and the flag word come to the host (outside every span): the preconditions are decided
        // before anything is scattered
        off.resize((size_t)L + 2);
        SCANN_HIP_CHECK(hipMemcpyAsync(off.data(), a.new_off, off.size() * 4, hipMemcpyDeviceToHost, st));
        SCANN_HIP_CHECK(hipMemcpyAsync(leaf_off.p, a.new_off, ((size_t)L + 1) * 4, hipMemcpyDeviceToDevice, st));
        SCANN_TRY(sync(m));
        const uint32_t flag = off.back();
        off.pop_back();
        if (flag & 2u) return fail(SCANN_HIP_FAILED_PRECONDITION, "fold: the base holds a datapoint index outside its rows");
        if (flag & 1u)
            return fail(SCANN_HIP_FAILED_PRECONDITION, "fold: every leaf of the base must be strictly ascending in datapoint index");
        if (off[L] != n_live)
            return fail(SCANN_HIP_FAILED_PRECONDITION,
                        "fold: the leaves reach " + std::to_string(off[L] - nd) + " live rows, the live bitmap counts " +
                            std::to_string(m->live_base) + " (a datapoint in two leaves or in none)");
        // ---- pass 2: the stable scatter
        SCANN_HIP_CHECK(hipEventRecord(m->fev[4], st));
        SCANN_TRY(fold_scatter(a, st));
        SCANN_HIP_CHECK(hipEventRecord(m->fev[5], st));
    }
    SCANN_TRY(sync(m));
    const auto t_finish = std::chrono::steady_clock::now();
    // ---- the second half of the create functions, on the new arrays
    scann_hip_index *nb = nullptr;
    if (m->bv.brute_force) SCANN_TRY(index_fold_bf(m->base, rows, n_live, m->stride, &nb));
    else SCANN_TRY(index_fold_txh(m->base, rows, codes, leaf_off, leaf_ids, off, n_live, m->stride, &nb));
    // ---- the swap (ids that are 0 .. n' - 1 are the identity)
    const bool identity = ids.back() == n_live - 1;
    int s = set_dev(m);
    if (s == SCANN_HIP_OK) s = rebase_locked(m, nb, identity ? nullptr : ids.data(), n_live);
    if (s != SCANN_HIP_OK) {
        scann_hip_index_destroy(nb);
        return s;
    }
    // (a brute-force base has no middle stages: their events were not recorded)
    static const int span[4][2] = {{0, 1}, {1, 2}, {2, 3}, {4, 5}};
    for (int e = 0; e < 4; ++e) {
        m->fold_ms[e] = 0.0f;
        if (e == 0 || tree) (void)hipEventElapsedTime(&m->fold_ms[e], m->fev[span[e][0]], m->fev[span[e][1]]);
    }
    m->fold_ms[4] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_finish).count();
    if (out_base_ids) std::memcpy(out_base_ids, ids.data(), (size_t)n_live * 4);
    *out_new_base = nb;
    return SCANN_HIP_OK;
}

}  // extern "C"

// tokens.hip -- tag filters: a device-resident token map that writes per-query allow-bitmaps, and the word-wise
// combination of such blocks.  Callers of a filtered batch hold tags (a tenant, a category, an ACL group), not row
// ids.  RestrictTokenMap (restricts/allowlist.rs:184-244) keeps token -> datapoint indices; create_allowlist(tokens)
// allows a datapoint that carries at least one of the tokens.  Here the map is built once (pairs sorted by (token,
// index) on the host, duplicates and out-of-range indices dropped: a bitmap is a set union, RestrictAllowlist::add
// ignores an index at or past the capacity) and lives on the device as three arrays: the distinct tokens ascending, a
// CSR of offsets, the concatenated ascending postings.  A batch then sends a few tokens per query.
//
// token_bitmap_kernel: workgroup (t, y) owns tile t (SCANN_HIP_TOKEN_TILE_BITS bits, 8 KB of LDS: eight workgroups of
// 256 threads share a CU) of the bitmaps of queries y, y + gridDim.y, ...  Per query: zero the LDS tile; in chunks of
// up to 256 tokens, g lanes per token (64 while few tokens are left, 1 from 256 on) find the token (a g-ary search
// over the token array) and the part of its posting inside the tile (two lower bounds: the postings ascend), a block
// scan lays those parts end to end, and the threads walk
// the concatenation one id each, OR-ing bits into the tile with LDS atomics; barrier; the tile goes to global memory
// once, 16 bytes a lane, plain stores (the lines stay in L2 for the search that reads them next).  The last tile of
// a query also writes the zero gap words up to the stride.  No clear, no global atomic, no id traffic from the host;
// the last word needs no mask since postings are in range by construction.
#include <algorithm>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "allow.h"
#include "comm.h"   // ctx_device
#include "launch.h"
#include "tokens.h"

namespace scann {

namespace {

constexpr uint32_t kTokThreads = kBitmapThreads;

// ---- host form of the map: the model of the device arrays, and what get_indices reads ---------------------------
struct TokenCsr {
    std::vector<uint64_t> tokens;    // distinct, ascending (a token whose every index was out of range stays, empty)
    std::vector<uint64_t> offsets;   // tokens.size() + 1
    std::vector<uint32_t> postings;  // per token ascending, deduplicated, < num_datapoints
};

void build_csr(uint64_t n, const uint32_t *indices, const uint64_t *tokens, uint64_t n_pairs, TokenCsr *out) {
    std::vector<std::pair<uint64_t, uint32_t>> pairs(n_pairs);
    for (uint64_t i = 0; i < n_pairs; ++i) pairs[i] = {tokens[i], indices[i]};
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    out->tokens.clear();
    out->offsets.clear();
    out->postings.clear();
    for (const auto &p : pairs) {
        if (out->tokens.empty() || out->tokens.back() != p.first) {
            out->tokens.push_back(p.first);
            out->offsets.push_back(out->postings.size());
        }
        if (p.second < n) out->postings.push_back(p.second);
    }
    out->offsets.push_back(out->postings.size());
}

// position of `token` in the ascending array, or ntok
uint64_t find_token_host(const TokenCsr &m, uint64_t token) {
    const auto it = std::lower_bound(m.tokens.begin(), m.tokens.end(), token);
    return it != m.tokens.end() && *it == token ? (uint64_t)(it - m.tokens.begin()) : (uint64_t)m.tokens.size();
}

void csr_bitmaps_host(const TokenCsr &m, const uint64_t *q_tokens, const uint64_t *q_offsets, uint32_t nq, uint64_t stride,
                      uint64_t *out) {
    for (uint64_t i = 0; i < (uint64_t)nq * stride; ++i) out[i] = 0;
    for (uint32_t q = 0; q < nq; ++q) {
        uint64_t *row = out + (size_t)q * stride;
        for (uint64_t e = q_offsets[q]; e < q_offsets[q + 1]; ++e) {
            const uint64_t t = find_token_host(m, q_tokens[e]);
            if (t == m.tokens.size()) continue;
            for (uint64_t p = m.offsets[t]; p < m.offsets[t + 1]; ++p) {
                const uint32_t id = m.postings[p];
                row[id >> 6] |= 1ull << (id & 63u);
            }
        }
    }
}

int check_host_lists(const uint64_t *q_tokens, const uint64_t *q_offsets, uint32_t nq) {
    if (!q_offsets) return fail(SCANN_HIP_INVALID_ARGUMENT, "null offsets pointer");
    for (uint32_t q = 0; q < nq; ++q)
        if (q_offsets[q + 1] < q_offsets[q]) return fail(SCANN_HIP_INVALID_ARGUMENT, "offsets must ascend");
    if (q_offsets[nq] > q_offsets[0] && !q_tokens) return fail(SCANN_HIP_INVALID_ARGUMENT, "tokens is null");
    return SCANN_HIP_OK;
}

// ---- device ----------------------------------------------------------------------------------------------------
// First i in [lo, hi) with a[i] >= v, else hi, found by the g lanes of a group together: g a power of two <= 64, the
// group's lanes contiguous in one wave and all here with the same lo / hi / v; sub = the lane's place in its group,
// gshift = the group's first lane.  A step probes g points lo + len * k / g (k = sub), all inside the range; the
// number of probes below v picks the part to go on with, 1 / g of the range: one dependent load per step, three for
// a posting of 100 k ids at g = 64 where a binary search takes seventeen.  g = 1 is the binary search.
template <typename T>
__device__ __forceinline__ uint64_t group_lower_bound(const T *__restrict__ a, uint64_t lo, uint64_t hi, uint64_t v, uint32_t g,
                                                      uint32_t sub, uint32_t gshift) {
    if (g == 1) {
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            if ((uint64_t)a[mid] < v) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    }
    const uint32_t lg = 31u - (uint32_t)__clz((int)g);
    const unsigned long long gmask = (g == 64 ? ~0ull : (1ull << g) - 1ull) << gshift;
    while (lo < hi) {
        const uint64_t len = hi - lo;   // (< 2^33: len * g fits 64 bits)
        const bool less = (uint64_t)a[lo + ((len * sub) >> lg)] < v;
        const uint32_t c = (uint32_t)__popcll(__ballot(less) & gmask);   // probes 0 .. c - 1 are below v (a ascends)
        if (c == 0) break;                                               // a[lo] >= v
        const uint64_t nlo = lo + ((len * (c - 1)) >> lg) + 1;
        if (c < g) hi = lo + ((len * c) >> lg);
        lo = nlo;
    }
    return lo;
}

__global__ __launch_bounds__(kTokThreads) void token_bitmap_kernel(
    const uint64_t *__restrict__ map_tokens, uint64_t ntok, const uint64_t *__restrict__ map_offsets,
    const uint32_t *__restrict__ postings, const uint64_t *__restrict__ q_tokens, const uint64_t *__restrict__ q_offsets,
    uint32_t nq, uint64_t bits, uint64_t words, uint64_t stride, uint64_t *__restrict__ out) {
    __shared__ uint64_t tile[kTokenTileWords];
    __shared__ uint64_t s_start[kTokThreads];   // first posting position of a token inside this tile
    __shared__ uint32_t s_cnt[kTokThreads];     // ids of a token inside this tile
    __shared__ uint32_t s_end[kTokThreads];     // running end of the tokens' parts laid end to end
    __shared__ uint32_t s_wave[kTokThreads / 64];
    uint32_t *tile32 = reinterpret_cast<uint32_t *>(tile);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t t = blockIdx.x;
    const uint64_t lo_bit = t * SCANN_HIP_TOKEN_TILE_BITS, hi_bit = min(lo_bit + SCANN_HIP_TOKEN_TILE_BITS, bits);
    const uint64_t w0 = min(t * kTokenTileWords, words), w1 = min(w0 + kTokenTileWords, words);
    const uint32_t tile_words = (uint32_t)(w1 - w0);
    const bool last_tile = t + 1 == gridDim.x;
    for (uint32_t q = blockIdx.y; q < nq; q += gridDim.y) {
        for (uint32_t i = tid; i < tile_words; i += kTokThreads) tile[i] = 0;
        __syncthreads();
        const uint64_t e0 = q_offsets[q], e1 = q_offsets[q + 1];
        for (uint64_t c = e0; c < e1 && tile_words;) {
            // 1. g lanes per token -- a whole wave while at most four tokens are left, one lane from 256 tokens on --
            //    find the token and its posting's part inside [lo_bit, hi_bit): the searches are chains of dependent
            //    loads, and g lanes make each chain log_g long instead of log_2
            uint32_t g = 64;
            while (g > 1 && (uint64_t)(kTokThreads / g) < e1 - c) g >>= 1;
            const uint32_t sub = tid & (g - 1u), gshift = lane - sub;
            const uint64_t mine = c + tid / g;
            c += kTokThreads / g;
            uint64_t start = 0;
            uint32_t cnt = 0;
            if (mine < e1) {
                const uint64_t tok = q_tokens[mine];
                const uint64_t a = group_lower_bound(map_tokens, 0, ntok, tok, g, sub, gshift);
                if (a < ntok && map_tokens[a] == tok) {
                    const uint64_t p0 = map_offsets[a], p1 = map_offsets[a + 1];
                    start = group_lower_bound(postings, p0, p1, lo_bit, g, sub, gshift);
                    // (distinct ids inside one tile: at most SCANN_HIP_TOKEN_TILE_BITS of them, 2^24 per chunk)
                    const uint64_t stop = min(p1, start + SCANN_HIP_TOKEN_TILE_BITS);
                    cnt = (uint32_t)(group_lower_bound(postings, start, stop, hi_bit, g, sub, gshift) - start);
                }
            }
            // 2. the groups' first lanes put their token in slot tid / g (a slot for each of the 256 / g groups, a
            //    token or not); inclusive scan of the slots' counts over the block, the slots past them counting 0
            if (sub == 0) {
                s_cnt[tid / g] = cnt;
                s_start[tid / g] = start;
            }
            __syncthreads();
            uint32_t incl = tid < kTokThreads / g ? s_cnt[tid] : 0u;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
                if ((int)lane >= o) incl += up;
            }
            if (lane == 63) s_wave[wave] = incl;
            __syncthreads();
            uint32_t base = 0, total = 0;
#pragma unroll
            for (uint32_t w = 0; w < kTokThreads / 64; ++w) {
                const uint32_t s = s_wave[w];
                base += w < wave ? s : 0u;
                total += s;
            }
            s_end[tid] = incl + base;
            __syncthreads();
            // 3. one id per thread and step over the concatenated parts; a thread's positions ascend, so its token
            //    index only moves forward.  Four loads are in flight before the first atomic.
            constexpr uint32_t kUnroll = 4;
            uint32_t j = 0, beg = 0, end = s_end[0];
            for (uint32_t w = tid; w < total; w += kUnroll * kTokThreads) {
                uint32_t id[kUnroll];
#pragma unroll
                for (uint32_t u = 0; u < kUnroll; ++u) {
                    const uint32_t wu = w + u * kTokThreads;
                    if (wu < total) {
                        while (wu >= end) {   // (wu < total = s_end[255]: j stays below 256)
                            beg = end;
                            end = s_end[++j];
                        }
                        id[u] = postings[s_start[j] + (wu - beg)];
                    }
                }
#pragma unroll
                for (uint32_t u = 0; u < kUnroll; ++u)
                    if (w + u * kTokThreads < total) {
                        const uint32_t rel = (uint32_t)(id[u] - lo_bit);   // < tile bits
                        atomicOr(&tile32[rel >> 5], 1u << (rel & 31u));
                    }
            }
            __syncthreads();   // the next chunk rewrites s_wave / s_start / s_end
        }
        __syncthreads();
        uint64_t *row = out + (size_t)q * stride;
        store_words(row + w0, tile, tile_words);
        if (last_tile) store_words(row + words, nullptr, stride - words);
        __syncthreads();   // the next query zeroes the tile
    }
}

// words [0, words) of every query's row; VEC: two words (16 bytes) a lane, every row 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(kTokThreads) void allow_combine_kernel(int op, const uint64_t *a, uint64_t stride_a,
                                                                    const uint64_t *b, uint64_t stride_b, uint32_t nq,
                                                                    uint64_t words, uint64_t last_mask, uint64_t *out,
                                                                    uint64_t stride_out) {
    // (out may be a or b: a lane reads its own words before it writes them, and no other lane touches them)
    const uint64_t first = (uint64_t)blockIdx.x * kTokThreads + threadIdx.x, step = (uint64_t)gridDim.x * kTokThreads;
    for (uint32_t q = blockIdx.y; q < nq; q += gridDim.y) {
        const uint64_t *ra = a + (size_t)q * stride_a;
        const uint64_t *rb = b ? b + (size_t)q * stride_b : nullptr;
        uint64_t *ro = out + (size_t)q * stride_out;
        if constexpr (VEC) {
            const uint64_t pairs = words >> 1;
            for (uint64_t p = first; p < pairs; p += step) {
                const ulonglong2 x = reinterpret_cast<const ulonglong2 *>(ra)[p];
                ulonglong2 y = make_ulonglong2(0ull, 0ull);
                if (rb) y = reinterpret_cast<const ulonglong2 *>(rb)[p];
                ulonglong2 r = make_ulonglong2(allow_combine_word(op, x.x, y.x), allow_combine_word(op, x.y, y.y));
                if (2 * p + 2 == words) r.y &= last_mask;
                reinterpret_cast<ulonglong2 *>(ro)[p] = r;
            }
            if ((words & 1ull) && first == 0)
                ro[words - 1] = allow_combine_word(op, ra[words - 1], rb ? rb[words - 1] : 0ull) & last_mask;
        } else {
            for (uint64_t w = first; w < words; w += step) {
                uint64_t r = allow_combine_word(op, ra[w], rb ? rb[w] : 0ull);
                if (w + 1 == words) r &= last_mask;
                ro[w] = r;
            }
        }
    }
}

uint64_t last_word_mask(uint64_t bits) { return bits & 63u ? (1ull << (bits & 63u)) - 1 : ~0ull; }

int check_combine_args(int op, const void *a, uint64_t stride_a, const void *b, uint64_t stride_b, uint32_t nq, uint64_t bits,
                       const void *out, uint64_t stride_out) {
    if (op < SCANN_HIP_ALLOW_AND || op > SCANN_HIP_ALLOW_NOT) return fail(SCANN_HIP_INVALID_ARGUMENT, "unknown combine op");
    const uint64_t words = allow_words(bits);
    const bool two = op != SCANN_HIP_ALLOW_NOT;
    if ((stride_a && stride_a < words) || (two && stride_b && stride_b < words) || stride_out < words)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "a stride is smaller than one bitmap (ceil(bits / 64) words)");
    if (nq && words && (!a || (two && !b) || !out)) return fail(SCANN_HIP_INVALID_ARGUMENT, "null operand/output pointer");
    return SCANN_HIP_OK;
}

}  // namespace

int token_bitmaps_launch(const uint64_t *d_map_tokens, uint64_t ntok, const uint64_t *d_map_offsets, const uint32_t *d_postings,
                         const uint64_t *d_q_tokens, const uint64_t *d_q_offsets, uint32_t nq, uint64_t bits, uint64_t stride,
                         uint64_t *d_out, hipStream_t st) {
    if (nq == 0 || stride == 0) return SCANN_HIP_OK;
    // (bits = 0: one tile of no words, which owns the gap)
    const uint64_t tiles = std::max<uint64_t>(1, ceil_div_u64(bits, SCANN_HIP_TOKEN_TILE_BITS));
    // queries beyond the grid's y extent are looped over; very long bitmaps take fewer rows of workgroups
    const uint32_t gy = (uint32_t)std::min<uint64_t>(std::min<uint32_t>(nq, 65535u), std::max<uint64_t>(1, (1ull << 22) / tiles));
    return launch(token_bitmap_kernel, dim3((uint32_t)tiles, gy), dim3(kTokThreads), 0, st, d_map_tokens, ntok, d_map_offsets,
                  d_postings, d_q_tokens, d_q_offsets, nq, bits, allow_words(bits), stride, d_out);
}

int allow_combine_launch(int op, const uint64_t *d_a, uint64_t stride_a, const uint64_t *d_b, uint64_t stride_b, uint32_t nq,
                         uint64_t bits, uint64_t *d_out, uint64_t stride_out, hipStream_t st) {
    const uint64_t words = allow_words(bits);
    if (nq == 0 || words == 0) return SCANN_HIP_OK;
    if (op == SCANN_HIP_ALLOW_NOT) d_b = nullptr, stride_b = 0;
    const bool vec = (((uint64_t)d_a | (uint64_t)d_b | (uint64_t)d_out) & 15ull) == 0 && ((stride_a | stride_b | stride_out) & 1ull) == 0;
    const uint64_t items = vec ? std::max<uint64_t>(words >> 1, 1) : words;
    const uint32_t gy = std::min<uint32_t>(nq, 65535u);
    const uint32_t gx = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(ceil_div_u64(items, kTokThreads),
                                                                          std::max<uint32_t>(1u, (uint32_t)num_cus() * 8u / gy)));
    const uint64_t mask = last_word_mask(bits);
    if (vec)
        return launch(allow_combine_kernel<true>, dim3(gx, gy), dim3(kTokThreads), 0, st, op, d_a, stride_a, d_b, stride_b, nq,
                      words, mask, d_out, stride_out);
    return launch(allow_combine_kernel<false>, dim3(gx, gy), dim3(kTokThreads), 0, st, op, d_a, stride_a, d_b, stride_b, nq,
                  words, mask, d_out, stride_out);
}

}  // namespace scann

using namespace scann;

struct scann_hip_token_map {
    int device = 0;
    uint64_t n = 0;
    TokenCsr host;                        // get_indices / num_tokens read this copy: no device round trip
    DevBuf d_tokens, d_offsets, d_postings;
    // the host-pointer forms: one stream and grow-only staging buffers, one call at a time
    std::mutex mu;
    hipStream_t stream = nullptr;
    DevBuf s_tokens, s_offsets;
    FilterSearchBufs fs;   // fs.block: the block of the host-pointer forms
    ~scann_hip_token_map() {
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

// the host-pointer form under m->mu: lists up, one kernel, the block left in m->fs.block (no copy back, no synchronise)
int stage_block(scann_hip_token_map *m, const uint64_t *q_tokens, const uint64_t *q_offsets, uint32_t nq, uint64_t stride) {
    const uint64_t nt = q_offsets[nq] - q_offsets[0];
    SCANN_TRY(m->s_tokens.ensure(nt * 8));
    SCANN_TRY(m->s_offsets.ensure(((size_t)nq + 1) * 8));
    SCANN_TRY(m->fs.block.ensure((size_t)nq * stride * 8));
    if (nt) SCANN_HIP_CHECK(hipMemcpyAsync(m->s_tokens.p, q_tokens + q_offsets[0], nt * 8, hipMemcpyHostToDevice, m->stream));
    std::vector<uint64_t> rel((size_t)nq + 1);   // offsets relative to the first token sent
    for (uint32_t q = 0; q <= nq; ++q) rel[q] = q_offsets[q] - q_offsets[0];
    SCANN_HIP_CHECK(hipMemcpyAsync(m->s_offsets.p, rel.data(), rel.size() * 8, hipMemcpyHostToDevice, m->stream));
    SCANN_HIP_CHECK(hipStreamSynchronize(m->stream));   // rel leaves scope; pageable copies may still be in flight
    return token_bitmaps_launch(m->d_tokens.as<uint64_t>(), m->host.tokens.size(), m->d_offsets.as<uint64_t>(),
                                m->d_postings.as<uint32_t>(), m->s_tokens.as<uint64_t>(), m->s_offsets.as<uint64_t>(), nq,
                                m->n, stride, m->fs.block.as<uint64_t>(), m->stream);
}

}  // namespace

extern "C" {

int scann_hip_token_map_create(scann_hip_ctx *ctx, uint64_t num_datapoints, const uint32_t *indices, const uint64_t *tokens,
                               uint64_t n_pairs, scann_hip_token_map **out) {
    if (!out) return fail(SCANN_HIP_INVALID_ARGUMENT, "out is null");
    *out = nullptr;
    if (!ctx) return fail(SCANN_HIP_INVALID_ARGUMENT, "context is null");
    if (num_datapoints >= 0xFFFFFFFFull) return fail(SCANN_HIP_OUT_OF_RANGE, "num_datapoints must be below 2^32 - 1");
    if (n_pairs && (!indices || !tokens)) return fail(SCANN_HIP_INVALID_ARGUMENT, "null indices/tokens with n_pairs > 0");
    std::unique_ptr<scann_hip_token_map> m(new scann_hip_token_map());
    m->device = ctx_device(ctx);
    m->n = num_datapoints;
    build_csr(num_datapoints, indices, tokens, n_pairs, &m->host);
    SCANN_HIP_CHECK(hipSetDevice(m->device));
    SCANN_TRY(upload(m->d_tokens, m->host.tokens.data(), m->host.tokens.size() * 8));
    SCANN_TRY(upload(m->d_offsets, m->host.offsets.data(), m->host.offsets.size() * 8));
    SCANN_TRY(upload(m->d_postings, m->host.postings.data(), m->host.postings.size() * 4));
    SCANN_HIP_CHECK(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
    *out = m.release();
    return SCANN_HIP_OK;
}

void scann_hip_token_map_destroy(scann_hip_token_map *m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    delete m;
}

uint64_t scann_hip_token_map_num_tokens(const scann_hip_token_map *m) { return m ? m->host.tokens.size() : 0; }

uint64_t scann_hip_token_map_num_datapoints(const scann_hip_token_map *m) { return m ? m->n : 0; }

int scann_hip_token_map_get_indices(const scann_hip_token_map *m, uint64_t token, uint32_t *out, uint64_t capacity,
                                    uint64_t *out_n) {
    if (!m || !out_n) return fail(SCANN_HIP_INVALID_ARGUMENT, "null map/out_n pointer");
    const uint64_t t = find_token_host(m->host, token);
    const uint64_t cnt = t == m->host.tokens.size() ? 0 : m->host.offsets[t + 1] - m->host.offsets[t];
    *out_n = cnt;
    if (cnt == 0) return SCANN_HIP_OK;
    if (capacity < cnt) return fail(SCANN_HIP_RESOURCE_EXHAUSTED, "the posting is longer than the output's capacity");
    if (!out) return fail(SCANN_HIP_INVALID_ARGUMENT, "out is null");
    std::copy(m->host.postings.begin() + m->host.offsets[t], m->host.postings.begin() + m->host.offsets[t + 1], out);
    return SCANN_HIP_OK;
}

int scann_hip_token_map_allow_bitmaps_device(const scann_hip_token_map *m, const uint64_t *d_tokens, const uint64_t *d_offsets,
                                             uint32_t nq, uint64_t stride_words, uint64_t *d_out_words, void *hip_stream) {
    if (!m) return fail(SCANN_HIP_INVALID_ARGUMENT, "token map is null");
    SCANN_TRY(check_block_args(m->n, stride_words));
    if (nq == 0) return SCANN_HIP_OK;
    // (d_tokens may be null when every list is empty: the kernel reads no token then)
    if (!d_offsets || (stride_words && !d_out_words)) return fail(SCANN_HIP_INVALID_ARGUMENT, "null offsets/output pointer");
    SCANN_HIP_CHECK(hipSetDevice(m->device));
    return token_bitmaps_launch(m->d_tokens.as<uint64_t>(), m->host.tokens.size(), m->d_offsets.as<uint64_t>(),
                                m->d_postings.as<uint32_t>(), d_tokens, d_offsets, nq, m->n, stride_words, d_out_words,
                                static_cast<hipStream_t>(hip_stream));
}

int scann_hip_token_map_allow_bitmaps(scann_hip_token_map *m, const uint64_t *tokens, const uint64_t *offsets, uint32_t nq,
                                      uint64_t stride_words, uint64_t *out_words) {
    if (!m) return fail(SCANN_HIP_INVALID_ARGUMENT, "token map is null");
    SCANN_TRY(check_block_args(m->n, stride_words));
    if (nq == 0) return SCANN_HIP_OK;
    SCANN_TRY(check_host_lists(tokens, offsets, nq));
    if (stride_words == 0) return SCANN_HIP_OK;
    if (!out_words) return fail(SCANN_HIP_INVALID_ARGUMENT, "null output pointer");
    std::lock_guard<std::mutex> lock(m->mu);
    SCANN_HIP_CHECK(hipSetDevice(m->device));
    SCANN_TRY(stage_block(m, tokens, offsets, nq, stride_words));
    SCANN_HIP_CHECK(hipMemcpyAsync(out_words, m->fs.block.p, (size_t)nq * stride_words * 8, hipMemcpyDeviceToHost, m->stream));
    SCANN_HIP_CHECK(hipStreamSynchronize(m->stream));
    return SCANN_HIP_OK;
}

int scann_hip_allow_bitmaps_from_tokens(const uint32_t *indices, const uint64_t *tokens, uint64_t n_pairs,
                                        uint64_t num_datapoints, const uint64_t *q_tokens, const uint64_t *q_offsets,
                                        uint32_t nq, uint64_t stride_words, uint64_t *out_words) {
    if (num_datapoints >= 0xFFFFFFFFull) return fail(SCANN_HIP_OUT_OF_RANGE, "num_datapoints must be below 2^32 - 1");
    if (n_pairs && (!indices || !tokens)) return fail(SCANN_HIP_INVALID_ARGUMENT, "null indices/tokens with n_pairs > 0");
    SCANN_TRY(check_block_args(num_datapoints, stride_words));
    if (nq == 0) return SCANN_HIP_OK;
    SCANN_TRY(check_host_lists(q_tokens, q_offsets, nq));
    if (stride_words == 0) return SCANN_HIP_OK;
    if (!out_words) return fail(SCANN_HIP_INVALID_ARGUMENT, "null output pointer");
    TokenCsr csr;
    build_csr(num_datapoints, indices, tokens, n_pairs, &csr);
    csr_bitmaps_host(csr, q_tokens, q_offsets, nq, stride_words, out_words);
    return SCANN_HIP_OK;
}

int scann_hip_search_batched_tokens(scann_hip_index *index, scann_hip_token_map *m, const float *queries, uint32_t nq,
                                    uint32_t q_stride, uint32_t q_dim, uint32_t k, const scann_hip_search_opts *opts,
                                    const uint64_t *q_tokens, const uint64_t *q_offsets, uint32_t *out_idx, float *out_dist,
                                    uint32_t *out_count) {
    if (!index || !m) return fail(SCANN_HIP_INVALID_ARGUMENT, "null index/token map");
    if (nq == 0) return SCANN_HIP_OK;
    SCANN_TRY(filter_search_check(index, queries, q_stride, q_dim, k, opts, out_idx, out_dist, out_count, "the token lists"));
    SCANN_TRY(check_host_lists(q_tokens, q_offsets, nq));
    const uint64_t stride = std::max<uint64_t>(allow_words(m->n), 1);   // (a stride of 0 would mean one shared bitmap)
    scann_hip_search_opts o;
    if (opts) o = *opts;
    else scann_hip_search_opts_default(&o);
    std::lock_guard<std::mutex> lock(m->mu);
    SCANN_HIP_CHECK(hipSetDevice(m->device));
    SCANN_TRY(filter_search_begin(m->fs, m->stream, queries, nq, q_stride, k));
    // the block is built and read on one stream, with nothing between the two enqueues
    SCANN_TRY(stage_block(m, q_tokens, q_offsets, nq, stride));
    return filter_search_finish(index, m->fs, m->stream, queries, nq, q_stride, q_dim, k, o, m->n, stride, out_idx, out_dist,
                                out_count);
}

int scann_hip_allow_bitmaps_combine(int op, const uint64_t *a, uint64_t stride_a, const uint64_t *b, uint64_t stride_b,
                                    uint32_t nq, uint64_t bits, uint64_t *out, uint64_t stride_out) {
    SCANN_TRY(check_combine_args(op, a, stride_a, b, stride_b, nq, bits, out, stride_out));
    const uint64_t words = allow_words(bits), mask = last_word_mask(bits);
    const bool two = op != SCANN_HIP_ALLOW_NOT;
    for (uint32_t q = 0; q < nq; ++q)
        for (uint64_t w = 0; w < words; ++w) {
            uint64_t r = allow_combine_word(op, a[(size_t)q * stride_a + w], two ? b[(size_t)q * stride_b + w] : 0ull);
            if (w + 1 == words) r &= mask;
            out[(size_t)q * stride_out + w] = r;
        }
    return SCANN_HIP_OK;
}

int scann_hip_allow_bitmaps_combine_device(scann_hip_ctx *ctx, int op, const uint64_t *d_a, uint64_t stride_a,
                                           const uint64_t *d_b, uint64_t stride_b, uint32_t nq, uint64_t bits, uint64_t *d_out,
                                           uint64_t stride_out, void *hip_stream) {
    if (!ctx) return fail(SCANN_HIP_INVALID_ARGUMENT, "context is null");
    SCANN_TRY(check_combine_args(op, d_a, stride_a, d_b, stride_b, nq, bits, d_out, stride_out));
    SCANN_HIP_CHECK(hipSetDevice(ctx_device(ctx)));
    return allow_combine_launch(op, d_a, stride_a, d_b, stride_b, nq, bits, d_out, stride_out, static_cast<hipStream_t>(hip_stream));
}

}  // extern "C"

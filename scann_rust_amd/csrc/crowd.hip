// crowd.hip -- the crowding stage behind every search: CrowdingConstraint::apply (restricts/crowding.rs:81-104)
// over the [nq][depth] rows a search with k = depth left in the workspace.
//
// The rule: walk the row in order, keep entry i iff fewer than `limit` EARLIER entries of the row carry the same
// attribute, stop at k kept.  (The reference counts earlier KEPT entries; for one attribute dimension the two
// coincide: an attribute's first `limit` entries are all kept, and once one is rejected every later one is too.)
// "Earlier entries with my attribute" needs no accept decision of anybody else, so a wave decides 64 entries at once.
//
// One wave per query.  The row is walked in chunks of 64 entries; per chunk
//   1. gather attr[idx] (8-byte loads; idx >= n_attrs -> 0, crowding.rs:90); the next chunk's loads are issued
//      before this chunk is processed, so that the two dependent global latencies overlap the table work;
//   2. group the lanes by equal attribute: the first unresolved lane broadcasts its attribute, a ballot of the equal
//      lanes gives every member its rank inside the chunk and the group's size (one round per DISTINCT attribute);
//   3. each group's first lane looks its attribute up in an open-addressed LDS table (linear probing, keyed on the
//      full 64 bits: a hash collision costs probes, never a wrong count) and reads the count of earlier chunks;
//   4. after a barrier the same lanes add the group's size, or claim an empty slot (compare-and-swap on the count
//      word: two new attributes of one chunk may hash to the same slot);
//   5. keep = earlier count + rank < limit; a prefix sum of the keep ballot places the survivors.
// The loop ends once k entries are kept: at small k with plenty of distinct attributes it reads one or two chunks.
//
// Table: slots(depth) = clamp(next_pow2(2 depth), 128, 12288) entries of {u64 key, u32 count}; count 0 = empty (an
// inserted key has count >= 1, so attribute values 0 and 2^64-1 need no reserved marker).  At most `depth` distinct
// keys are ever inserted and slots > depth, so a probe always meets its key or an empty slot.  Slot of a key =
// mulhi32(high word of the splitmix64 finaliser, slots): any slot count, no modulo.
#include <algorithm>
#include <cmath>
#include <string>

#include "crowd.h"
#include "launch.h"

namespace scann {

uint32_t crowd_table_slots(uint32_t depth) {
    const uint64_t want = 2ull * std::max(depth, 1u);
    uint32_t s = kCrowdMinSlots;
    while (s < want && s < kCrowdMaxSlots) s <<= 1;
    return std::min(s, kCrowdMaxSlots);
}

namespace {

constexpr uint32_t kCrowdInvalid = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t crowd_slot_of(uint64_t key, uint32_t slots) {
    uint64_t z = key + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return __umulhi((uint32_t)(z >> 32), slots);
}

// multi-attribute table: the dimension takes part in the home slot
__device__ __forceinline__ uint32_t crowd_md_slot_of(uint64_t key, uint32_t dim, uint32_t slots) {
    return crowd_slot_of(key ^ ((uint64_t)(dim + 1u) * 0xD6E8FEB86659FD93ull), slots);
}

__global__ __launch_bounds__(64) void crowd_kernel(const uint32_t *__restrict__ rows_idx,
                                                   const float *__restrict__ rows_dist,
                                                   const uint32_t *__restrict__ rows_cnt, uint32_t depth,
                                                   const uint64_t *__restrict__ attrs, uint64_t n_attrs, uint32_t k,
                                                   uint32_t limit, uint32_t slots, uint32_t *__restrict__ out_idx,
                                                   float *__restrict__ out_dist, uint32_t *__restrict__ out_cnt) {
    extern __shared__ uint64_t s_key[];                              // [slots]
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_key + slots);   // [slots]
    const uint32_t q = blockIdx.x, lane = threadIdx.x;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    const uint32_t *ri = rows_idx + (size_t)q * depth;
    const float *rd = rows_dist + (size_t)q * depth;
    uint32_t *oi = out_idx + (size_t)q * k;
    float *od = out_dist + (size_t)q * k;
    const uint32_t cnt = min(rows_cnt[q], depth);   // a short row is walked to its count: no sentinel is looked up

    for (uint32_t s = lane; s < slots; s += 64) s_cnt[s] = 0;
    __syncthreads();

    uint32_t kept = 0;
    // chunk 0's loads
    uint32_t n_idx = kCrowdInvalid;
    float n_dist = INFINITY;
    uint64_t n_attr = 0;
    if (limit > 0 && lane < cnt) {
        n_idx = ri[lane];
        n_dist = rd[lane];
        n_attr = (uint64_t)n_idx < n_attrs ? attrs[n_idx] : 0ull;
    }
    for (uint32_t base = 0; limit > 0 && base < cnt && kept < k; base += 64) {
        const uint32_t i = base + lane;
        const bool valid = i < cnt;
        const uint32_t idx = n_idx;
        const float dist = n_dist;
        const uint64_t attr = n_attr;
        if (i + 64 < cnt) {   // next chunk
            n_idx = ri[i + 64];
            n_dist = rd[i + 64];
            n_attr = (uint64_t)n_idx < n_attrs ? attrs[n_idx] : 0ull;
        }
        // 2. groups of equal attributes
        const uint32_t a_lo = (uint32_t)attr, a_hi = (uint32_t)(attr >> 32);
        uint64_t pending = __ballot(valid);
        uint32_t rank = 0, gsize = 0, gleader = lane;
        while (pending) {
            const int l = __ffsll((unsigned long long)pending) - 1;
            const uint32_t b_lo = __shfl(a_lo, l), b_hi = __shfl(a_hi, l);
            const bool mine = valid && a_lo == b_lo && a_hi == b_hi;
            const uint64_t match = __ballot(mine);
            if (mine) {
                rank = (uint32_t)__popcll(match & lt_mask);
                gsize = (uint32_t)__popcll(match);
                gleader = (uint32_t)l;
            }
            pending &= ~match;
        }
        const bool leader = valid && gleader == lane;
        // 3. earlier chunks' count of the group's attribute (the table is read-only in this phase)
        const uint32_t home = crowd_slot_of(attr, slots);
        uint32_t prior = 0, found = kCrowdInvalid;
        if (leader) {
            uint32_t s = home;
            for (uint32_t probes = 0; probes < slots; ++probes) {
                const uint32_t c = s_cnt[s];
                if (c == 0) break;
                if (s_key[s] == attr) {
                    found = s;
                    prior = c;
                    break;
                }
                s = s + 1 == slots ? 0 : s + 1;
            }
        }
        __syncthreads();
        // 4. table update: one writer per attribute; new attributes claim an empty slot
        if (leader) {
            if (found != kCrowdInvalid) {
                s_cnt[found] = prior + gsize;
            } else {
                uint32_t s = home;
                for (uint32_t probes = 0; probes < slots; ++probes) {
                    if (atomicCAS(&s_cnt[s], 0u, gsize) == 0u) {
                        s_key[s] = attr;
                        break;
                    }
                    s = s + 1 == slots ? 0 : s + 1;
                }
            }
        }
        __syncthreads();
        // 5. decide and place
        const uint32_t before = __shfl(prior, (int)gleader) + rank;   // <= depth: no overflow
        const bool keep = valid && before < limit;
        const uint64_t kmask = __ballot(keep);
        const uint32_t pos = kept + (uint32_t)__popcll(kmask & lt_mask);
        if (keep && pos < k) {
            oi[pos] = idx;
            od[pos] = dist;
        }
        kept += (uint32_t)__popcll(kmask);
    }
    kept = min(kept, k);
    for (uint32_t i = kept + lane; i < k; i += 64) {
        oi[i] = kCrowdInvalid;
        od[i] = INFINITY;
    }
    if (lane == 0) out_cnt[q] = kept;
}

// ---- multi-attribute crowding: CrowdingMultidimensional::apply (restricts/crowding.rs:166-200) -------------------
// Entry i is kept iff, for EVERY dimension j, fewer than limits[j] earlier KEPT entries carry its attribute in
// dimension j.  Unlike the one-attribute rule this depends on the accept decisions of the earlier entries (an entry
// rejected by dimension 0 does not count in dimension 1), so "earlier entries with my attribute" decides nothing.
//
// Same frame as crowd_kernel: one wave per query, chunks of 64 entries, the next chunk's loads issued early.  The LDS
// table counts ACCEPTED entries only; its entries carry the dimension in the top four bits of the count word (counts
// stay <= 8192), so one open-addressed table serves every dimension.  At most n_dims * min(k, depth) keys are ever
// inserted (entries past the k-th kept one are not), and slots is sized from that bound.  Per chunk
//   1. per dimension, the ballot rounds of crowd_kernel give every lane the 64-bit mask of the chunk's lanes with an
//      equal attribute; the group's first lane reads the accepted count of earlier chunks from the table;
//   2. the chunk is decided by a fixed point over two ballots, acc (decided: accepted) and und (undecided).  For a
//      lane and dimension j, with lt = the lanes below it:
//        lower_j = prior_j + popc(match_j & acc & lt),   upper_j = lower_j + popc(match_j & und & lt);
//      accept when upper_j < limit_j for all j, reject when lower_j >= limit_j for some j, else stay undecided.  The
//      lowest undecided lane has lower == upper, so every iteration decides at least one lane (typical data: one or
//      two iterations).  A lane with k kept entries certainly before it is dropped at once: it is never written and
//      only lanes above it, which are never written either, could depend on it;
//   3. the accepted lanes that are written (the first k kept) add to the table: per dimension, the lowest such lane of
//      each group writes prior + group size, or claims an empty slot (compare-and-swap, as in crowd_kernel);
//   4. a prefix sum of the written lanes places the survivors.
struct CrowdMdLimits {
    uint32_t v[kCrowdMaxDims];
};

constexpr uint32_t kCrowdDimShift = 28;                       // count word = dimension << 28 | accepted count
constexpr uint32_t kCrowdCountMask = (1u << kCrowdDimShift) - 1u;

template <int ND>
__global__ __launch_bounds__(64) void crowd_md_kernel(const uint32_t *__restrict__ rows_idx,
                                                      const float *__restrict__ rows_dist,
                                                      const uint32_t *__restrict__ rows_cnt, uint32_t depth,
                                                      const uint64_t *__restrict__ attrs, uint64_t n_attrs, uint32_t k,
                                                      CrowdMdLimits limits, uint32_t slots,
                                                      uint32_t *__restrict__ out_idx, float *__restrict__ out_dist,
                                                      uint32_t *__restrict__ out_cnt) {
    extern __shared__ uint64_t s_key[];                              // [slots]
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_key + slots);   // [slots]
    const uint32_t q = blockIdx.x, lane = threadIdx.x;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    const uint32_t *ri = rows_idx + (size_t)q * depth;
    const float *rd = rows_dist + (size_t)q * depth;
    uint32_t *oi = out_idx + (size_t)q * k;
    float *od = out_dist + (size_t)q * k;
    const uint32_t cnt = min(rows_cnt[q], depth);   // a short row is walked to its count: no sentinel is looked up

    for (uint32_t s = lane; s < slots; s += 64) s_cnt[s] = 0;
    __syncthreads();

    uint32_t kept = 0;
    // chunk 0's loads
    uint32_t n_idx = kCrowdInvalid;
    float n_dist = INFINITY;
    uint64_t n_attr[ND];
#pragma unroll
    for (int j = 0; j < ND; ++j) n_attr[j] = 0;
    if (lane < cnt) {
        n_idx = ri[lane];
        n_dist = rd[lane];
        if ((uint64_t)n_idx < n_attrs) {
#pragma unroll
            for (int j = 0; j < ND; ++j) n_attr[j] = attrs[(size_t)j * n_attrs + n_idx];
        }
    }
    for (uint32_t base = 0; base < cnt && kept < k; base += 64) {
        const uint32_t i = base + lane;
        const bool valid = i < cnt;
        const uint32_t idx = n_idx;
        const float dist = n_dist;
        uint64_t attr[ND];
#pragma unroll
        for (int j = 0; j < ND; ++j) attr[j] = n_attr[j];
        if (i + 64 < cnt) {   // next chunk
            n_idx = ri[i + 64];
            n_dist = rd[i + 64];
            const bool have = (uint64_t)n_idx < n_attrs;
#pragma unroll
            for (int j = 0; j < ND; ++j) n_attr[j] = have ? attrs[(size_t)j * n_attrs + n_idx] : 0ull;
        }
        // 1. per dimension: the lanes of equal attribute, the accepted count of earlier chunks (table read-only)
        uint64_t match[ND];
        uint32_t prior[ND], found[ND];
#pragma unroll
        for (int j = 0; j < ND; ++j) {
            const uint32_t a_lo = (uint32_t)attr[j], a_hi = (uint32_t)(attr[j] >> 32);
            uint64_t pending = __ballot(valid);
            uint64_t mt = 0;
            while (pending) {
                const int l = __ffsll((unsigned long long)pending) - 1;
                const uint32_t b_lo = __shfl(a_lo, l), b_hi = __shfl(a_hi, l);
                const bool mine = valid && a_lo == b_lo && a_hi == b_hi;
                const uint64_t m = __ballot(mine);
                if (mine) mt = m;
                pending &= ~m;
            }
            match[j] = mt;
            const int gleader = mt ? __ffsll((unsigned long long)mt) - 1 : (int)lane;
            uint32_t pr = 0, fd = kCrowdInvalid;
            if (valid && gleader == (int)lane) {
                uint32_t s = crowd_md_slot_of(attr[j], (uint32_t)j, slots);
                for (uint32_t probes = 0; probes < slots; ++probes) {
                    const uint32_t c = s_cnt[s];
                    if (c == 0) break;
                    if ((c >> kCrowdDimShift) == (uint32_t)j && s_key[s] == attr[j]) {
                        fd = s;
                        pr = c & kCrowdCountMask;
                        break;
                    }
                    s = s + 1 == slots ? 0 : s + 1;
                }
            }
            prior[j] = __shfl(pr, gleader);
            found[j] = __shfl(fd, gleader);
        }
        // 2. the chunk's accept decisions
        uint64_t acc = 0, und = __ballot(valid);
        while (und) {
            const bool mine = (und >> lane) & 1ull;
            bool accept = mine, reject = false;
#pragma unroll
            for (int j = 0; j < ND; ++j) {
                const uint32_t lower = prior[j] + (uint32_t)__popcll(match[j] & acc & lt_mask);   // <= 8192 + 63
                const uint32_t upper = lower + (uint32_t)__popcll(match[j] & und & lt_mask);
                accept = accept && upper < limits.v[j];
                reject = reject || lower >= limits.v[j];
            }
            reject = reject || kept + (uint32_t)__popcll(acc & lt_mask) >= k;   // past the k-th kept: never written
            const uint64_t a = __ballot(accept && !reject), r = __ballot(mine && reject);
            acc |= a;
            und &= ~(a | r);
        }
        const uint32_t pos = kept + (uint32_t)__popcll(acc & lt_mask);
        const bool keep = ((acc >> lane) & 1ull) && pos < k;
        const uint64_t kmask = __ballot(keep);
        __syncthreads();
        // 3. table update: per dimension one writer per attribute among the kept lanes
#pragma unroll
        for (int j = 0; j < ND; ++j) {
            const uint64_t grp = match[j] & kmask;
            if (keep && (grp & lt_mask) == 0) {
                const uint32_t gsize = (uint32_t)__popcll(grp);
                const uint32_t tag = (uint32_t)j << kCrowdDimShift;
                if (found[j] != kCrowdInvalid) {
                    s_cnt[found[j]] = tag | (prior[j] + gsize);
                } else {
                    uint32_t s = crowd_md_slot_of(attr[j], (uint32_t)j, slots);
                    for (uint32_t probes = 0; probes < slots; ++probes) {
                        if (atomicCAS(&s_cnt[s], 0u, tag | gsize) == 0u) {
                            s_key[s] = attr[j];
                            break;
                        }
                        s = s + 1 == slots ? 0 : s + 1;
                    }
                }
            }
        }
        __syncthreads();
        // 4. place
        if (keep) {
            oi[pos] = idx;
            od[pos] = dist;
        }
        kept += (uint32_t)__popcll(kmask);
    }
    for (uint32_t i = kept + lane; i < k; i += 64) {
        oi[i] = kCrowdInvalid;
        od[i] = INFINITY;
    }
    if (lane == 0) out_cnt[q] = kept;
}

}  // namespace

int crowd_launch(const uint32_t *rows_idx, const float *rows_dist, const uint32_t *rows_cnt, uint32_t nq,
                 uint32_t depth, const uint64_t *attrs, uint64_t n_attrs, uint32_t k, uint32_t limit,
                 uint32_t *out_idx, float *out_dist, uint32_t *out_cnt, hipStream_t st) {
    if (nq == 0) return SCANN_HIP_OK;
    if (depth == 0 || depth > kCrowdMaxDepth)
        return fail(SCANN_HIP_UNIMPLEMENTED, "crowding depth " + std::to_string(depth) + " exceeds " +
                                                 std::to_string(kCrowdMaxDepth));
    if (k > depth) return fail(SCANN_HIP_INVALID_ARGUMENT, "crowding: depth < k");
    if (!attrs) n_attrs = 0;
    const uint32_t slots = crowd_table_slots(depth);
    const size_t lds = (size_t)slots * 12;
    return launch(crowd_kernel, dim3(nq), dim3(64), lds, st, rows_idx, rows_dist, rows_cnt, depth, attrs, n_attrs, k, limit,
                  slots, out_idx, out_dist, out_cnt);
}

int crowd_md_launch(const uint32_t *rows_idx, const float *rows_dist, const uint32_t *rows_cnt, uint32_t nq,
                    uint32_t depth, const uint64_t *attrs, uint32_t n_dims, uint64_t n_attrs, uint32_t k,
                    const uint32_t *limits, uint32_t *out_idx, float *out_dist, uint32_t *out_cnt, hipStream_t st) {
    if (nq == 0) return SCANN_HIP_OK;
    if (n_dims == 0 || n_dims > kCrowdMaxDims)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "crowding dimensions must be 1.." + std::to_string(kCrowdMaxDims));
    if (depth == 0 || depth > kCrowdMaxDepth)
        return fail(SCANN_HIP_UNIMPLEMENTED, "crowding depth " + std::to_string(depth) + " exceeds " +
                                                 std::to_string(kCrowdMaxDepth));
    if (k > depth) return fail(SCANN_HIP_INVALID_ARGUMENT, "crowding: depth < k");
    const uint64_t keys = (uint64_t)n_dims * std::min(k, depth);
    if (keys > kCrowdMdMaxKeys)
        return fail(SCANN_HIP_UNIMPLEMENTED, "multi-attribute crowding: n_dims * k = " + std::to_string(keys) + " exceeds " +
                                                 std::to_string(kCrowdMdMaxKeys));
    if (!attrs) n_attrs = 0;
    CrowdMdLimits lim{};
    for (uint32_t j = 0; j < n_dims; ++j) lim.v[j] = limits[j];
    const uint32_t slots = crowd_table_slots((uint32_t)keys);   // > keys: a probe meets its key or an empty slot
    const size_t lds = (size_t)slots * 12;
    return with_value<1, 2, 3, 4, 5, 6, 7, 8>((int)n_dims, [&](auto ND) {
        return launch(crowd_md_kernel<decltype(ND)::value>, dim3(nq), dim3(64), lds, st, rows_idx, rows_dist, rows_cnt,
                      depth, attrs, n_attrs, k, lim, slots, out_idx, out_dist, out_cnt);
    });
}

}  // namespace scann

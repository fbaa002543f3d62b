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

}  // namespace scann

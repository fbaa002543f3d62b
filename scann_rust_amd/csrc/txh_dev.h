// txh_dev.h -- device helpers, types and constants that more than one unit of the tree / flat-hasher search reads
// (txh.hip, txh_prefilter.hip).  Internal: only those units include it.  The library is built without relocatable
// device code, so a __device__ function two units call lives here (forceinline: every unit gets its own copy) and a
// __global__ function lives in exactly one unit.  A helper only one unit calls stays in that unit.
#pragma once
#include "launch.h"
#include "txh.h"

namespace scann {

// Per-query allow-lists (scann_hip_search_opts.allow_bitmap_stride): query q of the call reads the bitmap that starts
// `stride` 64-bit words after query q - 1's; stride 0 = one bitmap for the whole batch.  Every site forms this address
// inside its branch on the (wave-uniform) base pointer, so an unfiltered search executes none of it.
__device__ __forceinline__ const uint64_t *query_allow(const uint64_t *allow, uint64_t stride, uint32_t q) {
    return allow + (size_t)q * stride;
}
// RestrictFilter::is_allowed (restricts/mod.rs:17-30) for the allow-bitmap form of
// search_with_filter (tree_x_hybrid/mod.rs:327-332): bit i of the bitmap = datapoint i.
// Indices at or beyond the bitmap's capacity are not allowed (allowlist.rs:97-100).
// The six-argument form tests the bitmap of query q (query_allow).
__device__ __forceinline__ bool row_allowed(const TxhIndexDev &ix, const uint64_t *allow, uint64_t allow_bits, uint32_t csr) {
    if (!allow) return true;
    const uint32_t idx = ix.leaf_ids ? ix.leaf_ids[csr] : csr;
    return idx < allow_bits && ((allow[idx >> 6] >> (idx & 63u)) & 1ull);
}
__device__ __forceinline__ bool row_allowed(const TxhIndexDev &ix, const uint64_t *allow, uint64_t stride, uint32_t q,
                                            uint64_t allow_bits, uint32_t csr) {
    if (!allow) return true;
    return row_allowed(ix, query_allow(allow, stride, q), allow_bits, csr);
}
// the test of a kernel with a per-query instantiation: PQ = false is the one-bitmap form, word for word
template <bool PQ>
__device__ __forceinline__ bool row_allowed_if(const TxhIndexDev &ix, const uint64_t *allow, uint64_t stride, uint32_t q,
                                               uint64_t allow_bits, uint32_t csr) {
    if constexpr (PQ) return row_allowed(ix, allow, stride, q, allow_bits, csr);
    else return row_allowed(ix, allow, allow_bits, csr);
}

// A kernel whose one-bitmap form must keep its registers to the last one takes no stride argument: its
// per-query form is the instantiation for PqCodec<C>, launched with the stride packed above the capacity in the
// allow_bits it already takes.  Both fit 32 bits: a datapoint index is a u32 and 0xFFFFFFFF is none, so a capacity
// clamps to 2^32 - 1 exactly; a stride of 2^32 words (32 GiB per query) is refused by the entry points.
static inline uint64_t pq_allow_bits(uint64_t allow_bits, uint64_t stride) {
    return (stride << 32) | (allow_bits < 0xFFFFFFFFull ? allow_bits : 0xFFFFFFFFull);
}
template <bool PQ>
__device__ __forceinline__ uint64_t pq_capacity(uint64_t allow_bits) {
    if constexpr (PQ) return allow_bits & 0xFFFFFFFFull;
    else return allow_bits;
}
template <bool PQ>
__device__ __forceinline__ uint64_t pq_stride(uint64_t allow_bits) {
    if constexpr (PQ) return allow_bits >> 32;
    else return 0;
}

// Code layouts the scan understands.  BITS = 4: K <= 16, 8 subspaces per u32 word
// (PackedCodes4Bit, hashes/lut16.rs:43-61), 16-entry tables.  BITS = 8: 16 < K <= 256 (the
// reference's default 256 x 8 codebooks, hashes/hasher.rs:36-46), one byte per subspace, 4
// subspaces per word, 256-entry tables.  A subspace's quad-interleaved table is KP x 16 B.
template <int S_, int BITS_>
struct Codec {
    static constexpr int S = S_, BITS = BITS_;
    static constexpr bool PQ = false;                             // (PqCodec: the per-query instantiation of a kernel)
    static constexpr int NWORDS = BITS == 4 ? S / 8 : S / 4;      // packed u32 words per point
    static constexpr int REGS = BITS == 4 ? 2 * NWORDS : NWORDS;  // registers per point in the scan
    static constexpr int KP = BITS == 4 ? 16 : 256;               // table entries per subspace
    static constexpr int SUB_BYTES = KP * 16;
    static constexpr int LUT4 = S * KP;                           // float4 per quad
    // points per thread per tile chunk: byte-code tables are 16x larger per subspace and there
    // are 4x fewer subspaces, so a tile takes 4x more points per staged table
    static constexpr int PPT = BITS == 4 ? (int)kScanPPT : 8;
    static constexpr int TP = (int)kScanThreads * PPT;            // points per tile chunk
    static_assert((S - 1) * SUB_BYTES < 65536, "ds_read immediate offset");
    // workgroups per CU the kernel is built for (LDS: two LUT buffers + survivor stage)
    static constexpr int WGS = BITS == 4 ? (S <= 32 ? (int)kScanWaves : 3)
                                         : (2 * LUT4 * 16 + 12288 <= 40 * 1024 ? 4
                                            : 2 * LUT4 * 16 + 12288 <= 80 * 1024 ? 2 : 1);
    // packed words -> register form: 4-bit codes pre-shifted to "code * 16" bytes
    __device__ static __forceinline__ void unpack(const uint32_t (&w)[NWORDS], uint32_t (&r)[REGS]) {
        if constexpr (BITS == 4) {
#pragma unroll
            for (int wi = 0; wi < NWORDS; ++wi) {
                r[2 * wi] = (w[wi] & 0x0F0F0F0Fu) << 4;
                r[2 * wi + 1] = w[wi] & 0xF0F0F0F0u;
            }
        } else {
#pragma unroll
            for (int wi = 0; wi < NWORDS; ++wi) r[wi] = w[wi];
        }
    }
    // byte offset of subspace s's code inside that subspace's table (code * 16)
    __device__ static __forceinline__ uint32_t offset(const uint32_t (&r)[REGS], int s) {
        if constexpr (BITS == 4) {
            const int wi = s >> 3, b = (s >> 1) & 3, h = s & 1;
            return (r[2 * wi + h] >> (8 * b)) & 0xFFu;
        } else {
            return ((r[s >> 2] >> (8 * (s & 3))) & 0xFFu) << 4;
        }
    }
    __device__ static __forceinline__ void load_words(const uint32_t *src, uint32_t (&w)[NWORDS]) {
        if constexpr (NWORDS == 4) {
            const uint4 v = *reinterpret_cast<const uint4 *>(src);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else if constexpr (NWORDS == 2) {
            const uint2 v = *reinterpret_cast<const uint2 *>(src);
            w[0] = v.x; w[1] = v.y;
        } else {
#pragma unroll
            for (int wi = 0; wi < NWORDS; ++wi) w[wi] = src[wi];
        }
    }
    __device__ static __forceinline__ void store_words(uint32_t *dst, const uint32_t (&w)[NWORDS]) {
        if constexpr (NWORDS == 4) {
            *reinterpret_cast<uint4 *>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
        } else if constexpr (NWORDS == 2) {
            *reinterpret_cast<uint2 *>(dst) = make_uint2(w[0], w[1]);
        } else {
#pragma unroll
            for (int wi = 0; wi < NWORDS; ++wi) dst[wi] = w[wi];
        }
    }
};

// the same layout, naming the per-query instantiation of a kernel (pq_allow_bits)
template <typename C>
struct PqCodec : C {
    static constexpr bool PQ = true;
};

// with_codec(ix, f) calls f(Codec<S, BITS>{}) for the index's code layout and returns what f returns; only the listed
// layouts are instantiated (cf. with_value in launch.h).
template <typename F>
int with_codec(const TxhIndexDev &ix, F &&f) {
    switch (ix.code_bits * 1000 + ix.S) {
        case 4008: return f(Codec<8, 4>{});
        case 4016: return f(Codec<16, 4>{});
        case 4024: return f(Codec<24, 4>{});
        case 4032: return f(Codec<32, 4>{});
        case 4048: return f(Codec<48, 4>{});
        case 4064: return f(Codec<64, 4>{});
        case 8004: return f(Codec<4, 8>{});
        case 8008: return f(Codec<8, 8>{});
        case 8016: return f(Codec<16, 8>{});
        default:
            return fail(SCANN_HIP_UNIMPLEMENTED,
                        "num_subspaces must be 8,16,24,32,48,64 (num_codes <= 16) or 4,8,16 (num_codes <= 256)");
    }
}

// One item of the tile queue of the queue-driven scan kernels.  leaf: the largest l with tile_off[l] <= tile; its points
// are [lb, lb + size) and its (query, leaf) pairs the slots [slot0, slot_end); local: the item's number inside the leaf,
// from which every kernel derives its own chunk / range and quad numbers.  All wave-uniform (scalar loads).
struct WorkItem {
    uint32_t leaf, lb, size, local, slot0, slot_end;
};
__device__ __forceinline__ WorkItem decode_item(const TxhIndexDev &ix, const uint32_t *tile_off, const uint32_t *pair_off,
                                                uint32_t tile) {
    uint32_t lo = 0, hi = ix.L;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (uniform_load(tile_off + mid) <= tile) lo = mid; else hi = mid;
    }
    WorkItem w;
    w.leaf = lo;
    w.lb = uniform_load(ix.leaf_off + lo);
    w.size = uniform_load(ix.leaf_off + lo + 1) - w.lb;
    w.local = tile - uniform_load(tile_off + lo);
    w.slot0 = uniform_load(pair_off + lo);
    w.slot_end = uniform_load(pair_off + lo + 1);
    return w;
}

// Next tile of this workgroup: XCD x (blockIdx % 8) owns tiles t = x (mod 8) in queue x and
// steals from the other queues when its own is dry.  kInvalid = no tiles left.
__device__ __forceinline__ uint32_t grab_tile(uint32_t *queues, uint32_t total_tiles) {
    const uint32_t xcd = blockIdx.x & 7u;
    for (uint32_t a2 = 0; a2 < 8u; ++a2) {
        const uint32_t x = (xcd + a2) & 7u;
        const uint32_t nx = (total_tiles + 7u - x) >> 3;   // tiles = x (mod 8)
        uint32_t *ctr = queues + x * CNT_XQ_STRIDE;
        if (a2 && __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= nx) continue;
        const uint32_t l = atomicAdd(ctr, 1u);
        if (l < nx) return l * 8u + x;
    }
    return kInvalid;
}

// points per work item of the integer-MFMA prefilters (txh_prefilter.hip K6d); the work lists are cut to it
#ifndef SCANN_MFMA_RANGE
#define SCANN_MFMA_RANGE 2048
#endif
constexpr uint32_t kMfmaRange = SCANN_MFMA_RANGE;     // points per item
// ... of the sparse prefilter's 64-pair form: kSpRange64 (txh.h; the plan sizes the survivor bitmaps by it)

// per pair slot, next to its quantised tables (lut8_build_kernel, txh_prefilter.hip; read again by K5e in txh.hip)
struct Lut8Meta {
    double bias_sum;   // sum over subspaces of the per-subspace minimum
    double scale;      // table step; 0 = this pair is not prefiltered (every point passes)
};

}  // namespace scann

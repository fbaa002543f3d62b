// tokens.h -- the device token map (RestrictTokenMap, restricts/allowlist.rs:184-244) and the word-wise combination of
// strided allow-bitmap blocks (AndFilter / OrFilter / NotFilter, restricts/mod.rs:98-170).
#pragma once
#include "common.h"

namespace scann {

// 64-bit words / 32-bit LDS words of one tile of token_bitmap_kernel
constexpr uint32_t kTokenTileWords = SCANN_HIP_TOKEN_TILE_BITS / 64;
constexpr uint32_t kTokenTileU32 = SCANN_HIP_TOKEN_TILE_BITS / 32;
static_assert((SCANN_HIP_TOKEN_TILE_BITS & (SCANN_HIP_TOKEN_TILE_BITS - 1)) == 0 && SCANN_HIP_TOKEN_TILE_BITS >= 128,
              "the tile is a power of two of at least one 16-byte store");

// one word of a combination: op is SCANN_HIP_ALLOW_AND / _OR / _ANDNOT / _NOT (checked by the caller)
__host__ __device__ static inline uint64_t allow_combine_word(int op, uint64_t a, uint64_t b) {
    switch (op) {
        case SCANN_HIP_ALLOW_AND: return a & b;
        case SCANN_HIP_ALLOW_OR: return a | b;
        case SCANN_HIP_ALLOW_ANDNOT: return a & ~b;
        default: return ~a;
    }
}

// threads of a workgroup of the kernels that write bitmap blocks (token_bitmap_kernel, allow_combine_kernel,
// range_bitmap_kernel)
constexpr uint32_t kBitmapThreads = 256;

#ifdef __HIPCC__
// nw words to dst (8-byte aligned), from src (LDS) or zeros (src null): 16-byte stores wherever dst allows them, an
// 8-byte store for a misaligned first word and for an odd last one.  Every thread of a block of kBitmapThreads calls.
__device__ __forceinline__ void store_words(uint64_t *__restrict__ dst, const uint64_t *src, uint64_t nw) {
    if (nw == 0) return;
    const uint64_t head = ((uint64_t)dst >> 3) & 1ull;
    const uint64_t pairs = (nw - head) >> 1, tail = (nw - head) & 1ull;
    if (threadIdx.x == 0) {
        if (head) dst[0] = src ? src[0] : 0ull;
        if (tail) dst[nw - 1] = src ? src[nw - 1] : 0ull;
    }
    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
    for (uint64_t p = threadIdx.x; p < pairs; p += kBitmapThreads) {
        const uint64_t w = head + 2 * p;
        u64x2 v = {0ull, 0ull};
        if (src) v = u64x2{src[w], src[w + 1]};
#ifdef SCANN_TOKEN_NT_STORES   // (tools/time_token_filters.py's variant build: DESIGN 3.3c-t has the comparison)
        __builtin_nontemporal_store(v, reinterpret_cast<u64x2 *>(dst + w));
#else
        *reinterpret_cast<u64x2 *>(dst + w) = v;
#endif
    }
}
#endif

// d_out[i * stride .. (i + 1) * stride): bit j set iff j is in the posting of one of query i's tokens
// d_q_tokens[d_q_offsets[i] .. d_q_offsets[i + 1]); every other word zero.  The map is three device arrays: ntok
// ascending distinct tokens, ntok + 1 posting offsets, the ascending in-range (< bits) postings.  stride >=
// ceil(bits / 64) (the caller checks).  Enqueue only: one kernel, no clear, no global atomic.
int token_bitmaps_launch(const uint64_t *d_map_tokens, uint64_t ntok, const uint64_t *d_map_offsets, const uint32_t *d_postings,
                         const uint64_t *d_q_tokens, const uint64_t *d_q_offsets, uint32_t nq, uint64_t bits, uint64_t stride,
                         uint64_t *d_out, hipStream_t st);

// d_out row i, words [0, ceil(bits / 64)) = op(a row i, b row i), the last word masked to bits; a stride of 0 shares
// one row among all queries.  Strides and op checked by the caller.  Enqueue only: one kernel.
int allow_combine_launch(int op, const uint64_t *d_a, uint64_t stride_a, const uint64_t *d_b, uint64_t stride_b, uint32_t nq,
                         uint64_t bits, uint64_t *d_out, uint64_t stride_out, hipStream_t st);

}  // namespace scann

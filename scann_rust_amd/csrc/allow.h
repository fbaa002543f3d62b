// allow.h -- strided allow-bitmap blocks (scann_hip_search_opts.allow_bitmap_stride) from per-query id lists:
// RestrictAllowlist::from_indices (restricts/allowlist.rs:27-40) for a whole batch, on the device.
#pragma once
#include "common.h"

namespace scann {

// words of one bitmap of capacity `bits`
static inline uint64_t allow_words(uint64_t bits) { return bits / 64 + (bits % 64 ? 1 : 0); }

// scann_hip_search_opts.allow_bitmap_stride of a call: 0 where there is no bitmap (the field is ignored without one)
static inline uint64_t allow_stride_of(const scann_hip_search_opts *o) {
    return o && o->allow_bitmap ? o->allow_bitmap_stride : 0;
}
// words a host entry point copies for nq queries: one bitmap, or nq of them `stride` words apart
static inline size_t allow_copy_words(const scann_hip_search_opts *o, uint32_t nq) {
    const uint64_t stride = allow_stride_of(o);
    return (size_t)(stride ? (uint64_t)nq * stride : allow_words(o->allow_bitmap_bits));
}
// InvalidArgument for a stride that makes consecutive bitmaps overlap
static inline int check_allow_stride(const scann_hip_search_opts *o) {
    const uint64_t stride = allow_stride_of(o);
    if (stride && stride < allow_words(o->allow_bitmap_bits))
        return fail(SCANN_HIP_INVALID_ARGUMENT, "allow_bitmap_stride is smaller than one bitmap (ceil(allow_bitmap_bits / 64) words)");
    if (stride > 0xFFFFFFFFull)   // (32 GiB per query; the kernels carry the stride in 32 bits, txh_dev.h pq_allow_bits)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "allow_bitmap_stride must be below 2^32 words");
    return SCANN_HIP_OK;
}
// the entry points that take one bitmap per call only
static inline int refuse_allow_stride(const scann_hip_search_opts *o, const char *what) {
    if (allow_stride_of(o))
        return fail(SCANN_HIP_UNIMPLEMENTED, std::string("per-query allow-bitmaps (allow_bitmap_stride != 0) are not built for ") + what);
    return SCANN_HIP_OK;
}

// the checks every builder of a bitmap block shares: stride_words >= ceil(bits / 64) and < 2^32, else InvalidArgument
int check_block_args(uint64_t bits, uint64_t stride_words);

// ---- a filtered batch in one host call: the block is built on the device, the enqueue-only search reads it on the
// same stream (scann_hip_search_batched_tokens, scann_hip_search_batched_ranges) -----------------------------------
// grow-only staging of such a call, owned by the filter's handle (one call at a time per handle)
struct FilterSearchBufs {
    DevBuf block, queries, idx, dist, count;
};
// the argument checks the two entries share; `filter_is` names the filter in the allow_bitmap refusal
int filter_search_check(const scann_hip_index *index, const float *queries, uint32_t q_stride, uint32_t q_dim, uint32_t k,
                        const scann_hip_search_opts *opts, const uint32_t *out_idx, const float *out_dist,
                        const uint32_t *out_count, const char *filter_is);
// sizes the staging and enqueues the queries' upload on st
int filter_search_begin(FilterSearchBufs &b, hipStream_t st, const float *queries, uint32_t nq, uint32_t q_stride, uint32_t k);
// after the block's kernel was enqueued on st into b.block (`stride` words a query, capacity `bits`): the enqueue-only
// search right behind it, the rows back; where that search reports Aborted or ResourceExhausted the batch is answered
// by scann_hip_search_batched under the same block.  Synchronous.
int filter_search_finish(scann_hip_index *index, FilterSearchBufs &b, hipStream_t st, const float *queries, uint32_t nq,
                         uint32_t q_stride, uint32_t q_dim, uint32_t k, scann_hip_search_opts o, uint64_t bits,
                         uint64_t stride, uint32_t *out_idx, float *out_dist, uint32_t *out_count);

// d_out[i * stride .. (i + 1) * stride): bit id set for every id < bits of d_ids[d_offsets[i] .. d_offsets[i + 1]),
// every other word zero.  stride >= allow_words(bits) (the caller checks).  Enqueue only: a clear and one kernel.
int allow_from_ids_launch(const uint32_t *d_ids, const uint64_t *d_offsets, uint32_t nq, uint64_t bits, uint64_t stride,
                          uint64_t *d_out, hipStream_t st);

}  // namespace scann

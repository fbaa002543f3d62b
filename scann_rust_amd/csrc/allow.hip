// allow.hip -- per-query allow-bitmaps from id lists.  Callers of a filtered batch hold one id list per query (an ACL,
// a tenant's rows); the search reads one bitmap per query, `stride` 64-bit words apart
// (scann_hip_search_opts.allow_bitmap_stride).  RestrictAllowlist::from_indices (restricts/allowlist.rs:27-40) sets
// bit id for every id below the capacity and ignores the others; this unit does that for nq lists at once, on the
// host (the model and the no-GPU form) and on the device, where the lists are a fraction of the bytes of the bitmaps
// they become.
//
// Device form: hipMemsetAsync over the whole block (gap words included), then ONE kernel.  Workgroup (x, y) walks the
// lists of queries y, y + gridDim.y, ... in steps of gridDim.x * 256 ids; a thread ORs its id's bit into the query's
// word with a 64-bit atomic (agent scope, no return value): duplicates and any order give the same words.  The
// total number of ids stays on the device (offsets[nq] is never read by the host): no synchronisation.
#include <algorithm>
#include <string>
#include <vector>

#include "allow.h"
#include "comm.h"   // ctx_device
#include "launch.h"

namespace scann {

namespace {

constexpr uint32_t kAllowThreads = 256;

__global__ __launch_bounds__(kAllowThreads) void allow_scatter_kernel(const uint32_t *__restrict__ ids,
                                                                      const uint64_t *__restrict__ offsets, uint32_t nq,
                                                                      uint64_t bits, uint64_t stride,
                                                                      unsigned long long *__restrict__ out) {
    for (uint32_t q = blockIdx.y; q < nq; q += gridDim.y) {
        const uint64_t e0 = offsets[q], e1 = offsets[q + 1];
        unsigned long long *row = out + (size_t)q * stride;
        for (uint64_t e = e0 + (uint64_t)blockIdx.x * kAllowThreads + threadIdx.x; e < e1;
             e += (uint64_t)gridDim.x * kAllowThreads) {
            const uint32_t id = ids[e];
            // id < bits: word id / 64 < ceil(bits / 64) <= stride, inside the query's own row
            if (id < bits) atomicOr(row + (id >> 6), 1ull << (id & 63u));
        }
    }
}

}  // namespace

int allow_from_ids_launch(const uint32_t *d_ids, const uint64_t *d_offsets, uint32_t nq, uint64_t bits, uint64_t stride,
                          uint64_t *d_out, hipStream_t st) {
    if (nq == 0 || stride == 0) return SCANN_HIP_OK;
    SCANN_HIP_CHECK(hipMemsetAsync(d_out, 0, (size_t)nq * stride * 8, st));
    if (bits == 0) return SCANN_HIP_OK;
    // enough workgroups to fill the device whatever the split between queries and ids per query
    const uint32_t gy = std::min<uint32_t>(nq, 65535u);
    const uint32_t gx = std::max<uint32_t>(1u, std::min<uint32_t>(64u, (uint32_t)num_cus() * 8u / gy));
    return launch(allow_scatter_kernel, dim3(gx, gy), dim3(kAllowThreads), 0, st, d_ids, d_offsets, nq, bits, stride,
                  reinterpret_cast<unsigned long long *>(d_out));
}

int check_block_args(uint64_t bits, uint64_t stride_words) {
    if (stride_words < allow_words(bits))
        return fail(SCANN_HIP_INVALID_ARGUMENT, "allow-bitmap stride is smaller than one bitmap (ceil(bits / 64) words)");
    if (stride_words > 0xFFFFFFFFull)   // (check_allow_stride's limit: the search kernels carry the stride in 32 bits)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "allow-bitmap stride must be below 2^32 words");
    return SCANN_HIP_OK;
}

int filter_search_check(const scann_hip_index *index, const float *queries, uint32_t q_stride, uint32_t q_dim, uint32_t k,
                        const scann_hip_search_opts *opts, const uint32_t *out_idx, const float *out_dist,
                        const uint32_t *out_count, const char *filter_is) {
    if (!queries || !out_idx || !out_dist || !out_count) return fail(SCANN_HIP_INVALID_ARGUMENT, "null query/output pointer");
    if (k == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "k must be > 0");
    if (opts && opts->allow_bitmap)
        return fail(SCANN_HIP_INVALID_ARGUMENT, std::string(filter_is) + " are the filter: allow_bitmap must be null");
    if (q_dim != scann_hip_index_dimensionality(index)) return fail(SCANN_HIP_INVALID_ARGUMENT, "Query dimensionality mismatch");
    if (q_stride < q_dim) return fail(SCANN_HIP_INVALID_ARGUMENT, "q_stride < q_dim");
    return SCANN_HIP_OK;
}

int filter_search_begin(FilterSearchBufs &b, hipStream_t st, const float *queries, uint32_t nq, uint32_t q_stride, uint32_t k) {
    const size_t qb = (size_t)nq * q_stride * 4, ob = (size_t)nq * k * 4;
    SCANN_TRY(b.queries.ensure(qb));
    SCANN_TRY(b.idx.ensure(ob));
    SCANN_TRY(b.dist.ensure(ob));
    SCANN_TRY(b.count.ensure((size_t)nq * 4));
    SCANN_HIP_CHECK(hipMemcpyAsync(b.queries.p, queries, qb, hipMemcpyHostToDevice, st));
    return SCANN_HIP_OK;
}

int filter_search_finish(scann_hip_index *index, FilterSearchBufs &b, hipStream_t st, const float *queries, uint32_t nq,
                         uint32_t q_stride, uint32_t q_dim, uint32_t k, scann_hip_search_opts o, uint64_t bits,
                         uint64_t stride, uint32_t *out_idx, float *out_dist, uint32_t *out_count) {
    const size_t ob = (size_t)nq * k * 4;
    o.allow_bitmap = b.block.as<uint64_t>();
    o.allow_bitmap_bits = bits;
    o.allow_bitmap_stride = stride;
    SCANN_TRY(scann_hip_search_batched_device(index, b.queries.as<float>(), nq, q_stride, k, &o, b.idx.as<uint32_t>(),
                                              b.dist.as<float>(), b.count.as<uint32_t>(), st));
    const int status = scann_hip_index_last_device_status(index, st);   // (synchronises the stream)
    if (status == SCANN_HIP_ABORTED || status == SCANN_HIP_RESOURCE_EXHAUSTED) {
        // the enqueue-only search's documented misses: the host entry point repeats such a batch, under the same block
        std::vector<uint64_t> block((size_t)nq * stride);
        SCANN_HIP_CHECK(hipMemcpy(block.data(), b.block.p, block.size() * 8, hipMemcpyDeviceToHost));
        o.allow_bitmap = block.data();
        return scann_hip_search_batched(index, queries, nq, q_stride, q_dim, k, &o, out_idx, out_dist, out_count);
    }
    SCANN_TRY(status);
    SCANN_HIP_CHECK(hipMemcpyAsync(out_idx, b.idx.p, ob, hipMemcpyDeviceToHost, st));
    SCANN_HIP_CHECK(hipMemcpyAsync(out_dist, b.dist.p, ob, hipMemcpyDeviceToHost, st));
    SCANN_HIP_CHECK(hipMemcpyAsync(out_count, b.count.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    return SCANN_HIP_OK;
}

}  // namespace scann

using namespace scann;

extern "C" {

int scann_hip_allow_bitmaps_from_ids(const uint32_t *ids, const uint64_t *offsets, uint32_t nq, uint64_t bits,
                                     uint64_t stride_words, uint64_t *out_words) {
    if (stride_words < allow_words(bits))
        return fail(SCANN_HIP_INVALID_ARGUMENT, "allow-bitmap stride is smaller than one bitmap (ceil(bits / 64) words)");
    if (nq == 0) return SCANN_HIP_OK;
    if (!offsets || (stride_words && !out_words)) return fail(SCANN_HIP_INVALID_ARGUMENT, "null offsets/output pointer");
    for (uint32_t q = 0; q < nq; ++q)
        if (offsets[q + 1] < offsets[q]) return fail(SCANN_HIP_INVALID_ARGUMENT, "offsets must ascend");
    if (offsets[nq] > offsets[0] && !ids) return fail(SCANN_HIP_INVALID_ARGUMENT, "ids is null");
    for (uint64_t i = 0; i < (uint64_t)nq * stride_words; ++i) out_words[i] = 0;
    for (uint32_t q = 0; q < nq; ++q) {
        uint64_t *row = out_words + (size_t)q * stride_words;
        for (uint64_t e = offsets[q]; e < offsets[q + 1]; ++e) {
            const uint32_t id = ids[e];
            if (id < bits) row[id >> 6] |= 1ull << (id & 63u);
        }
    }
    return SCANN_HIP_OK;
}

int scann_hip_allow_bitmaps_from_ids_device(scann_hip_ctx *ctx, const uint32_t *d_ids, const uint64_t *d_offsets,
                                            uint32_t nq, uint64_t bits, uint64_t stride_words, uint64_t *d_out_words,
                                            void *hip_stream) {
    if (!ctx) return fail(SCANN_HIP_INVALID_ARGUMENT, "context is null");
    if (stride_words < allow_words(bits))
        return fail(SCANN_HIP_INVALID_ARGUMENT, "allow-bitmap stride is smaller than one bitmap (ceil(bits / 64) words)");
    if (nq == 0) return SCANN_HIP_OK;
    if (!d_offsets || !d_ids || (stride_words && !d_out_words))
        return fail(SCANN_HIP_INVALID_ARGUMENT, "null ids/offsets/output pointer");
    SCANN_HIP_CHECK(hipSetDevice(ctx_device(ctx)));
    return allow_from_ids_launch(d_ids, d_offsets, nq, bits, stride_words, d_out_words, static_cast<hipStream_t>(hip_stream));
}

}  // extern "C"

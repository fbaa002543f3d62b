// api_stages.hip -- C ABI, the stages behind a search at k = depth: crowding attributes, crowding, multi-attribute
// crowding and MMR, through the slots and the enqueue-only search of api_search.hip.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "allow.h"
#include "crowd.h"
#include "handle.h"
#include "mmr.h"

using namespace scann;

// ---- the stage behind a search at k = depth: crowding, multi-attribute crowding or MMR ----------------------------
// The three kinds differ only in the kernel that turns the [nq][depth] rows into the [nq][k] answer; the routes (host
// entry on the device, host entry through the plain search with its repeats, device entry, caller rows) are one code.
struct Stage {
    enum Kind { Crowd, CrowdMd, Mmr } kind = Crowd;
    uint32_t limit = 0;                 // Crowd: per_crowd_limit
    const uint32_t *limits = nullptr;   // CrowdMd: [n_limits] host array
    uint32_t n_limits = 0;
    float lambda = 0.0f;                // Mmr: clamped to [0, 1] by stage_args
    const char *name() const { return kind == Mmr ? "MMR" : "crowding"; }
    uint32_t max_depth() const { return kind == Mmr ? kMmrMaxDepth : kCrowdMaxDepth; }
};

// The f32 rows of the handle by datapoint index (MMR's similarities), or why it has none.
static int mmr_rows(const scann_hip_index *ix, const float **rows, uint64_t *n, uint32_t *dim, uint32_t *stride,
                    int *measure) {
    if (ix->kind == KIND_BF) {
        if (ix->bf.fmt != 0) return fail(SCANN_HIP_UNIMPLEMENTED, "MMR over quantized rows is not built");
        *rows = ix->bf.rows, *n = ix->bf.n, *dim = ix->bf.dim, *stride = ix->bf.stride, *measure = ix->bf.measure;
        return SCANN_HIP_OK;
    }
    if (ix->sharded) return fail(SCANN_HIP_UNIMPLEMENTED, "MMR on a shard (leaf_sizes_global) is not built");
    if (ix->tx.qfmt) return fail(SCANN_HIP_UNIMPLEMENTED, "MMR over quantized rows is not built");
    if (ix->proj.kind) return fail(SCANN_HIP_UNIMPLEMENTED, "MMR on a handle that searches through a projection is not built");
    if (!ix->tx.rows) return fail(SCANN_HIP_FAILED_PRECONDITION, "MMR needs the handle's f32 rows (desc.data)");
    if (ix->tx.rows_csr && !ix->tx.ah_mode)
        return fail(SCANN_HIP_UNIMPLEMENTED, "MMR over rows held in CSR order is not built");
    *rows = ix->tx.rows, *n = ix->tx.n_local, *dim = ix->tx.dim, *stride = ix->tx.stride, *measure = ix->tx.measure;
    return SCANN_HIP_OK;
}

// depth = 0 means k; depth < k -> InvalidArgument; then the stage's own preconditions
static int stage_args(const scann_hip_index *ix, Stage *sg, uint32_t k, uint32_t *depth) {
    if (*depth == 0) *depth = k;
    if (*depth < k) return fail(SCANN_HIP_INVALID_ARGUMENT, std::string(sg->name()) + " depth " + std::to_string(*depth) +
                                                                 " is smaller than k " + std::to_string(k));
    if (sg->kind == Stage::Crowd) {
        if (!ix->has_crowd_attrs)
            return fail(SCANN_HIP_FAILED_PRECONDITION, "no crowding attributes attached (scann_hip_index_set_crowding_attributes)");
    } else if (sg->kind == Stage::CrowdMd) {
        if (ix->crowd_md_dims == 0)
            return fail(SCANN_HIP_FAILED_PRECONDITION,
                        "no multi-attribute crowding attributes attached (scann_hip_index_set_crowding_attributes_md)");
        if (!sg->limits || sg->n_limits != ix->crowd_md_dims)
            return fail(SCANN_HIP_INVALID_ARGUMENT, "crowding: " + std::to_string(sg->n_limits) + " limits for " +
                                                        std::to_string(ix->crowd_md_dims) + " attribute dimensions");
        if ((uint64_t)ix->crowd_md_dims * std::min(k, *depth) > kCrowdMdMaxKeys)
            return fail(SCANN_HIP_UNIMPLEMENTED, "multi-attribute crowding: n_dims * k exceeds " + std::to_string(kCrowdMdMaxKeys));
    } else {
        if (std::isnan(sg->lambda)) return fail(SCANN_HIP_INVALID_ARGUMENT, "MMR: lambda is NaN");
        sg->lambda = std::min(1.0f, std::max(0.0f, sg->lambda));   // MmrDiversifier::new (crowding.rs:211-215)
        const float *rows;
        uint64_t n;
        uint32_t dim, stride;
        int measure;
        SCANN_TRY(mmr_rows(ix, &rows, &n, &dim, &stride, &measure));
        if (*depth > kMmrMaxDepth)
            return fail(SCANN_HIP_UNIMPLEMENTED, "MMR depth exceeds " + std::to_string(kMmrMaxDepth));
    }
    return SCANN_HIP_OK;
}

static int stage_depth_error(const Stage &sg) {
    return fail(SCANN_HIP_UNIMPLEMENTED, std::string(sg.name()) + " depth exceeds " + std::to_string(sg.max_depth()));
}

// The stage's kernel: [nq][depth] device rows -> [nq][k] device rows.  Enqueue only.
static int stage_launch(const scann_hip_index *ix, const Stage &sg, const uint32_t *rows_idx, const float *rows_dist,
                        const uint32_t *rows_cnt, uint32_t nq, uint32_t depth, uint32_t k, uint32_t *out_idx,
                        float *out_dist, uint32_t *out_cnt, hipStream_t st) {
    if (sg.kind == Stage::Crowd)
        return crowd_launch(rows_idx, rows_dist, rows_cnt, nq, depth, ix->crowd_attrs.as<uint64_t>(), ix->n_crowd_attrs, k,
                            sg.limit, out_idx, out_dist, out_cnt, st);
    if (sg.kind == Stage::CrowdMd)
        return crowd_md_launch(rows_idx, rows_dist, rows_cnt, nq, depth, ix->crowd_md_attrs.as<uint64_t>(),
                               ix->crowd_md_dims, ix->n_crowd_md_attrs, k, sg.limits, out_idx, out_dist, out_cnt, st);
    const float *rows;
    uint64_t n;
    uint32_t dim, stride;
    int measure;
    SCANN_TRY(mmr_rows(ix, &rows, &n, &dim, &stride, &measure));
    return mmr_launch(rows_idx, rows_dist, rows_cnt, nq, depth, rows, n, dim, stride, measure, k, sg.lambda, out_idx,
                      out_dist, out_cnt, st);
}

// The host entry point's first route: queries (and the allow bitmap) up, the enqueue-only search at k = depth into the
// slot's stage rows, the stage's kernel, the [nq][k] answer down -- the [nq][depth] rows never leave the device.
// Taken when the enqueue-only search can serve the call as the plain host entry point would: a brute-force depth
// within the index (its rows have pitch k = depth), no per-stage outputs.
static bool stage_on_device(const scann_hip_index *ix, const Stage &sg, uint32_t q_stride, uint32_t q_dim, uint32_t depth,
                            const scann_hip_search_opts *o) {
    if (depth > sg.max_depth() || q_stride < q_dim) return false;
    if (o && (o->tokens || o->token_dists || o->cand_idx || o->cand_dist || o->cand_count)) return false;
    if (ix->kind == KIND_BF) return ix->bf.n > 0 && q_dim == ix->bf.dim && depth <= ix->bf.n;
    return q_dim == ix->tx.row_dim;
}

// OK: the caller's arrays hold the answer.  Any other status: nothing was written that the second route does not
// overwrite (a status the device left -- a sampled bound that missed, a candidate buffer that overflowed -- included).
static int staged_host_on_device(scann_hip_index *ix, const Stage &sg, const float *queries, uint32_t nq, uint32_t q_stride,
                                 uint32_t k, uint32_t depth, const scann_hip_search_opts *opts, uint32_t *out_idx,
                                 float *out_dist, uint32_t *out_count) {
    SlotLock sl;
    SCANN_TRY(acquire_slot(ix, &sl));
    SCANN_TRY(set_device(ix->ctx));
    CrowdWorkspace &cw = sl.sc->crowd;
    const hipStream_t st = sl.stream;
    SCANN_TRY(cw.ensure_rows(nq, depth));
    SCANN_TRY(cw.ensure_out(nq, k));
    SCANN_TRY(cw.queries.ensure((size_t)nq * q_stride * 4));
    scann_hip_search_opts o;
    scann_hip_search_opts_default(&o);
    if (opts) o = *opts;
    SCANN_TRY(check_allow_stride(&o));
    if (o.allow_bitmap) {   // host pointer -> the slot's copy (capacity 0: a pointer no row reads)
        const size_t words = allow_copy_words(&o, nq);   // (one bitmap, or nq of them allow_bitmap_stride words apart)
        SCANN_TRY(cw.allow.ensure(std::max<size_t>(words, 1) * 8));
        if (words) SCANN_HIP_CHECK(hipMemcpyAsync(cw.allow.p, o.allow_bitmap, words * 8, hipMemcpyHostToDevice, st));
        o.allow_bitmap = cw.allow.as<uint64_t>();
    }
    SCANN_HIP_CHECK(hipMemcpyAsync(cw.queries.p, queries, (size_t)nq * q_stride * 4, hipMemcpyHostToDevice, st));
    // (the batched pipeline only: the few-query pipelines report an overflow through their polled host words)
    int s = search_device_ws(ix, nullptr, *sl.sc, TxhPipeline::Staged, cw.queries.as<float>(), nq, q_stride, depth, &o,
                             cw.idx.as<uint32_t>(), cw.dist.as<float>(), cw.cnt.as<uint32_t>(), st);
    if (s == SCANN_HIP_OK)
        s = stage_launch(ix, sg, cw.idx.as<uint32_t>(), cw.dist.as<float>(), cw.cnt.as<uint32_t>(), nq, depth, k,
                         cw.out_idx.as<uint32_t>(), cw.out_dist.as<float>(), cw.out_cnt.as<uint32_t>(), st);
    if (s != SCANN_HIP_OK) {
        (void)hipStreamSynchronize(st);   // (the uploads read the caller's memory)
        return s;
    }
    const size_t ob = (size_t)nq * k * 4;
    SCANN_HIP_CHECK(hipMemcpyAsync(out_idx, cw.out_idx.p, ob, hipMemcpyDeviceToHost, st));
    SCANN_HIP_CHECK(hipMemcpyAsync(out_dist, cw.out_dist.p, ob, hipMemcpyDeviceToHost, st));
    SCANN_HIP_CHECK(hipMemcpyAsync(out_count, cw.out_cnt.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    if (ix->kind == KIND_BF) return bf_last_status(sl.sc->bfw, st);   // (synchronises)
    uint32_t counters[CNT_N] = {};
    if (sl.sc->ws.counters.p)
        SCANN_HIP_CHECK(hipMemcpyAsync(counters, sl.sc->ws.counters.p, sizeof(counters), hipMemcpyDeviceToHost, st));
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    if (counters[CNT_STATUS] != SCANN_HIP_OK) return fail((int)counters[CNT_STATUS], "device reported a search failure");
    return SCANN_HIP_OK;
}

// Host rows [nq][depth] up, the stage's kernel, the [nq][k] answer down (k > 0, depth within the stage's maximum).
static int staged_rows_host(scann_hip_index *ix, const Stage &sg, const uint32_t *ri, const float *rd, const uint32_t *rc,
                            uint32_t nq, uint32_t depth, uint32_t k, uint32_t *out_idx, float *out_dist,
                            uint32_t *out_count) {
    SlotLock sl;
    SCANN_TRY(acquire_slot(ix, &sl));
    SCANN_TRY(set_device(ix->ctx));
    CrowdWorkspace &cw = sl.sc->crowd;
    SCANN_TRY(cw.ensure_rows(nq, depth));
    SCANN_TRY(cw.ensure_out(nq, k));
    const hipStream_t st = sl.stream;
    const size_t rb = (size_t)nq * depth * 4, ob = (size_t)nq * k * 4;
    SCANN_HIP_CHECK(hipMemcpyAsync(cw.idx.p, ri, rb, hipMemcpyHostToDevice, st));
    SCANN_HIP_CHECK(hipMemcpyAsync(cw.dist.p, rd, rb, hipMemcpyHostToDevice, st));
    SCANN_HIP_CHECK(hipMemcpyAsync(cw.cnt.p, rc, (size_t)nq * 4, hipMemcpyHostToDevice, st));
    int s = stage_launch(ix, sg, cw.idx.as<uint32_t>(), cw.dist.as<float>(), cw.cnt.as<uint32_t>(), nq, depth, k,
                         cw.out_idx.as<uint32_t>(), cw.out_dist.as<float>(), cw.out_cnt.as<uint32_t>(), st);
    if (s != SCANN_HIP_OK) {
        (void)hipStreamSynchronize(st);   // (the uploads read the caller's memory)
        return s;
    }
    SCANN_HIP_CHECK(hipMemcpyAsync(out_idx, cw.out_idx.p, ob, hipMemcpyDeviceToHost, st));
    SCANN_HIP_CHECK(hipMemcpyAsync(out_dist, cw.out_dist.p, ob, hipMemcpyDeviceToHost, st));
    SCANN_HIP_CHECK(hipMemcpyAsync(out_count, cw.out_cnt.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    return SCANN_HIP_OK;
}

static int staged_search_host(scann_hip_index *ix, Stage sg, const float *queries, uint32_t nq, uint32_t q_stride,
                              uint32_t q_dim, uint32_t k, uint32_t depth, const scann_hip_search_opts *opts,
                              uint32_t *out_idx, float *out_dist, uint32_t *out_count) {
    if (!ix) return fail(SCANN_HIP_INVALID_ARGUMENT, "index is null");
    SCANN_TRY(stage_args(ix, &sg, k, &depth));
    if (nq == 0) return SCANN_HIP_OK;
    if (!queries || !out_count || (k > 0 && (!out_idx || !out_dist)))
        return fail(SCANN_HIP_INVALID_ARGUMENT, "null query/output pointer");
    if (k > 0 && stage_on_device(ix, sg, q_stride, q_dim, depth, opts)) {
        int s = staged_host_on_device(ix, sg, queries, nq, q_stride, k, depth, opts, out_idx, out_dist, out_count);
        if (s == SCANN_HIP_OK) return s;
        // anything else (a bound that missed, a buffer that overflowed, a limit of the enqueue-only search): the route
        // below answers it, with the plain host entry point's repeats or its error
    }
    // search(query, depth): the plain host entry point, with its pipelines, filter planning and repeats
    std::vector<uint32_t> ri((size_t)nq * depth), rc(nq);
    std::vector<float> rd((size_t)nq * depth);
    SCANN_TRY(scann_hip_search_batched(ix, queries, nq, q_stride, q_dim, depth, opts, ri.data(), rd.data(), rc.data()));
    if (k == 0) {
        fill_empty(nq, 0, nullptr, nullptr, out_count);
        return SCANN_HIP_OK;
    }
    if (depth > sg.max_depth()) return stage_depth_error(sg);
    return staged_rows_host(ix, sg, ri.data(), rd.data(), rc.data(), nq, depth, k, out_idx, out_dist, out_count);
}

// The stage over the caller's own rows (host pointers): rows_count[i] <= depth; MMR: every index below it < the index size.
static int staged_apply(scann_hip_index *ix, Stage sg, const uint32_t *rows_idx, const float *rows_dist,
                        const uint32_t *rows_count, uint32_t nq, uint32_t depth, uint32_t k, uint32_t *out_idx,
                        float *out_dist, uint32_t *out_count) {
    if (!ix) return fail(SCANN_HIP_INVALID_ARGUMENT, "index is null");
    SCANN_TRY(stage_args(ix, &sg, k, &depth));
    if (nq == 0) return SCANN_HIP_OK;
    if (!rows_count || !out_count || (depth > 0 && (!rows_idx || !rows_dist)) || (k > 0 && (!out_idx || !out_dist)))
        return fail(SCANN_HIP_INVALID_ARGUMENT, "null row/output pointer");
    const uint64_t n = scann_hip_index_size(ix);
    for (uint32_t i = 0; i < nq; ++i) {
        if (rows_count[i] > depth)
            return fail(SCANN_HIP_INVALID_ARGUMENT, "rows_count[" + std::to_string(i) + "] exceeds depth");
        if (sg.kind != Stage::Mmr) continue;
        for (uint32_t j = 0; j < rows_count[i]; ++j)
            if (rows_idx[(size_t)i * depth + j] >= n)
                return fail(SCANN_HIP_INVALID_ARGUMENT, "rows_idx[" + std::to_string(i) + "][" + std::to_string(j) +
                                                            "] is not a datapoint of the index");
    }
    if (k == 0) {
        fill_empty(nq, 0, nullptr, nullptr, out_count);
        return SCANN_HIP_OK;
    }
    if (depth > sg.max_depth()) return stage_depth_error(sg);
    return staged_rows_host(ix, sg, rows_idx, rows_dist, rows_count, nq, depth, k, out_idx, out_dist, out_count);
}

static int staged_search_device(scann_hip_index *ix, Stage sg, const float *d_queries, uint32_t nq, uint32_t q_stride,
                                uint32_t k, uint32_t depth, const scann_hip_search_opts *opts, uint32_t *d_out_idx,
                                float *d_out_dist, uint32_t *d_out_count, void *hip_stream) {
    if (!ix) return fail(SCANN_HIP_INVALID_ARGUMENT, "index is null");
    if (k == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "k must be > 0 on the device path");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::lock_guard<std::mutex> lock(ix->mu);
    SCANN_TRY(stage_args(ix, &sg, k, &depth));
    if (nq == 0) return SCANN_HIP_OK;
    SCANN_TRY(set_device(ix->ctx));
    DeviceSlot *dsl = nullptr;
    SCANN_TRY(device_slot(ix, st, &dsl));
    CrowdWorkspace &cw = dsl->sc->crowd;
    if (depth > sg.max_depth()) {   // past every handle's largest k: the plain search's own error where it has one
        if (ix->kind == KIND_TXH) {
            TxhPlan p;
            SCANN_TRY(plan_txh_search(ix, depth, opts, nq, false, TxhPipeline::Wide, read_knobs(), &p));
        }
        return stage_depth_error(sg);
    }
    SCANN_TRY(cw.ensure_rows(nq, depth));   // (no allocation after scann_hip_index_reserve_crowded / _mmr)
    SCANN_TRY(search_device_ws(ix, dsl, *dsl->sc, TxhPipeline::Wide, d_queries, nq, q_stride, depth, opts,
                               cw.idx.as<uint32_t>(), cw.dist.as<float>(), cw.cnt.as<uint32_t>(), st));
    SCANN_TRY(stage_launch(ix, sg, cw.idx.as<uint32_t>(), cw.dist.as<float>(), cw.cnt.as<uint32_t>(), nq, depth, k,
                           d_out_idx, d_out_dist, d_out_count, st));
    return device_slot_done(dsl, st);
}

// scann_hip_index_reserve for k = max_depth plus the stage's rows (max_depth = 0 means max_k)
static int staged_reserve(scann_hip_index *ix, const Stage &sg, uint32_t max_nq, uint32_t max_k, uint32_t max_depth,
                          const scann_hip_search_opts *opts) {
    if (!ix) return fail(SCANN_HIP_INVALID_ARGUMENT, "index is null");
    if (max_depth == 0) max_depth = max_k;
    if (max_depth < max_k) return fail(SCANN_HIP_INVALID_ARGUMENT, std::string(sg.name()) + " depth is smaller than k");
    if (max_depth > sg.max_depth()) return stage_depth_error(sg);
    SCANN_TRY(scann_hip_index_reserve(ix, max_nq, max_depth, opts));
    std::lock_guard<std::mutex> lock(ix->mu);
    SCANN_TRY(set_device(ix->ctx));
    SCANN_TRY(ix->primary.crowd.ensure_rows(max_nq, max_depth));
    return ix->primary.crowd.ensure_out(max_nq, std::max(1u, max_k));
}

static Stage crowd_stage(uint32_t per_crowd_limit) {
    Stage sg;
    sg.kind = Stage::Crowd;
    sg.limit = per_crowd_limit;
    return sg;
}
static Stage crowd_md_stage(const uint32_t *limits, uint32_t n_limits) {
    Stage sg;
    sg.kind = Stage::CrowdMd;
    sg.limits = limits;
    sg.n_limits = n_limits;
    return sg;
}
static Stage mmr_stage(float lambda) {
    Stage sg;
    sg.kind = Stage::Mmr;
    sg.lambda = lambda;
    return sg;
}

extern "C" {

// ---- crowding (restricts/crowding.rs) --------------------------------------------------------------------------
uint32_t scann_hip_crowd_table_slots(uint32_t depth) { return crowd_table_slots(depth); }

int scann_hip_index_set_crowding_attributes(scann_hip_index *ix, const uint64_t *attrs, uint64_t n_attrs) {
    if (!ix) return fail(SCANN_HIP_INVALID_ARGUMENT, "index is null");
    if (n_attrs && !attrs) return fail(SCANN_HIP_INVALID_ARGUMENT, "attrs is null");
    std::lock_guard<std::mutex> lock(ix->mu);
    SCANN_TRY(set_device(ix->ctx));
    SCANN_HIP_CHECK(hipDeviceSynchronize());   // searches enqueued on caller streams may still read the old array
    ix->crowd_attrs.release();
    ix->n_crowd_attrs = 0;
    ix->has_crowd_attrs = false;
    if (n_attrs == 0) return SCANN_HIP_OK;
    SCANN_TRY(upload(ix->crowd_attrs, attrs, (size_t)n_attrs * 8));
    ix->n_crowd_attrs = n_attrs;
    ix->has_crowd_attrs = true;
    return SCANN_HIP_OK;
}

int scann_hip_index_set_crowding_attributes_md(scann_hip_index *ix, const uint64_t *attrs, uint32_t n_dims,
                                               uint64_t n_attrs) {
    if (!ix) return fail(SCANN_HIP_INVALID_ARGUMENT, "index is null");
    if (n_dims == 0 || n_dims > kCrowdMaxDims)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "crowding dimensions must be 1.." + std::to_string(kCrowdMaxDims));
    if (n_attrs && !attrs) return fail(SCANN_HIP_INVALID_ARGUMENT, "attrs is null");
    std::lock_guard<std::mutex> lock(ix->mu);
    SCANN_TRY(set_device(ix->ctx));
    SCANN_HIP_CHECK(hipDeviceSynchronize());   // searches enqueued on caller streams may still read the old array
    ix->crowd_md_attrs.release();
    ix->n_crowd_md_attrs = 0;
    ix->crowd_md_dims = 0;
    if (n_attrs == 0) return SCANN_HIP_OK;
    SCANN_TRY(upload(ix->crowd_md_attrs, attrs, (size_t)n_dims * n_attrs * 8));
    ix->n_crowd_md_attrs = n_attrs;
    ix->crowd_md_dims = n_dims;
    return SCANN_HIP_OK;
}

int scann_hip_search_crowded(scann_hip_index *ix, const float *queries, uint32_t nq, uint32_t q_stride,
                             uint32_t q_dim, uint32_t k, uint32_t depth, uint32_t per_crowd_limit,
                             const scann_hip_search_opts *opts, uint32_t *out_idx, float *out_dist,
                             uint32_t *out_count) {
    return staged_search_host(ix, crowd_stage(per_crowd_limit), queries, nq, q_stride, q_dim, k, depth, opts, out_idx,
                              out_dist, out_count);
}

int scann_hip_index_reserve_crowded(scann_hip_index *ix, uint32_t max_nq, uint32_t max_k, uint32_t max_depth,
                                    const scann_hip_search_opts *opts) {
    return staged_reserve(ix, crowd_stage(0), max_nq, max_k, max_depth, opts);
}

int scann_hip_search_crowded_device(scann_hip_index *ix, const float *d_queries, uint32_t nq, uint32_t q_stride,
                                    uint32_t k, uint32_t depth, uint32_t per_crowd_limit,
                                    const scann_hip_search_opts *opts, uint32_t *d_out_idx, float *d_out_dist,
                                    uint32_t *d_out_count, void *hip_stream) {
    return staged_search_device(ix, crowd_stage(per_crowd_limit), d_queries, nq, q_stride, k, depth, opts, d_out_idx,
                                d_out_dist, d_out_count, hip_stream);
}

int scann_hip_search_crowded_md(scann_hip_index *ix, const float *queries, uint32_t nq, uint32_t q_stride, uint32_t q_dim,
                                uint32_t k, uint32_t depth, const uint32_t *limits, uint32_t n_limits,
                                const scann_hip_search_opts *opts, uint32_t *out_idx, float *out_dist,
                                uint32_t *out_count) {
    return staged_search_host(ix, crowd_md_stage(limits, n_limits), queries, nq, q_stride, q_dim, k, depth, opts, out_idx,
                              out_dist, out_count);
}

int scann_hip_search_crowded_md_device(scann_hip_index *ix, const float *d_queries, uint32_t nq, uint32_t q_stride,
                                       uint32_t k, uint32_t depth, const uint32_t *limits, uint32_t n_limits,
                                       const scann_hip_search_opts *opts, uint32_t *d_out_idx, float *d_out_dist,
                                       uint32_t *d_out_count, void *hip_stream) {
    return staged_search_device(ix, crowd_md_stage(limits, n_limits), d_queries, nq, q_stride, k, depth, opts, d_out_idx,
                                d_out_dist, d_out_count, hip_stream);
}

int scann_hip_crowd_md_apply(scann_hip_index *ix, const uint32_t *rows_idx, const float *rows_dist,
                             const uint32_t *rows_count, uint32_t nq, uint32_t depth, uint32_t k, const uint32_t *limits,
                             uint32_t n_limits, uint32_t *out_idx, float *out_dist, uint32_t *out_count) {
    return staged_apply(ix, crowd_md_stage(limits, n_limits), rows_idx, rows_dist, rows_count, nq, depth, k, out_idx,
                        out_dist, out_count);
}

int scann_hip_search_mmr(scann_hip_index *ix, const float *queries, uint32_t nq, uint32_t q_stride, uint32_t q_dim,
                         uint32_t k, uint32_t depth, float lambda, const scann_hip_search_opts *opts, uint32_t *out_idx,
                         float *out_dist, uint32_t *out_count) {
    return staged_search_host(ix, mmr_stage(lambda), queries, nq, q_stride, q_dim, k, depth, opts, out_idx, out_dist,
                              out_count);
}

int scann_hip_search_mmr_device(scann_hip_index *ix, const float *d_queries, uint32_t nq, uint32_t q_stride, uint32_t k,
                                uint32_t depth, float lambda, const scann_hip_search_opts *opts, uint32_t *d_out_idx,
                                float *d_out_dist, uint32_t *d_out_count, void *hip_stream) {
    return staged_search_device(ix, mmr_stage(lambda), d_queries, nq, q_stride, k, depth, opts, d_out_idx, d_out_dist,
                                d_out_count, hip_stream);
}

int scann_hip_index_reserve_mmr(scann_hip_index *ix, uint32_t max_nq, uint32_t max_k, uint32_t max_depth,
                                const scann_hip_search_opts *opts) {
    return staged_reserve(ix, mmr_stage(0.0f), max_nq, max_k, max_depth, opts);
}

int scann_hip_mmr_apply(scann_hip_index *ix, const uint32_t *rows_idx, const float *rows_dist, const uint32_t *rows_count,
                        uint32_t nq, uint32_t depth, uint32_t k, float lambda, uint32_t *out_idx, float *out_dist,
                        uint32_t *out_count) {
    return staged_apply(ix, mmr_stage(lambda), rows_idx, rows_dist, rows_count, nq, depth, k, out_idx, out_dist, out_count);
}

}  // extern "C"

// api.hip -- C ABI of libscann_hip.so (include/scann_hip.h): the last error, contexts, the lifetime of an index handle
// and what other sources read of it (index_base_view, index_fold_view, index_download), and the stateless building
// blocks.  Handles are created in api_create.hip, searched in api_search.hip and api_stages.hip (handle.h).  No CPU
// compute fallback exists: every search entry point runs the HIP kernels or fails.
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "allow.h"
#include "comm.h"
#include "handle.h"
#include "index_arrays.h"
#include "launch.h"
#include "mutable.h"

namespace scann {

static thread_local std::string g_last_error;
void set_last_error(const std::string &msg) { g_last_error = msg; }
int fail(int status, const std::string &msg) {
    g_last_error = msg;
    return status;
}

}  // namespace scann

using namespace scann;

int scann::set_device(const scann_hip_ctx *ctx) {
    SCANN_HIP_CHECK(hipSetDevice(ctx->device));
    return SCANN_HIP_OK;
}

int scann::ctx_device(const scann_hip_ctx *ctx) { return ctx ? ctx->device : 0; }

// What mutable.hip needs to know of a base handle (mutable.h): its f32 rows by datapoint index and the measure of
// its final distances.
int scann::index_base_view(const scann_hip_index *ix, BaseView *v) {
    if (!ix || !v) return fail(SCANN_HIP_INVALID_ARGUMENT, "index is null");
    *v = BaseView();
    v->ctx = ix->ctx;
    v->brute_force = ix->kind == KIND_BF;
    if (ix->kind == KIND_BF) {
        v->rows = ix->bf.rows;
        v->n = ix->bf.n;
        v->dim = ix->bf.dim;
        v->stride = ix->bf.stride;
        v->measure = ix->bf.measure;
        v->quantized = ix->bf.fmt != 0;
    } else {
        v->rows = ix->tx.rows;
        v->quantized = ix->tx.qfmt != 0;
        v->projected = ix->proj.kind != 0;
        v->n = ix->tx.n_local;
        v->dim = ix->tx.dim;
        v->stride = ix->tx.stride;
        v->measure = ix->tx.measure;
        v->rows_csr = ix->tx.rows_csr != 0 && !ix->tx.ah_mode;   // (the flat hasher's one leaf is in datapoint order)
        v->partitioned = ix->tx.exact_scan != 0;
        v->sharded = ix->sharded;
    }
    return SCANN_HIP_OK;
}

int scann::index_fold_view(const scann_hip_index *ix, FoldView *v) {
    if (!ix || !v || ix->kind != KIND_TXH) return fail(SCANN_HIP_INVALID_ARGUMENT, "not a tree / hasher index");
    const TxhIndexDev &t = ix->tx;
    *v = FoldView();
    v->L = t.L; v->S = t.S; v->K = t.K; v->dsub = t.dsub; v->nw = t.nw;
    v->ah = t.ah_mode; v->use_residuals = t.use_residuals;
    v->n_local = t.n_local; v->n_rows = ix->n_rows;
    v->leaf_off = t.leaf_off; v->leaf_ids = t.leaf_ids; v->codes = t.codes;
    v->centers = t.centers; v->codebook = t.codebook;
    return SCANN_HIP_OK;
}

void scann::txh_desc_of(const scann_hip_index *ix, scann_hip_txh_desc *d) {
    const TxhIndexDev &t = ix->tx;
    std::memset(d, 0, sizeof(*d));
    d->n_rows = ix->n_rows;
    d->n_local = t.n_local;
    d->dim = t.dim;
    d->stride = t.stride;
    d->num_partitions = t.ah_mode ? 0u : t.L;
    d->num_subspaces = t.S;
    d->num_codes = t.exact_scan ? 0u : t.K;
    d->dims_per_subspace = t.dsub;
    d->distance_measure = t.measure;
    d->data_is_csr_order = (t.rows_csr && !t.ah_mode) ? 1 : 0;
    d->codes_packed4 = (!t.exact_scan && t.code_bits == 4) ? 1 : 0;
    d->use_residuals = t.use_residuals;
    d->partitions_to_search = t.ah_mode ? 0u : ix->default_P;
    d->pre_reorder_multiplier = ix->multiplier;
}

int scann::index_download(const scann_hip_index *ix, IndexHostArrays *o, bool with_rows) {
    if (!ix || !o) return fail(SCANN_HIP_INVALID_ARGUMENT, "index is null");
    SCANN_TRY(set_device(ix->ctx));
    auto down = [](auto &vec, const void *src, size_t count) -> int {
        vec.resize(count);
        if (count) SCANN_HIP_CHECK(hipMemcpy(vec.data(), src, count * sizeof(vec[0]), hipMemcpyDeviceToHost));
        return SCANN_HIP_OK;
    };
    scann_hip_txh_desc &d = o->d;
    if (ix->kind == KIND_BF) {
        if (ix->bf.fmt) return fail(SCANN_HIP_UNIMPLEMENTED, "index_write_file: quantized brute-force rows are not written");
        o->brute_force = true;
        std::memset(&d, 0, sizeof(d));
        d.n_rows = d.n_local = ix->bf.n;
        d.dim = ix->bf.dim;
        d.stride = ix->bf.stride;
        d.distance_measure = ix->bf.measure;
        SCANN_TRY(down(o->data, ix->bf.rows, (size_t)ix->bf.n * ix->bf.stride));
        d.data = o->data.data();
        return SCANN_HIP_OK;
    }
    if (ix->sharded) return fail(SCANN_HIP_UNIMPLEMENTED, "index_write_file: shards (leaf_sizes_global) are not written");
    const TxhIndexDev &t = ix->tx;
    o->brute_force = false;
    txh_desc_of(ix, &d);
    if (ix->proj.kind) {   // the projection, and the rows in their own space (d.data stays null: d is the index space)
        const ProjDev &pd = ix->proj;
        const uint32_t meta[5] = {(uint32_t)pd.kind, pd.in_dim, pd.out_dim, pd.start, t.row_stride};
        std::memcpy(o->proj_meta, meta, sizeof(meta));
        if (pd.matrix) SCANN_TRY(down(o->proj_matrix, pd.matrix, (size_t)pd.out_dim * pd.in_dim));
        if (pd.mean) SCANN_TRY(down(o->proj_mean, pd.mean, (size_t)pd.in_dim));
        if (t.rows && with_rows) SCANN_TRY(down(o->data, t.rows, (size_t)ix->n_rows * t.row_stride));
    } else if (t.rows && with_rows) {
        SCANN_TRY(down(o->data, t.rows, (size_t)ix->n_rows * t.stride));
        d.data = o->data.data();
    }
    if (!t.ah_mode) {
        SCANN_TRY(down(o->centers, t.centers, (size_t)t.L * t.dim));
        SCANN_TRY(down(o->leaf_offsets, t.leaf_off, (size_t)t.L + 1));
        SCANN_TRY(down(o->leaf_ids, t.leaf_ids, (size_t)t.n_local));
        d.centers = o->centers.data();
        d.leaf_offsets = o->leaf_offsets.data();
        d.leaf_ids = o->leaf_ids.data();
    }
    if (t.qrows && with_rows) {
        o->rows_q.resize((size_t)ix->n_rows * t.stride * (t.qfmt == SCANN_HIP_ROWS_BF16 ? 2 : 1));
        if (!o->rows_q.empty())
            SCANN_HIP_CHECK(hipMemcpy(o->rows_q.data(), t.qrows, o->rows_q.size(), hipMemcpyDeviceToHost));
        o->rows_q_fmt = t.qfmt;
        o->rows_q_inv = t.inv_mult;
    }
    if (!t.rows && !t.qrows) {   // a handle created without rows keeps no row count: the smallest that holds every datapoint index
        d.n_rows = t.n_local;
        for (uint32_t id : o->leaf_ids) d.n_rows = std::max<uint64_t>(d.n_rows, (uint64_t)id + 1);
    }
    if (!t.exact_scan) {
        SCANN_TRY(down(o->codebook, t.codebook, (size_t)t.S * t.K * t.dsub));
        SCANN_TRY(down(o->codes, t.codes, (size_t)t.n_local * t.nw));
        d.codebook = o->codebook.data();
        d.codes = reinterpret_cast<const uint8_t *>(o->codes.data());   // little-endian words == the file's byte layout
    }
    return SCANN_HIP_OK;
}

static int kmeans_args(scann_hip_index *ix, uint32_t col_offset, uint32_t sub_dim, uint32_t k, const void *c) {
    if (!ix || ix->kind != KIND_BF) return fail(SCANN_HIP_INVALID_ARGUMENT, "not a brute-force index");
    if (ix->bf.fmt) return fail(SCANN_HIP_INVALID_ARGUMENT, "the index holds quantized rows, not f32 rows");
    if (ix->bf.n == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "Cannot cluster empty dataset");   // kmeans.rs:167-169
    if (!c || k == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "null centres / zero clusters");
    if (sub_dim == 0 || (uint64_t)col_offset + sub_dim > ix->bf.dim)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "column window outside the rows");
    return SCANN_HIP_OK;
}

extern "C" {

const char *scann_hip_last_error(void) { return g_last_error.c_str(); }
const char *scann_hip_version(void) { return "scann_hip 0.1.0 (gfx950)"; }

uint32_t scann_hip_abi_layout(uint32_t *out, uint32_t n) {
    const uint32_t v[10] = {(uint32_t)sizeof(scann_hip_txh_desc), (uint32_t)offsetof(scann_hip_txh_desc, distance_measure),
                            (uint32_t)sizeof(scann_hip_search_opts), (uint32_t)offsetof(scann_hip_search_opts, bf_exact),
                            (uint32_t)sizeof(scann_hip_file_info), (uint32_t)offsetof(scann_hip_file_info, has_data),
                            (uint32_t)sizeof(scann_hip_build_config), (uint32_t)offsetof(scann_hip_build_config, distance_measure),
                            (uint32_t)sizeof(scann_hip_build_report), (uint32_t)offsetof(scann_hip_build_report, stage_ms)};
    for (uint32_t i = 0; i < 10 && i < n && out; ++i) out[i] = v[i];
    return 10;
}

uint32_t scann_hip_compute_stride(uint32_t dim) {
    const uint32_t per_line = 64 / sizeof(float);  // data_format/dataset.rs:90-96
    return (dim + per_line - 1) / per_line * per_line;
}

int scann_hip_init(int device_id, scann_hip_ctx **out_ctx) {
    if (!out_ctx) return fail(SCANN_HIP_INVALID_ARGUMENT, "out_ctx is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(SCANN_HIP_UNAVAILABLE,
                    "no HIP device available (libscann_hip has no CPU fallback)");
    if (device_id < 0 || device_id >= n)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "device_id out of range");
    SCANN_HIP_CHECK(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    SCANN_HIP_CHECK(hipGetDeviceProperties(&prop, device_id));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(SCANN_HIP_FAILED_PRECONDITION,
                    std::string("libscann_hip is built for gfx950 only; device is ") +
                        prop.gcnArchName);
    auto *c = new scann_hip_ctx();
    c->device = device_id;
    c->num_cus = prop.multiProcessorCount;
    *out_ctx = c;
    return SCANN_HIP_OK;
}

void scann_hip_shutdown(scann_hip_ctx *ctx) { delete ctx; }

void scann_hip_search_opts_default(scann_hip_search_opts *o) {
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->exact_reorder = 1;
}

void scann_hip_index_destroy(scann_hip_index *ix) {
    if (!ix) return;
    (void)hipSetDevice(ix->ctx->device);
    if (ix->stream) (void)hipStreamSynchronize(ix->stream);
    for (int i = 0; i < scann_hip_index::kEvRing; ++i) {
        if (ix->evs[i][0]) (void)hipEventDestroy(ix->evs[i][0]);
        if (ix->evs[i][1]) (void)hipEventDestroy(ix->evs[i][1]);
    }
    if (ix->stream) (void)hipStreamDestroy(ix->stream);
    (void)hipDeviceSynchronize();   // device entry points enqueue on caller streams
    for (auto &ds : ix->dslots)
        if (ds.done) (void)hipEventDestroy(ds.done);
    for (auto &sl : ix->slots)
        if (sl->stream) {
            (void)hipStreamSynchronize(sl->stream);
            (void)hipStreamDestroy(sl->stream);
        }
    delete ix;
}

uint64_t scann_hip_index_size(const scann_hip_index *ix) {
    if (!ix) return 0;
    return ix->kind == KIND_BF ? ix->bf.n : ix->tx.n_local;
}
uint32_t scann_hip_index_dimensionality(const scann_hip_index *ix) {
    if (!ix) return 0;
    return ix->kind == KIND_BF ? ix->bf.dim : ix->tx.row_dim;   // (projected handles: the rows' space)
}

void scann_hip_index_enable_timing(scann_hip_index *ix, int enable) {
    if (!ix) return;
    ix->timing = enable != 0;
    ix->ev_n = 0;
    ix->timing_valid = false;
}

float scann_hip_index_last_kernel_ms(scann_hip_index *ix, const char **name) {
    if (name) *name = ix ? ix->timed_kernel : "";
    if (!ix || !ix->timing_valid || ix->ev_n == 0) return 0.0f;
    const uint32_t cnt = ix->ev_n < (uint32_t)scann_hip_index::kEvRing
                             ? ix->ev_n : (uint32_t)scann_hip_index::kEvRing;
    double sum = 0.0;
    uint32_t ok = 0;
    for (uint32_t i = 0; i < cnt; ++i) {   // mean over the recorded launches
        float ms = 0.0f;
        // a pair handed to a call that failed before recording it (k > kBfMaxK, say) has no time: skip it and
        // clear the error the query leaves behind, or the next search's launch check reports it as its own
        if (hipEventSynchronize(ix->evs[i][1]) != hipSuccess ||
            hipEventElapsedTime(&ms, ix->evs[i][0], ix->evs[i][1]) != hipSuccess) {
            clear_last_hip_error();
            continue;
        }
        sum += ms;
        ++ok;
    }
    return ok ? (float)(sum / ok) : 0.0f;
}

int scann_hip_bf16_quantize(scann_hip_ctx *ctx, const float *values, uint64_t n, uint16_t *out_bits) {
    if (!ctx) return fail(SCANN_HIP_INVALID_ARGUMENT, "ctx is null");
    if (n == 0) return SCANN_HIP_OK;
    if (!values || !out_bits) return fail(SCANN_HIP_INVALID_ARGUMENT, "null values/output");
    SCANN_TRY(set_device(ctx));
    return bf16_quantize_host(values, n, out_bits, nullptr);
}

uint64_t scann_hip_index_device_bytes(const scann_hip_index *ix) {
    if (!ix) return 0;
    uint64_t sum = 0;
    for (const DevBuf *b : {&ix->bf_rows, &ix->bf_rows_b, &ix->bf_rows_bl, &ix->bf_norm2, &ix->bf_leaf, &ix->d_centers,
                            &ix->d_centers_t, &ix->d_leaf_off, &ix->d_leaf_gsize, &ix->d_leaf_ids, &ix->d_codes,
                            &ix->d_codes_sp, &ix->d_rows, &ix->d_codebook, &ix->d_rows8, &ix->d_rows8_meta, &ix->d_qrows,
                            &ix->crowd_attrs, &ix->crowd_md_attrs, &ix->d_proj_matrix, &ix->d_proj_mean})
        if (b->p) sum += b->bytes;
    return sum;
}

int scann_hip_txh_merge_device(scann_hip_ctx *ctx, uint32_t world, uint32_t nq, uint32_t m_local,
                               uint32_t m, uint32_t k, uint64_t rank_stride_bytes,
                               const uint64_t *d_keys, const uint32_t *d_idx,
                               const float *d_exact, const uint32_t *d_count, uint32_t *d_out_idx,
                               float *d_out_dist, uint32_t *d_out_count, uint32_t *d_status,
                               void *hip_stream) {
    if (!ctx) return fail(SCANN_HIP_INVALID_ARGUMENT, "ctx is null");
    SCANN_TRY(set_device(ctx));
    return txh_launch_merge(world, nq, m_local, m, k, (size_t)rank_stride_bytes, d_keys, d_idx, d_exact,
                            d_count, d_out_idx,
                            d_out_dist, d_out_count, d_status, static_cast<hipStream_t>(hip_stream));
}

int scann_hip_txh_pack_blocks_device(scann_hip_ctx *ctx, uint32_t world, uint32_t nq, uint32_t m_local,
                                     const uint64_t *d_keys, const uint32_t *d_idx, const float *d_exact,
                                     const uint32_t *d_count, void *d_out, uint64_t block_bytes,
                                     void *hip_stream) {
    if (!ctx) return fail(SCANN_HIP_INVALID_ARGUMENT, "ctx is null");
    if (!d_keys || !d_idx || !d_exact || !d_count || !d_out)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "null buffer");
    SCANN_TRY(set_device(ctx));
    return txh_launch_pack_blocks(world, nq, m_local, d_keys, d_idx, d_exact, d_count, d_out,
                                  (size_t)block_bytes, static_cast<hipStream_t>(hip_stream));
}

int scann_hip_assign_leaves(const uint32_t *sizes, uint32_t L, uint32_t world, uint32_t *owner) {
    if (!sizes || !owner || world == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "bad arguments");
    std::vector<uint32_t> order(L);
    for (uint32_t i = 0; i < L; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return sizes[a] > sizes[b]; });
    std::vector<uint64_t> load(world, 0);
    for (uint32_t i : order) {
        uint32_t best = 0;
        for (uint32_t g = 1; g < world; ++g)
            if (load[g] < load[best]) best = g;
        owner[i] = best;
        load[best] += sizes[i];
    }
    return SCANN_HIP_OK;
}

// ---- building blocks ---------------------------------------------------------------------

int scann_hip_lut_from_query(scann_hip_index *ix, const float *queries, uint32_t nq,
                             uint32_t q_stride, const uint32_t *leaf_for_query, float *out_lut) {
    if (!ix || ix->kind != KIND_TXH) return fail(SCANN_HIP_INVALID_ARGUMENT, "not a tree index");
    if (nq == 0) return SCANN_HIP_OK;
    if (leaf_for_query && ix->tx.ah_mode)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "no centroids in AsymmetricHasher mode");
    if (leaf_for_query)
        for (uint32_t i = 0; i < nq; ++i)
            if (leaf_for_query[i] >= ix->tx.L)  // mod.rs:304-306
                return fail(SCANN_HIP_OUT_OF_RANGE, "Invalid partition ID");
    std::lock_guard<std::mutex> lock(ix->mu);
    SCANN_TRY(set_device(ix->ctx));
    DevBuf dq, dl, dout;
    SCANN_TRY(upload(dq, queries, (size_t)nq * q_stride * 4));
    if (leaf_for_query) SCANN_TRY(upload(dl, leaf_for_query, (size_t)nq * 4));
    const size_t ob = (size_t)nq * ix->tx.S * ix->tx.K * 4;
    SCANN_TRY(dout.ensure(ob));
    SCANN_TRY(txh_launch_lut_from_query(ix->tx, dq.as<float>(), nq, q_stride,
                                        leaf_for_query ? dl.as<uint32_t>() : nullptr,
                                        dout.as<float>(), ix->stream));
    SCANN_HIP_CHECK(hipMemcpyAsync(out_lut, dout.p, ob, hipMemcpyDeviceToHost, ix->stream));
    SCANN_HIP_CHECK(hipStreamSynchronize(ix->stream));
    return SCANN_HIP_OK;
}

int scann_hip_adc_distances(scann_hip_index *ix, const float *luts, uint32_t nq, float *out_dist) {
    if (!ix || ix->kind != KIND_TXH) return fail(SCANN_HIP_INVALID_ARGUMENT, "not a tree index");
    if (nq == 0) return SCANN_HIP_OK;
    std::lock_guard<std::mutex> lock(ix->mu);
    SCANN_TRY(set_device(ix->ctx));
    DevBuf dl, dout;
    SCANN_TRY(upload(dl, luts, (size_t)nq * ix->tx.S * ix->tx.K * 4));
    const size_t ob = (size_t)nq * ix->tx.n_local * 4;
    SCANN_TRY(dout.ensure(ob));
    SCANN_TRY(txh_launch_adc_distances(ix->tx, dl.as<float>(), nq, dout.as<float>(), ix->stream));
    SCANN_HIP_CHECK(hipMemcpyAsync(out_dist, dout.p, ob, hipMemcpyDeviceToHost, ix->stream));
    SCANN_HIP_CHECK(hipStreamSynchronize(ix->stream));
    return SCANN_HIP_OK;
}

int scann_hip_lut16_distances_batch(scann_hip_ctx *ctx, const uint8_t *packed, const uint8_t *lut8,
                                    uint32_t S, uint64_t n, float bias, float multiplier,
                                    float *out) {
    if (!ctx) return fail(SCANN_HIP_INVALID_ARGUMENT, "ctx is null");
    if (n == 0) return SCANN_HIP_OK;
    if (!packed || !lut8 || !out || S == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "null argument");
    SCANN_TRY(set_device(ctx));
    DevBuf dp, dl, dout;
    SCANN_TRY(upload(dp, packed, (size_t)n * ((S + 1) / 2)));
    SCANN_TRY(upload(dl, lut8, (size_t)S * 16));
    SCANN_TRY(dout.ensure((size_t)n * 4));
    SCANN_TRY(launch_lut16_u8_batch(dp.as<uint8_t>(), dl.as<uint8_t>(), S, n, bias, multiplier,
                                    dout.as<float>(), nullptr));
    SCANN_HIP_CHECK(hipMemcpy(out, dout.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return SCANN_HIP_OK;
}

int scann_hip_lut16_quantize(scann_hip_ctx *ctx, const float *tables, uint32_t S, uint8_t *out_lut8,
                             float *out_bias, float *out_multiplier) {
    if (!ctx) return fail(SCANN_HIP_INVALID_ARGUMENT, "ctx is null");
    if (!out_bias || !out_multiplier) return fail(SCANN_HIP_INVALID_ARGUMENT, "null bias/multiplier");
    if (S == 0) {   // lut16_simd.rs:42-49
        *out_bias = 0.0f;
        *out_multiplier = 1.0f;
        return SCANN_HIP_OK;
    }
    if (!tables || !out_lut8) return fail(SCANN_HIP_INVALID_ARGUMENT, "null tables/output");
    SCANN_TRY(set_device(ctx));
    DevBuf dt, dq, dp;
    SCANN_TRY(upload(dt, tables, (size_t)S * 16 * 4));
    SCANN_TRY(dq.ensure((size_t)S * 16));
    SCANN_TRY(dp.ensure(8));
    SCANN_TRY(launch_lut16_quantize(dt.as<float>(), S, dq.as<uint8_t>(), dp.as<float>(), nullptr));
    float bm[2];
    SCANN_HIP_CHECK(hipMemcpy(out_lut8, dq.p, (size_t)S * 16, hipMemcpyDeviceToHost));
    SCANN_HIP_CHECK(hipMemcpy(bm, dp.p, 8, hipMemcpyDeviceToHost));
    *out_bias = bm[0];
    *out_multiplier = bm[1];
    return SCANN_HIP_OK;
}

int scann_hip_fp8_quantize(scann_hip_ctx *ctx, const float *values, uint64_t n, float scale, int format,
                           uint8_t *out_bits) {
    if (!ctx) return fail(SCANN_HIP_INVALID_ARGUMENT, "ctx is null");
    if (format != SCANN_HIP_FP8_E4M3 && format != SCANN_HIP_FP8_E5M2) return fail(SCANN_HIP_INVALID_ARGUMENT, "unknown FP8 format");
    if (n == 0) return SCANN_HIP_OK;
    if (!values || !out_bits) return fail(SCANN_HIP_INVALID_ARGUMENT, "null values/output");
    SCANN_TRY(set_device(ctx));
    DevBuf dv, dout;
    SCANN_TRY(upload(dv, values, (size_t)n * 4));
    SCANN_TRY(dout.ensure((size_t)n));
    SCANN_TRY(launch_fp8_quantize(dv.as<float>(), n, scale, format, dout.as<uint8_t>(), nullptr));
    SCANN_HIP_CHECK(hipMemcpy(out_bits, dout.p, (size_t)n, hipMemcpyDeviceToHost));
    return SCANN_HIP_OK;
}

int scann_hip_fp8_dequantize(scann_hip_ctx *ctx, const uint8_t *bits, uint64_t n, float scale, int format,
                             float *out_values) {
    if (!ctx) return fail(SCANN_HIP_INVALID_ARGUMENT, "ctx is null");
    if (format != SCANN_HIP_FP8_E4M3 && format != SCANN_HIP_FP8_E5M2) return fail(SCANN_HIP_INVALID_ARGUMENT, "unknown FP8 format");
    if (n == 0) return SCANN_HIP_OK;
    if (!bits || !out_values) return fail(SCANN_HIP_INVALID_ARGUMENT, "null bits/output");
    SCANN_TRY(set_device(ctx));
    DevBuf db, dout;
    SCANN_TRY(upload(db, bits, (size_t)n));
    SCANN_TRY(dout.ensure((size_t)n * 4));
    SCANN_TRY(launch_fp8_dequantize(db.as<uint8_t>(), n, scale, format, dout.as<float>(), nullptr));
    SCANN_HIP_CHECK(hipMemcpy(out_values, dout.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return SCANN_HIP_OK;
}

int scann_hip_fp8_distances(scann_hip_ctx *ctx, const float *query, uint32_t dim, const uint8_t *database,
                            uint64_t stride, uint64_t num_points, int measure, float *out_distances) {
    if (!ctx) return fail(SCANN_HIP_INVALID_ARGUMENT, "ctx is null");
    if (measure != SCANN_HIP_SQUARED_L2 && measure != SCANN_HIP_DOT_PRODUCT)
        return fail(SCANN_HIP_UNIMPLEMENTED, "the reference's FP8 kernels are squared L2 and dot product");
    if (num_points == 0) return SCANN_HIP_OK;
    if (!query || !database || !out_distances || dim == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "bad argument");
    if (stride < dim) return fail(SCANN_HIP_INVALID_ARGUMENT, "stride < dim");
    if (dim > 32768) return fail(SCANN_HIP_RESOURCE_EXHAUSTED, "dim > 32768");
    SCANN_TRY(set_device(ctx));
    DevBuf dq, ddb, dout;
    SCANN_TRY(upload(dq, query, (size_t)dim * 4));
    SCANN_TRY(upload(ddb, database, (size_t)num_points * stride));
    SCANN_TRY(dout.ensure((size_t)num_points * 4));
    SCANN_TRY(launch_fp8_one_to_many(dq.as<float>(), dim, ddb.as<uint8_t>(), stride, num_points,
                                     measure == SCANN_HIP_DOT_PRODUCT ? 1 : 0, dout.as<float>(), nullptr));
    SCANN_HIP_CHECK(hipMemcpy(out_distances, dout.p, (size_t)num_points * 4, hipMemcpyDeviceToHost));
    return SCANN_HIP_OK;
}

int scann_hip_encode(scann_hip_ctx *ctx, const float *codebook, uint32_t S, uint32_t K, uint32_t dsub,
                     const float *rows, uint64_t n, uint32_t stride, const float *centers,
                     const uint32_t *leaf_of_row, uint8_t *out_codes) {
    if (!ctx) return fail(SCANN_HIP_INVALID_ARGUMENT, "ctx is null");
    if (n == 0) return SCANN_HIP_OK;
    if (!codebook || !rows || !out_codes || S == 0 || K == 0 || K > 256 || dsub == 0)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "bad argument");
    if ((centers == nullptr) != (leaf_of_row == nullptr))
        return fail(SCANN_HIP_INVALID_ARGUMENT, "centers and leaf_of_row go together");
    if (stride < S * dsub) return fail(SCANN_HIP_INVALID_ARGUMENT, "stride < dim");
    SCANN_TRY(set_device(ctx));
    DevBuf dcb, drows, dcen, dleaf, dout;
    SCANN_TRY(upload(dcb, codebook, (size_t)S * K * dsub * 4));
    SCANN_TRY(upload(drows, rows, (size_t)n * stride * 4));
    if (centers) {
        uint32_t maxleaf = 0;
        for (uint64_t i = 0; i < n; ++i) maxleaf = std::max(maxleaf, leaf_of_row[i]);
        SCANN_TRY(upload(dcen, centers, (size_t)(maxleaf + 1) * S * dsub * 4));
        SCANN_TRY(upload(dleaf, leaf_of_row, (size_t)n * 4));
    }
    SCANN_TRY(dout.ensure((size_t)n * S));
    SCANN_TRY(launch_encode(dcb.as<float>(), S, K, dsub, drows.as<float>(), n, stride,
                            centers ? dcen.as<float>() : nullptr,
                            centers ? dleaf.as<uint32_t>() : nullptr, dout.as<uint8_t>(), nullptr));
    SCANN_HIP_CHECK(hipMemcpy(out_codes, dout.p, (size_t)n * S, hipMemcpyDeviceToHost));
    return SCANN_HIP_OK;
}

int scann_hip_bf_distances(scann_hip_index *ix, const float *queries, uint32_t nq, uint32_t q_stride,
                           float *out) {
    if (!ix || ix->kind != KIND_BF) return fail(SCANN_HIP_INVALID_ARGUMENT, "not a brute-force index");
    if (nq == 0 || ix->bf.n == 0) return SCANN_HIP_OK;
    std::lock_guard<std::mutex> lock(ix->mu);
    SCANN_TRY(set_device(ix->ctx));
    SCANN_TRY(claim_primary_workspace(ix));
    return bf_distances_host(ix->bf, ix->primary.bfw, queries, nq, q_stride, out, ix->stream);
}

int scann_hip_bf_search_radius(scann_hip_index *ix, const float *query, uint32_t q_dim, float radius,
                               uint32_t *out_idx, float *out_dist, uint64_t capacity,
                               uint64_t *out_count) {
    return scann_hip_bf_search_radius_opts(ix, query, q_dim, radius, nullptr, out_idx, out_dist, capacity, out_count);
}

uint64_t scann_hip_allow_bitmap_count(const uint64_t *allow_bitmap, uint64_t allow_bitmap_bits, uint64_t n) {
    return allow_bitmap ? bf_allowed_count(allow_bitmap, allow_bitmap_bits, n) : 0;
}

int scann_hip_bf_search_radius_opts(scann_hip_index *ix, const float *query, uint32_t q_dim, float radius,
                                    const scann_hip_search_opts *opts, uint32_t *out_idx, float *out_dist,
                                    uint64_t capacity, uint64_t *out_count) {
    if (!ix || ix->kind != KIND_BF) return fail(SCANN_HIP_INVALID_ARGUMENT, "not a brute-force index");
    if (!out_count) return fail(SCANN_HIP_INVALID_ARGUMENT, "null out_count");
    *out_count = 0;
    SCANN_TRY(refuse_allow_stride(opts, "radius search"));
    if (ix->bf.n == 0) return SCANN_HIP_OK;   // searcher.rs:143-145
    if (!query || q_dim != ix->bf.dim)        // searcher.rs:148-152
        return fail(SCANN_HIP_INVALID_ARGUMENT, "Query dimensionality does not match dataset");
    if (capacity && (!out_idx || !out_dist)) return fail(SCANN_HIP_INVALID_ARGUMENT, "null outputs");
    std::lock_guard<std::mutex> lock(ix->mu);
    SCANN_TRY(set_device(ix->ctx));
    SCANN_TRY(claim_primary_workspace(ix));
    return bf_search_radius_host(ix->bf, ix->primary.bfw, query, q_dim, radius, bf_filter_of(opts, read_knobs()), out_idx,
                                 out_dist, capacity, out_count, ix->stream);
}

int scann_hip_bf_assign_nearest(scann_hip_index *ix, const float *centers, uint32_t num_centers,
                                uint32_t *out_assign, float *out_dist) {
    if (!ix || ix->kind != KIND_BF) return fail(SCANN_HIP_INVALID_ARGUMENT, "not a brute-force index");
    if (ix->bf.fmt) return fail(SCANN_HIP_INVALID_ARGUMENT, "the index holds quantized rows, not f32 rows");
    if (!centers || num_centers == 0 || !out_assign)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "null/empty centres or output");
    std::lock_guard<std::mutex> lock(ix->mu);
    SCANN_TRY(set_device(ix->ctx));
    return bf_assign_nearest_host(ix->bf, centers, num_centers, out_assign, out_dist, ix->stream);
}

int scann_hip_kmeans_init_pp(scann_hip_index *ix, uint32_t col_offset, uint32_t sub_dim, uint32_t k,
                             uint64_t seed, uint32_t simd_threshold, float *centers_out) {
    SCANN_TRY(kmeans_args(ix, col_offset, sub_dim, k, centers_out));
    std::lock_guard<std::mutex> lock(ix->mu);
    SCANN_TRY(set_device(ix->ctx));
    return bf_kmeans_init_pp_host(ix->bf, col_offset, sub_dim, k, seed, simd_threshold, centers_out, ix->stream);
}

int scann_hip_kmeans_lloyd(scann_hip_index *ix, uint32_t col_offset, uint32_t sub_dim, float *centers,
                           uint32_t k, uint32_t max_iterations, double convergence_threshold,
                           uint32_t simd_threshold, uint32_t *out_assign, uint32_t *out_sizes,
                           double *out_inertia, uint32_t *out_iterations, int *out_converged) {
    SCANN_TRY(kmeans_args(ix, col_offset, sub_dim, k, centers));
    std::lock_guard<std::mutex> lock(ix->mu);
    SCANN_TRY(set_device(ix->ctx));
    return bf_kmeans_lloyd_host(ix->bf, col_offset, sub_dim, centers, k, max_iterations,
                                convergence_threshold, simd_threshold, out_assign, out_sizes, out_inertia,
                                out_iterations, out_converged, ix->stream);
}

}  // extern "C"

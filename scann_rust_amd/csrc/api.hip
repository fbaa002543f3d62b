// api.hip -- C ABI of libscann_hip.so (include/scann_hip.h): contexts, index handles,
// workspace management and host orchestration.  No CPU compute fallback exists: every
// search entry point runs the HIP kernels or fails.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <chrono>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "allow.h"
#include "bf.h"
#include "build.h"
#include "comm.h"
#include "common.h"
#include "crowd.h"
#include "index_arrays.h"
#include "mmr.h"
#include "mutable.h"
#include "pca.h"
#include "knobs.h"
#include "launch.h"
#include "project.h"
#include "scalarq.h"
#include "txh.h"

namespace scann {

static thread_local std::string g_last_error;
void set_last_error(const std::string &msg) { g_last_error = msg; }
int fail(int status, const std::string &msg) {
    g_last_error = msg;
    return status;
}

}  // namespace scann

using namespace scann;

struct scann_hip_ctx {
    int device = 0;
    int num_cus = 256;
};

enum IndexKind { KIND_BF = 1, KIND_TXH = 2 };

// A buffer of a search workspace: a range of the workspace's ARENA (one device allocation, sub-allocated at 256-byte
// granularity in declaration order).
struct WsBuf {
    void *p = nullptr;
    size_t bytes = 0;   // capacity assigned in the arena
    size_t need = 0;    // largest size any call has asked for
    template <typename T>
    T *as() const { return static_cast<T *>(p); }
};

// Per-call scratch of the Tree-X-Hybrid pipeline.  Every buffer lives in ONE device allocation: a call first states
// what it needs (want), then commit() rebuilds the arena if any buffer has to grow -- one hipFree (which waits for the
// device) + one hipMalloc, every buffer re-placed in declaration order at the largest size seen so far.  Placement
// is therefore a function of the sizes alone, never of the order in which a handle met its batch sizes and
// pre_reorder_k values: round 2 allocated every buffer separately, and a workspace that had grown buffer by buffer
// (free one, allocate it larger, next) left rerank_short_kernel 3x slower than a fresh one of the same sizes.
struct TxhWorkspace {
    WsBuf queries, cdist, tokens, token_dists, vbase, leaf_cnt, leaf_cursor, pair_off, tile_off,
        counters, pair_q, pair_leaf, pair_vbase, pair_thr, slot_of, lutq, thr, cand_cnt, cand, cand_key,
        cand_idx, cand_dist, cand_exact, cand_row, cand_count, out_idx, out_dist, out_count, allow,
        sbase, pair_sbase, stile_off, samp, lut8, lut8_meta, cand32, cand32_codes, cand32_cnt, mfma_thr1, rr_lb, rr_ub, small_tickets,
          wide_min, wide_ckey, wide_ceb, wide_cidx, wide_cnt,
        proj_q,   // projected handles: [nq][dim] projected queries (behind the rest: the buffers before it keep their places)
        surv;     // sparse prefilter's survivor bitmaps (likewise)
    void *arena = nullptr;
    size_t arena_bytes = 0;
    bool dirty = false;
    uint32_t rebuilds = 0;
    TxhWorkspace() = default;
    TxhWorkspace(const TxhWorkspace &) = delete;
    TxhWorkspace &operator=(const TxhWorkspace &) = delete;
    ~TxhWorkspace() { release_all(); }
    template <typename F>
    void for_each(F f) {
        WsBuf *all[] = {&queries, &cdist, &tokens, &token_dists, &vbase, &leaf_cnt, &leaf_cursor, &pair_off, &tile_off,
                        &counters, &pair_q, &pair_leaf, &pair_vbase, &pair_thr, &slot_of, &lutq, &thr, &cand_cnt, &cand,
                        &cand_key, &cand_idx, &cand_dist, &cand_exact, &cand_row, &cand_count, &out_idx, &out_dist,
                        &out_count, &allow, &sbase, &pair_sbase, &stile_off, &samp, &lut8, &lut8_meta, &cand32,
                        &cand32_codes, &cand32_cnt, &mfma_thr1, &rr_lb, &rr_ub, &small_tickets,
                        &wide_min, &wide_ckey, &wide_ceb, &wide_cidx, &wide_cnt, &proj_q, &surv};
        for (WsBuf *b : all) f(*b);
    }
    void want(WsBuf &b, size_t bytes) {
        if (bytes == 0) bytes = 16;
        if (bytes > b.need) b.need = bytes;
        if (b.need > b.bytes) dirty = true;
    }
    int commit() {
        if (!dirty) return SCANN_HIP_OK;
        // Every buffer starts at its own skew inside a 128 KB window.  Back to back, the six per-candidate arrays of a
        // batch ([nq][m] words each) lie exactly nq * m * 4 bytes apart -- 32 MB at nq = 1024, m = 8192 -- so that
        // element (q, i) of ALL of them maps to the same HBM channel and bank: rerank_short_kernel, which walks
        // several of them in step, ran 3x slower on such a layout (0.41 vs 0.14 ms; same instructions, same bytes:
        // round 2's "workspace growth" slowdown was this aliasing, present or absent by the accident of which other
        // buffers the handle had allocated in between).
        auto skew = [](size_t i) { return (((i + 1) * 37) % 509) * 256; };
        size_t total = 0, idx = 0;
        for_each([&](WsBuf &b) { total += ((b.need + 255) & ~(size_t)255) + skew(idx++); });
        if (arena) (void)hipFree(arena);   // (waits for the device: kernels of earlier calls may still read it)
        arena = nullptr;
        arena_bytes = 0;
        for_each([&](WsBuf &b) { b.p = nullptr; b.bytes = 0; });
        SCANN_HIP_CHECK(hipMalloc(&arena, total ? total : 256));
        arena_bytes = total;
        size_t off = 0;
        idx = 0;
        for_each([&](WsBuf &b) {
            off += skew(idx++);
            if (!b.need) return;
            b.p = static_cast<char *>(arena) + off;
            b.bytes = (b.need + 255) & ~(size_t)255;
            off += b.bytes;
        });
        // ticket counters of small_fused_kernel: zero between launches (the kernel leaves them zero)
        if (small_tickets.p) SCANN_HIP_CHECK(hipMemset(small_tickets.p, 0, small_tickets.bytes));
        dirty = false;
        ++rebuilds;
        return SCANN_HIP_OK;
    }
    void release_all() {
        if (arena) (void)hipFree(arena);
        arena = nullptr;
        arena_bytes = 0;
        for_each([&](WsBuf &b) { b = WsBuf(); });
        dirty = false;
    }
};

// Pinned host memory the GPU reads and writes in place (grow-only).  Small host-side searches keep
// their queries and result rows here: the kernels load the queries over the host link and store the
// rows straight into host memory, so a call is launches + ONE stream sync, with no copy commands (each
// hipMemcpyAsync to or from pageable memory costs 5-15 us of host time: five of them were most of a
// single-query call).
struct PinBuf {
    void *host = nullptr, *dev = nullptr;
    size_t bytes = 0;
    uint32_t seq = 0;   // completion-flag value of the last small call staged here
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    ~PinBuf() { release(); }
    void release() {
        if (host) (void)hipHostFree(host);
        host = dev = nullptr;
        bytes = 0;
    }
    int ensure(size_t need) {
        if (need <= bytes && host) return SCANN_HIP_OK;
        release();
        need = (need + 4095) & ~(size_t)4095;
        SCANN_HIP_CHECK(hipHostMalloc(&host, need, hipHostMallocMapped));
        SCANN_HIP_CHECK(hipHostGetDevicePointer(&dev, host, 0));
        std::memset(host, 0, need);   // (completion flags: no stale word may equal a live sequence number)
        bytes = need;
        return SCANN_HIP_OK;
    }
};

// An extra stream + workspaces: host-side searches of concurrent caller threads (Searcher: Send +
// Sync, tests/stress_tests.rs:256-297) run side by side instead of queueing on one mutex.
// Buffers of the crowding stage of one stream: the [nq][depth] rows the search leaves for it (device entry point:
// written by the search's final select, never seen by the host) and, host entry point only, its [nq][k] result.
struct CrowdWorkspace {
    DevBuf idx, dist, cnt, out_idx, out_dist, out_cnt, queries, allow;
    int ensure_rows(uint32_t nq, uint32_t depth) {
        SCANN_TRY(idx.ensure((size_t)nq * depth * 4));
        SCANN_TRY(dist.ensure((size_t)nq * depth * 4));
        return cnt.ensure((size_t)nq * 4);
    }
    int ensure_out(uint32_t nq, uint32_t k) {
        SCANN_TRY(out_idx.ensure((size_t)nq * k * 4));
        SCANN_TRY(out_dist.ensure((size_t)nq * k * 4));
        return out_cnt.ensure((size_t)nq * 4);
    }
};

struct SearchSlot {
    std::mutex mu;
    hipStream_t stream = nullptr;
    TxhWorkspace ws;
    BfWorkspace bfw;
    CrowdWorkspace crowd;
    PinBuf pin;
};

struct scann_hip_index {
    scann_hip_ctx *ctx = nullptr;
    int kind = 0;
    std::mutex mu;  // the primary slot (stream, ws, bfw below): device entry points and timing use it
    std::mutex slots_mu;
    std::vector<std::unique_ptr<SearchSlot>> slots;   // created on demand, at most max_slots() - 1
    hipStream_t stream = nullptr;
    // ring of HIP event pairs bracketing the dominant kernel of each search launch
    static constexpr int kEvRing = 64;
    hipEvent_t evs[kEvRing][2] = {};
    uint32_t ev_n = 0;      // launches recorded since timing was enabled
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // pair handed to the current launch
    bool timing = false;
    bool timing_valid = false;
    void next_events() {
        if (!timing) {
            ev0 = ev1 = nullptr;
            return;
        }
        ev0 = evs[ev_n % kEvRing][0];
        ev1 = evs[ev_n % kEvRing][1];
        ++ev_n;
    }
    const char *timed_kernel = "";
    DevBuf status_word;

    // ---- crowding (scann_hip_index_set_crowding_attributes): one u64 per datapoint index, may be shorter ----
    DevBuf crowd_attrs;
    uint64_t n_crowd_attrs = 0;
    bool has_crowd_attrs = false;
    // multi-attribute crowding (scann_hip_index_set_crowding_attributes_md): [crowd_md_dims][n_crowd_md_attrs] u64,
    // dimension-major; crowd_md_dims == 0: none attached
    DevBuf crowd_md_attrs;
    uint64_t n_crowd_md_attrs = 0;
    uint32_t crowd_md_dims = 0;
    CrowdWorkspace crowd;     // primary slot's

    // ---- brute force ----
    BfIndexDev bf{};
    DevBuf bf_rows, bf_rows_b, bf_rows_bl, bf_norm2, bf_leaf;
    BfWorkspace bfw;
    TxhIndexDev bfx{};        // the same rows as a one-leaf exact-scan index: the small-batch pipeline's view

    // ---- tree-x-hybrid / AH ----
    TxhIndexDev tx{};
    DevBuf d_centers, d_centers_t, d_leaf_off, d_leaf_gsize, d_leaf_ids, d_codes, d_codes_sp, d_rows, d_codebook, d_rows8, d_rows8_meta;
    DevBuf d_qrows;           // scann_hip_txh_create_quantized: the re-rank rows as given (d_rows, d_rows8 stay empty)
    int q_fmt = 0;            // ... their SCANN_HIP_ROWS_* format (0: f32 rows or none) and the int8 inv_multiplier
    float q_inv = 1.0f;
    // scann_hip_txh_create_projected: the handle's own copy of the projection (kind 0: none).  tx.dim is then the
    // projection's out_dim, tx.row_dim / row_stride describe d_rows, and launch_txh projects every call's queries.
    ProjDev proj;
    DevBuf d_proj_matrix, d_proj_mean;
    std::vector<uint32_t> local_sizes_desc;  // local leaf sizes, descending, prefix-summed
    uint32_t default_P = 0;
    float multiplier = 3.0f;
    TxhWorkspace ws;
    PinBuf pin;               // primary slot's pinned staging
    TxhWork last_work{};
    // Workspaces of the `_device` entry points, one per CALLER STREAM (scann_hip.h "Device entry points"): slot 0 is
    // the primary workspace (ws / bfw above), further ones are created on demand.  A slot that changes streams is
    // ordered behind its previous stream's last call with an event.
    struct DeviceSlot {
        hipStream_t key = nullptr;
        bool used = false, done_valid = false;
        hipEvent_t done = nullptr;
        uint64_t tick = 0;
        TxhWorkspace *ws = nullptr;
        BfWorkspace *bfw = nullptr;
        CrowdWorkspace *crowd = nullptr;
        std::unique_ptr<TxhWorkspace> ws_own;
        std::unique_ptr<BfWorkspace> bfw_own;
        std::unique_ptr<CrowdWorkspace> crowd_own;
    };
    static constexpr int kMaxDeviceSlots = 4;
    DeviceSlot dslots[kMaxDeviceSlots];
    uint64_t dslot_tick = 0;
    bool sharded = false;     // created with leaf_sizes_global: local leaves are a subset of the global stream
    uint64_t n_rows = 0;      // rows of d_rows / d_qrows (0: the handle stores none)
};

static int set_device(const scann_hip_ctx *ctx) {
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

static int index_common_init(scann_hip_index *ix);
static int bf_finish(scann_hip_index *ix, uint64_t n, uint32_t dim, uint32_t stride, int measure);
static int bf_finish_quantized(scann_hip_index *ix, uint64_t n, uint32_t dim, uint32_t stride, int row_format,
                               float inv_multiplier, int measure);
static int txh_finish(scann_hip_index *ix, const scann_hip_txh_desc *d, const std::vector<uint32_t> &off);

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

// scalar fields of the descriptor a tree / hasher handle was created from
static void txh_desc_of(const scann_hip_index *ix, scann_hip_txh_desc *d) {
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

int scann::index_fold_bf(const scann_hip_index *old, DevBuf &rows, uint64_t n, uint32_t stride, scann_hip_index **out) {
    DevBuf held;
    held.take(rows);
    if (!old || !out || old->kind != KIND_BF) return fail(SCANN_HIP_INVALID_ARGUMENT, "not a brute-force index");
    SCANN_TRY(set_device(old->ctx));
    auto *ix = new scann_hip_index();
    ix->ctx = old->ctx;
    ix->kind = KIND_BF;
    ix->bf_rows.take(held);
    int s = index_common_init(ix);
    if (s == SCANN_HIP_OK) s = bf_finish(ix, n, old->bf.dim, stride, old->bf.measure);
    if (s != SCANN_HIP_OK) {
        scann_hip_index_destroy(ix);
        return s;
    }
    *out = ix;
    return SCANN_HIP_OK;
}

int scann::index_fold_txh(const scann_hip_index *old, DevBuf &rows, DevBuf &codes, DevBuf &leaf_off, DevBuf &leaf_ids,
                          const std::vector<uint32_t> &off, uint64_t n, uint32_t stride, scann_hip_index **out) {
    DevBuf h_rows, h_codes, h_off, h_ids;
    h_rows.take(rows);
    h_codes.take(codes);
    h_off.take(leaf_off);
    h_ids.take(leaf_ids);
    if (!old || !out || old->kind != KIND_TXH) return fail(SCANN_HIP_INVALID_ARGUMENT, "not a tree / hasher index");
    const TxhIndexDev &t = old->tx;
    if (off.size() != (size_t)t.L + 1) return fail(SCANN_HIP_INTERNAL, "fold: leaf offsets of the wrong length");
    SCANN_TRY(set_device(old->ctx));
    auto *ix = new scann_hip_index();
    ix->ctx = old->ctx;
    ix->kind = KIND_TXH;
    auto bail = [&](int s) {
        scann_hip_index_destroy(ix);
        return s;
    };
    int s = index_common_init(ix);
    if (s != SCANN_HIP_OK) return bail(s);
    ix->d_rows.take(h_rows);
    ix->d_codes.take(h_codes);
    ix->d_leaf_off.take(h_off);
    if (!t.ah_mode) ix->d_leaf_ids.take(h_ids);
    scann_hip_txh_desc d;
    txh_desc_of(old, &d);
    d.n_rows = n;
    d.n_local = n;
    d.stride = stride;
    d.data = ix->d_rows.as<float>();   // (txh_finish asks only whether rows are stored)
    ix->n_rows = n;
    std::vector<uint32_t> gsz(t.L);
    for (uint32_t l = 0; l < t.L; ++l) gsz[l] = off[l + 1] - off[l];
    if ((s = upload(ix->d_leaf_gsize, gsz.data(), (size_t)t.L * 4)) != SCANN_HIP_OK) return bail(s);
    const size_t cb_bytes = (size_t)t.S * t.K * t.dsub * 4;
    if ((s = ix->d_codebook.ensure(cb_bytes)) != SCANN_HIP_OK) return bail(s);
    if (hipMemcpy(ix->d_codebook.p, t.codebook, cb_bytes, hipMemcpyDeviceToDevice) != hipSuccess)
        return bail(fail(SCANN_HIP_INTERNAL, "fold: codebook copy failed"));
    if (!t.ah_mode) {
        const size_t c_bytes = (size_t)t.L * t.dim * 4;
        if ((s = ix->d_centers.ensure(c_bytes)) != SCANN_HIP_OK) return bail(s);
        if (hipMemcpy(ix->d_centers.p, t.centers, c_bytes, hipMemcpyDeviceToDevice) != hipSuccess)
            return bail(fail(SCANN_HIP_INTERNAL, "fold: centre copy failed"));
    }
    if ((s = txh_finish(ix, &d, off)) != SCANN_HIP_OK) return bail(s);
    *out = ix;
    return SCANN_HIP_OK;
}

// The handle of scann_hip_txh_build (build.h): the arrays build_txh_device wrote, a device copy of the source's rows
// when they are stored, then the second half of every tree / hasher create.
// With `proj` (scann_hip_txh_build_projected) the arrays were built from the projected rows: the handle's index space is
// out_dim wide at stride out_dim, the source's rows are the re-rank rows in their own space and the projection is copied
// in, as scann_hip_txh_create_projected lays a handle out.
int scann::index_build_txh(const scann_hip_index *src, const scann_hip_build_config &cfg, BuildParts &parts,
                           scann_hip_index **out, scann_hip_build_report *rep, const scann_hip_projection *proj) {
    if (!src || !out || src->kind != KIND_BF) return fail(SCANN_HIP_INVALID_ARGUMENT, "not a brute-force index");
    const auto t0 = std::chrono::steady_clock::now();
    const bool tree = cfg.num_partitions != 0;
    const uint64_t n = src->bf.n;
    const uint32_t dim = proj ? proj->dev.out_dim : src->bf.dim, stride = proj ? proj->dev.out_dim : src->bf.stride;
    const uint32_t L = parts.L;
    if (parts.off.size() != (size_t)L + 1) return fail(SCANN_HIP_INTERNAL, "build: leaf offsets of the wrong length");
    SCANN_TRY(set_device(src->ctx));
    auto *ix = new scann_hip_index();
    ix->ctx = src->ctx;
    ix->kind = KIND_TXH;
    auto bail = [&](int s) {
        scann_hip_index_destroy(ix);
        return s;
    };
    int s = index_common_init(ix);
    if (s != SCANN_HIP_OK) return bail(s);
    if (cfg.store_rows) {
        const size_t bytes = (size_t)n * src->bf.stride * 4;
        if ((s = ix->d_rows.ensure(bytes)) != SCANN_HIP_OK) return bail(s);
        if (hipMemcpy(ix->d_rows.p, src->bf.rows, bytes, hipMemcpyDeviceToDevice) != hipSuccess)
            return bail(fail(SCANN_HIP_INTERNAL, "build: row copy failed"));
    }
    ix->d_codes.take(parts.codes);
    ix->d_leaf_off.take(parts.leaf_off);
    ix->d_codebook.take(parts.codebook);
    if (tree) {
        ix->d_leaf_ids.take(parts.leaf_ids);
        ix->d_centers.take(parts.centers);
    }
    scann_hip_txh_desc d;
    std::memset(&d, 0, sizeof(d));
    d.n_rows = d.n_local = n;
    d.dim = dim;
    d.stride = stride;
    d.num_partitions = tree ? L : 0u;
    d.num_subspaces = cfg.num_subspaces;
    d.num_codes = cfg.num_codes;
    d.dims_per_subspace = dim / cfg.num_subspaces;
    d.distance_measure = cfg.distance_measure;
    d.codes_packed4 = cfg.num_codes <= 16 ? 1 : 0;
    d.use_residuals = (tree && cfg.use_residuals) ? 1 : 0;
    d.partitions_to_search = tree ? cfg.partitions_to_search : 0u;
    d.pre_reorder_multiplier = cfg.pre_reorder_multiplier;
    // (txh_finish asks only whether rows are stored; a projected handle's rows are not in the index space)
    d.data = (cfg.store_rows && !proj) ? ix->d_rows.as<float>() : nullptr;
    ix->n_rows = (cfg.store_rows && !proj) ? n : 0;
    std::vector<uint32_t> gsz(L);
    for (uint32_t l = 0; l < L; ++l) gsz[l] = parts.off[l + 1] - parts.off[l];
    if ((s = upload(ix->d_leaf_gsize, gsz.data(), (size_t)L * 4)) != SCANN_HIP_OK) return bail(s);
    if ((s = txh_finish(ix, &d, parts.off)) != SCANN_HIP_OK) return bail(s);
    if (proj) {
        const ProjDev &pd = proj->dev;
        ix->proj = pd;
        ix->proj.matrix = ix->proj.mean = nullptr;
        if (pd.kind != SCANN_HIP_PROJ_TRUNCATE) {
            if ((s = upload(ix->d_proj_matrix, proj->matrix.data(), proj->matrix.size() * 4)) != SCANN_HIP_OK) return bail(s);
            ix->proj.matrix = ix->d_proj_matrix.as<float>();
        }
        if (pd.kind == SCANN_HIP_PROJ_PCA) {
            if ((s = upload(ix->d_proj_mean, proj->mean.data(), proj->mean.size() * 4)) != SCANN_HIP_OK) return bail(s);
            ix->proj.mean = ix->d_proj_mean.as<float>();
        }
        if (cfg.store_rows) {
            ix->tx.rows = ix->d_rows.as<float>();
            ix->n_rows = n;
        }
        ix->tx.row_dim = src->bf.dim;
        ix->tx.row_stride = src->bf.stride;
    }
    if (rep) rep->stage_ms[6] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = ix;
    return SCANN_HIP_OK;
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

static int index_common_init(scann_hip_index *ix) {
    SCANN_HIP_CHECK(hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking));
    for (int i = 0; i < scann_hip_index::kEvRing; ++i) {
        SCANN_HIP_CHECK(hipEventCreate(&ix->evs[i][0]));
        SCANN_HIP_CHECK(hipEventCreate(&ix->evs[i][1]));
    }
    return SCANN_HIP_OK;
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

// =====================================================================================
// Brute force
// =====================================================================================
int scann_hip_bf_create(scann_hip_ctx *ctx, const float *data, uint64_t n, uint32_t dim,
                        uint32_t stride, int measure, scann_hip_index **out) {
    if (!ctx || !out) return fail(SCANN_HIP_INVALID_ARGUMENT, "null ctx/out_index");
    if (n > 0 && !data) return fail(SCANN_HIP_INVALID_ARGUMENT, "data is null");
    if (n > 0 && (dim == 0 || stride < dim))
        return fail(SCANN_HIP_INVALID_ARGUMENT, "bad dim/stride");
    if (measure < SCANN_HIP_SQUARED_L2 || measure > SCANN_HIP_COSINE)
        return fail(SCANN_HIP_UNIMPLEMENTED,
                    "brute force supports SquaredL2, L2, DotProduct, L1 and Cosine on the GPU path");
    if (n >= 0xFFFFFFFFull) return fail(SCANN_HIP_OUT_OF_RANGE, "DatapointIndex is u32");
    SCANN_TRY(set_device(ctx));
    auto *ix = new scann_hip_index();
    ix->ctx = ctx;
    ix->kind = KIND_BF;
    int s = index_common_init(ix);
    if (s == SCANN_HIP_OK) s = upload(ix->bf_rows, data, (size_t)n * stride * sizeof(float));
    if (s == SCANN_HIP_OK) s = bf_finish(ix, n, dim, stride, measure);
    if (s != SCANN_HIP_OK) {
        scann_hip_index_destroy(ix);
        return s;
    }
    *out = ix;
    return SCANN_HIP_OK;
}

}  // extern "C"

// The second half of scann_hip_bf_create: the f32 rows are in ix->bf_rows on the device.  scann_hip_fold_mutable ends
// here too, with rows its gather wrote.  The caller destroys the handle on failure.
static int bf_finish(scann_hip_index *ix, uint64_t n, uint32_t dim, uint32_t stride, int measure) {
    int s = SCANN_HIP_OK;
    ix->bf.rows = ix->bf_rows.as<float>();
    ix->bf.n = n;
    ix->bf.dim = dim;
    ix->bf.stride = stride;
    ix->bf.measure = measure;
    ix->bf.rows_b = nullptr;
    ix->bf.rows_bl = nullptr;
    ix->bf.norm2 = nullptr;
    ix->bf.max_norm = 0.0f;
    if (n > 0 && n <= kSmallMaxStream) {   // view for the three-launch small-batch pipeline (txh.hip)
        const uint32_t leaf[3] = {0u, (uint32_t)n, (uint32_t)n};   // leaf_off[0..1], leaf_gsize[0]
        s = upload(ix->bf_leaf, leaf, sizeof(leaf));
        if (s != SCANN_HIP_OK) return s;
        TxhIndexDev &t = ix->bfx;
        t.dim = dim; t.stride = stride; t.L = 1; t.S = 0; t.K = 16; t.dsub = 0; t.nw = 0; t.code_bits = 4; t.kp = 16;
        t.n_local = n; t.centers = nullptr; t.leaf_off = ix->bf_leaf.as<uint32_t>();
        t.leaf_gsize = ix->bf_leaf.as<uint32_t>() + 2; t.leaf_ids = nullptr; t.codes = nullptr;
        t.rows = ix->bf_rows.as<float>(); t.rows8 = nullptr; t.rows8_meta = nullptr; t.rows_csr = 1;
        t.codebook = nullptr; t.use_residuals = 0; t.ah_mode = 1; t.measure = measure; t.exact_scan = 1;
    }
    if ((stride & 3u) == 0) {   // bf16 copy + norms for the shortlist path (big indexes only)
        s = bf_build_shortlist_data(ix->bf, ix->bf_rows_b, ix->bf_rows_bl, ix->bf_norm2, &ix->bf.max_norm,
                                    ix->stream);
        if (s != SCANN_HIP_OK) return s;
        if (ix->bf_rows_b.p) {
            ix->bf.rows_b = ix->bf_rows_b.as<uint16_t>();
            ix->bf.rows_bl = ix->bf_rows_bl.as<uint16_t>();
            ix->bf.norm2 = ix->bf_norm2.as<float>();
        }
    }
    return SCANN_HIP_OK;
}

// The second half of scann_hip_bf_create_quantized: the rows are in ix->bf_rows on the device, as given or written by
// the quantize pass of scann_hip_index_quantize_rows.  The caller destroys the handle on failure.
static int bf_finish_quantized(scann_hip_index *ix, uint64_t n, uint32_t dim, uint32_t stride, int row_format,
                               float inv_multiplier, int measure) {
    ix->bf.rows = nullptr;
    ix->bf.n = n;
    ix->bf.dim = dim;
    ix->bf.stride = stride;
    ix->bf.measure = measure;
    ix->bf.fmt = row_format;
    ix->bf.qrows = ix->bf_rows.p;
    ix->bf.inv_mult = row_format == SCANN_HIP_ROWS_INT8 ? inv_multiplier : 1.0f;
    SCANN_TRY(bf_build_shortlist_data(ix->bf, ix->bf_rows_b, ix->bf_rows_bl, ix->bf_norm2, &ix->bf.max_norm, ix->stream));
    if (ix->bf_norm2.p) ix->bf.norm2 = ix->bf_norm2.as<float>();
    return SCANN_HIP_OK;
}

extern "C" {

// Rows the caller stores quantized (scann_hip.h): uploaded as given, no f32 copy and no small-batch view (bfx stays
// empty); the bf16 shortlist reads the rows themselves and needs only their squared norms.
int scann_hip_bf_create_quantized(scann_hip_ctx *ctx, const void *rows, uint64_t n, uint32_t dim, uint32_t stride,
                                  int row_format, float inv_multiplier, int measure, scann_hip_index **out) {
    if (!ctx || !out) return fail(SCANN_HIP_INVALID_ARGUMENT, "null ctx/out_index");
    if (row_format != SCANN_HIP_ROWS_BF16 && row_format != SCANN_HIP_ROWS_FP8_E4M3 && row_format != SCANN_HIP_ROWS_INT8)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "unknown row format " + std::to_string(row_format));
    if (n > 0 && !rows) return fail(SCANN_HIP_INVALID_ARGUMENT, "rows is null");
    if (n > 0 && (dim == 0 || stride < dim)) return fail(SCANN_HIP_INVALID_ARGUMENT, "bad dim/stride");
    if (row_format == SCANN_HIP_ROWS_INT8 && !std::isfinite(inv_multiplier))
        return fail(SCANN_HIP_INVALID_ARGUMENT, "inv_multiplier is not finite");
    if (measure == SCANN_HIP_L1 || measure == SCANN_HIP_COSINE)
        return fail(SCANN_HIP_UNIMPLEMENTED, "quantized rows: SquaredL2, L2 and DotProduct only");
    if (measure < SCANN_HIP_SQUARED_L2 || measure > SCANN_HIP_DOT_PRODUCT)
        return fail(SCANN_HIP_UNIMPLEMENTED, "unknown distance measure");
    if (n >= 0xFFFFFFFFull) return fail(SCANN_HIP_OUT_OF_RANGE, "DatapointIndex is u32");
    SCANN_TRY(set_device(ctx));
    auto *ix = new scann_hip_index();
    ix->ctx = ctx;
    ix->kind = KIND_BF;
    const size_t bytes = (size_t)n * stride * (row_format == SCANN_HIP_ROWS_BF16 ? 2 : 1);
    int s = index_common_init(ix);
    if (s == SCANN_HIP_OK) s = upload(ix->bf_rows, rows, bytes);
    if (s != SCANN_HIP_OK) {
        scann_hip_index_destroy(ix);
        return s;
    }
    s = bf_finish_quantized(ix, n, dim, stride, row_format, inv_multiplier, measure);
    if (s != SCANN_HIP_OK) {
        scann_hip_index_destroy(ix);
        return s;
    }
    *out = ix;
    return SCANN_HIP_OK;
}

int scann_hip_bf16_quantize(scann_hip_ctx *ctx, const float *values, uint64_t n, uint16_t *out_bits) {
    if (!ctx) return fail(SCANN_HIP_INVALID_ARGUMENT, "ctx is null");
    if (n == 0) return SCANN_HIP_OK;
    if (!values || !out_bits) return fail(SCANN_HIP_INVALID_ARGUMENT, "null values/output");
    SCANN_TRY(set_device(ctx));
    return bf16_quantize_host(values, n, out_bits, nullptr);
}

// =====================================================================================
// Tree-X-Hybrid / AsymmetricHasher index
// =====================================================================================
}  // extern "C"

// content_status: what inconsistent array CONTENTS are reported as (InvalidArgument for caller-built
// descriptors, DataLoss for index files, whose section sizes were already checked)
int scann::txh_create_checked(scann_hip_ctx *ctx, const scann_hip_txh_desc *d, scann_hip_index **out,
                              int content_status, const void *qrows, int qfmt, float qinv, DevBuf *qrows_dev) {
    if (!ctx || !d || !out) return fail(SCANN_HIP_INVALID_ARGUMENT, "null ctx/desc/out_index");
    const bool ah = d->num_partitions == 0;
    const bool has_rows = d->data || qrows || qrows_dev;   // re-rank rows, f32 or quantized: indexed and validated alike
    if (d->n_local == 0)  // tree_x_hybrid/mod.rs:132-134, hashes/hasher.rs:110-112
        return fail(SCANN_HIP_INVALID_ARGUMENT, "Cannot build from empty dataset");
    if (d->n_local >= 0xFFFFFFFFull) return fail(SCANN_HIP_OUT_OF_RANGE, "DatapointIndex is u32");
    // SearchMode::Partitioned (scann.rs:213-252): no codebook, the selected leaves are scored exactly
    const bool exact = !d->codebook && !d->codes && d->num_subspaces == 0;
    if (!exact && (!d->codebook || !d->codes)) return fail(SCANN_HIP_INVALID_ARGUMENT, "codebook/codes null");
    if (d->distance_measure < SCANN_HIP_SQUARED_L2 || d->distance_measure > SCANN_HIP_COSINE)
        return fail(SCANN_HIP_UNIMPLEMENTED, "distance_measure must be SquaredL2, L2, DotProduct, L1 or Cosine");
    const uint32_t S = d->num_subspaces, K = exact ? 16u : d->num_codes, dsub = d->dims_per_subspace;
    if (d->dim == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "dim is 0");
    if (exact) {
        if (ah || !d->data || d->leaf_sizes_global || d->n_rows != d->n_local)
            return fail(SCANN_HIP_INVALID_ARGUMENT,
                        "the exact leaf scan needs centers, the dataset rows and an unsharded index");
    } else if (S == 0 || d->dim % S != 0 || dsub != d->dim / S) {  // codebook.rs:154-159
        return fail(SCANN_HIP_INVALID_ARGUMENT,
                    "Dimensionality " + std::to_string(d->dim) +
                        " must be divisible by num_subspaces " + std::to_string(S));
    }
    if (K == 0 || K > 256)
        return fail(SCANN_HIP_UNIMPLEMENTED, "num_codes must be 1..256");
    // K <= 16: 4-bit packed codes + 16-slot tables (LUT16); else bytes + 256-slot tables
    const uint32_t bits = K <= 16 ? 4u : 8u;
    if (!exact && bits == 4 && (S % 8 != 0 || S > 64 || S == 40 || S == 56))
        return fail(SCANN_HIP_UNIMPLEMENTED, "num_subspaces must be 8,16,24,32,48 or 64 for num_codes <= 16");
    if (bits == 8 && S != 4 && S != 8 && S != 16)
        return fail(SCANN_HIP_UNIMPLEMENTED, "num_subspaces must be 4, 8 or 16 for 16 < num_codes <= 256");
    if (bits == 8 && d->codes_packed4)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "codes_packed4 needs num_codes <= 16");
    if (!ah) {
        if (!d->centers || !d->leaf_offsets || !d->leaf_ids)
            return fail(SCANN_HIP_INVALID_ARGUMENT, "centers/leaf_offsets/leaf_ids null");
        if (d->num_partitions > kMaxLeavesSelect)
            return fail(SCANN_HIP_UNIMPLEMENTED, "num_partitions > 16384");
        if (d->leaf_offsets[0] != 0 || d->leaf_offsets[d->num_partitions] != d->n_local)
            return fail(content_status, "leaf_offsets must span [0, n_local]");
        for (uint32_t l = 0; l < d->num_partitions; ++l) {
            if (d->leaf_offsets[l + 1] < d->leaf_offsets[l])
                return fail(content_status, "leaf_offsets not monotone");
            // merge keys and their decoding assume a leaf's local rows are a prefix of the global leaf
            if (d->leaf_sizes_global && d->leaf_sizes_global[l] < d->leaf_offsets[l + 1] - d->leaf_offsets[l])
                return fail(content_status, "leaf_sizes_global smaller than the local leaf");
        }
        // the re-rank and the exact leaf scan read data + leaf_ids[row] * stride
        if (has_rows && !d->data_is_csr_order)
            for (uint64_t i = 0; i < d->n_local; ++i)
                if (d->leaf_ids[i] >= d->n_rows)
                    return fail(content_status, "leaf_ids entry " + std::to_string(i) + " >= n_rows");
    }
    if (has_rows && d->stride < d->dim) return fail(SCANN_HIP_INVALID_ARGUMENT, "stride < dim");
    if (has_rows && d->data_is_csr_order && d->n_rows != d->n_local)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "CSR-ordered data must have n_local rows");
    // AsymmetricHasher mode reads row i of data for CSR row i
    if (has_rows && ah && d->n_rows < d->n_local)
        return fail(content_status, "data has fewer rows than the index has points");
    SCANN_TRY(set_device(ctx));

    auto *ix = new scann_hip_index();
    ix->ctx = ctx;
    ix->kind = KIND_TXH;
    auto bail = [&](int s) {
        scann_hip_index_destroy(ix);
        return s;
    };
    int s = index_common_init(ix);
    if (s != SCANN_HIP_OK) return bail(s);

    const uint32_t L = ah ? 1u : d->num_partitions;
    const uint32_t nw = bits == 4 ? S / 8 : S / 4;
    const uint64_t n = d->n_local;

    // leaf tables
    std::vector<uint32_t> off(L + 1), gsz(L);
    if (ah) {
        off[0] = 0;
        off[1] = (uint32_t)n;
        gsz[0] = (uint32_t)n;
    } else {
        std::memcpy(off.data(), d->leaf_offsets, (size_t)(L + 1) * 4);
        for (uint32_t l = 0; l < L; ++l)
            gsz[l] = d->leaf_sizes_global ? d->leaf_sizes_global[l] : off[l + 1] - off[l];
    }
    // packed codes: [n][nw] words, nibble nb of word wi = subspace 8*wi+nb
    // (PackedCodes4Bit layout, hashes/lut16.rs:43-61, read little-endian)
    std::vector<uint32_t> words;
    const uint32_t *code_words = nullptr;
    const size_t bpp = S / 2;
    if (exact) {
        // no codes
    } else if (d->codes_packed4) {
        if (K < 16) {   // every nibble must address a trained centre (K == 16: all values are valid)
            const size_t nbytes = (size_t)n * bpp;
            for (size_t i = 0; i < nbytes; ++i)
                if ((d->codes[i] & 15u) >= K || (d->codes[i] >> 4) >= K)
                    return bail(fail(content_status, "code value >= num_codes"));
        }
        if ((reinterpret_cast<uintptr_t>(d->codes) & 3u) == 0) {
            code_words = reinterpret_cast<const uint32_t *>(d->codes);
        } else {
            words.resize((size_t)n * nw);
            std::memcpy(words.data(), d->codes, (size_t)n * bpp);
            code_words = words.data();
        }
    } else {
        words.assign((size_t)n * nw, 0u);
        for (uint64_t i = 0; i < n; ++i) {
            const uint8_t *c = d->codes + i * S;
            uint32_t *w = words.data() + i * nw;
            for (uint32_t sidx = 0; sidx < S; ++sidx) {
                if (c[sidx] >= K) {
                    return bail(fail(content_status, "code value >= num_codes"));
                }
                if (bits == 4) w[sidx >> 3] |= (uint32_t)(c[sidx] & 0x0F) << (4 * (sidx & 7u));
                else w[sidx >> 2] |= (uint32_t)c[sidx] << (8 * (sidx & 3u));
            }
        }
        code_words = words.data();
    }

    if ((s = upload(ix->d_leaf_off, off.data(), (size_t)(L + 1) * 4)) != SCANN_HIP_OK) return bail(s);
    if ((s = upload(ix->d_leaf_gsize, gsz.data(), (size_t)L * 4)) != SCANN_HIP_OK) return bail(s);
    if (!exact) {
        if ((s = upload(ix->d_codes, code_words, (size_t)n * nw * 4)) != SCANN_HIP_OK) return bail(s);
        if ((s = upload(ix->d_codebook, d->codebook, (size_t)S * K * dsub * 4)) != SCANN_HIP_OK) return bail(s);
    }
    if (!ah) {
        if ((s = upload(ix->d_centers, d->centers, (size_t)L * d->dim * 4)) != SCANN_HIP_OK) return bail(s);
        if ((s = upload(ix->d_leaf_ids, d->leaf_ids, (size_t)n * 4)) != SCANN_HIP_OK) return bail(s);
    }
    if (d->data) {
        if ((s = upload(ix->d_rows, d->data, (size_t)d->n_rows * d->stride * 4)) != SCANN_HIP_OK)
            return bail(s);
    }

    if (qrows) {   // as given: no f32 copy, and txh_finish builds no 8-bit shadow store without d->data
        const size_t qbytes = (size_t)d->n_rows * d->stride * (qfmt == SCANN_HIP_ROWS_BF16 ? 2 : 1);
        if ((s = upload(ix->d_qrows, qrows, qbytes)) != SCANN_HIP_OK) return bail(s);
        ix->q_fmt = qfmt;
        ix->q_inv = qfmt == SCANN_HIP_ROWS_INT8 ? qinv : 1.0f;
    } else if (qrows_dev) {   // the same rows, written on the device by the quantize pass
        ix->d_qrows.take(*qrows_dev);
        ix->q_fmt = qfmt;
        ix->q_inv = qfmt == SCANN_HIP_ROWS_INT8 ? qinv : 1.0f;
    }
    ix->n_rows = has_rows ? d->n_rows : 0;
    if ((s = txh_finish(ix, d, off)) != SCANN_HIP_OK) return bail(s);
    *out = ix;
    return SCANN_HIP_OK;
}

// The second half of every tree / hasher create: the handle's arrays are on the device (d_leaf_off, d_leaf_gsize,
// d_codes, d_codebook, d_centers, d_leaf_ids, d_rows), `off` is the host copy of the leaf offsets.  Reads the scalar
// fields of `d` and whether d->data / d->leaf_sizes_global are set, never the host arrays: scann_hip_fold_mutable ends
// here too, with arrays its kernels wrote.  The caller destroys the handle on failure.
static int txh_finish(scann_hip_index *ix, const scann_hip_txh_desc *d, const std::vector<uint32_t> &off) {
    const bool ah = d->num_partitions == 0;
    const bool exact = d->num_subspaces == 0;
    const uint32_t S = d->num_subspaces, K = exact ? 16u : d->num_codes, dsub = d->dims_per_subspace;
    const uint32_t bits = K <= 16 ? 4u : 8u;
    const uint32_t L = ah ? 1u : d->num_partitions;
    const uint32_t nw = bits == 4 ? S / 8 : S / 4;
    const uint64_t n = d->n_local;
    int s = SCANN_HIP_OK;
    ix->local_sizes_desc.resize(L);
    for (uint32_t l = 0; l < L; ++l) ix->local_sizes_desc[l] = off[l + 1] - off[l];
    std::sort(ix->local_sizes_desc.begin(), ix->local_sizes_desc.end(), std::greater<uint32_t>());

    TxhIndexDev &t = ix->tx;
    t.dim = d->dim;
    t.stride = d->stride;
    t.row_dim = d->dim;       // (scann_hip_txh_create_projected overwrites the two)
    t.row_stride = d->stride;
    t.L = L;
    t.S = S;
    t.K = K;
    t.dsub = dsub;
    t.nw = nw;
    t.code_bits = bits;
    t.kp = bits == 4 ? 16u : 256u;
    t.n_local = n;
    t.centers = ah ? nullptr : ix->d_centers.as<float>();
    t.centers_t = nullptr;
    t.centers_pitch = 0;
    if (!ah && L <= 4096) {   // transposed centroids: the small-batch leaf selection reads them coalesced (txh.hip)
        const uint32_t pitch = (L + 63u) & ~63u;
        if ((s = ix->d_centers_t.ensure((size_t)pitch * d->dim * 4)) != SCANN_HIP_OK) return s;
        if ((s = launch_transpose_centers(ix->d_centers.as<float>(), L, d->dim, pitch, ix->d_centers_t.as<float>(),
                                          ix->stream)) != SCANN_HIP_OK)
            return s;
        if (hipStreamSynchronize(ix->stream) != hipSuccess) return fail(SCANN_HIP_INTERNAL, "centroid transpose failed");
        t.centers_t = ix->d_centers_t.as<float>();
        t.centers_pitch = pitch;
    }
    t.leaf_off = ix->d_leaf_off.as<uint32_t>();
    t.leaf_gsize = ix->d_leaf_gsize.as<uint32_t>();
    t.leaf_ids = ah ? nullptr : ix->d_leaf_ids.as<uint32_t>();
    t.codes = exact ? nullptr : ix->d_codes.as<uint32_t>();
    t.codes_sp = nullptr;
    const Knobs kn = read_knobs();
    // operand planes of the sparse-MFMA prefilter (txh_prefilter.hip K6e): a second copy of the 4-bit codes, S/2 .. 2 S bytes
    // per point.  SCANN_HIP_SMFMAC=0: not built, the dense integer-MFMA prefilter is used instead.
    {
        if (!exact && bits == 4 && kn.smfmac) {
            if ((s = ix->d_codes_sp.ensure((size_t)n * sp_words(S) * 4)) != SCANN_HIP_OK) return s;
            if ((s = launch_codes_sp_build(ix->d_codes.as<uint32_t>(), n, S, ix->d_codes_sp.as<uint32_t>(), ix->stream)) != SCANN_HIP_OK)
                return s;
            if (hipStreamSynchronize(ix->stream) != hipSuccess) return fail(SCANN_HIP_INTERNAL, "code plane build failed");
            t.codes_sp = ix->d_codes_sp.as<uint32_t>();
        }
    }
    t.measure = d->distance_measure;
    t.exact_scan = exact ? 1 : 0;
    t.rows = d->data ? ix->d_rows.as<float>() : nullptr;
    t.rows8 = nullptr;
    t.rows8_meta = nullptr;
    t.qrows = ix->q_fmt ? ix->d_qrows.p : nullptr;
    t.qfmt = ix->q_fmt;
    t.inv_mult = ix->q_inv;
    // 8-bit copy of the rows for the re-rank filter (txh.hip K8b): +25 % of the row bytes.  Large indexes
    // only (the filter pays for long candidate lists); SCANN_HIP_RERANK_I8 = 0 never, 2 always.
    // SCANN_HIP_RERANK_STORE = int8 (default: per-row scaled integers, the tighter filter) or fp8 (the
    // reference's E4M3 codec with a per-row calibrate_scale, quantization/fp8.rs).
    t.rows8_fmt = 0;
    t.rows8_uniform = 0;
    t.rows8_scale = t.rows8_emax = 0.0f;
    {
        const int mode = kn.rerank_i8;
        const bool fp8 = kn.rerank_fp8;
        const bool want = d->data && !exact && d->distance_measure == SCANN_HIP_SQUARED_L2 && (d->dim & 15u) == 0 &&
                          (mode == 2 || (mode == 1 && d->n_rows >= 65536));
        if (want) {
            if ((s = ix->d_rows8.ensure((size_t)d->n_rows * d->dim)) != SCANN_HIP_OK) return s;
            if ((s = ix->d_rows8_meta.ensure((size_t)d->n_rows * 8)) != SCANN_HIP_OK) return s;
            if (fp8) {
                DevBuf mism;
                if ((s = mism.ensure(4)) != SCANN_HIP_OK) return s;
                if (hipMemsetAsync(mism.p, 0, 4, ix->stream) != hipSuccess) return fail(SCANN_HIP_INTERNAL, "memset failed");
                if ((s = launch_rows_fp8_build(ix->d_rows.as<float>(), d->n_rows, d->dim, d->stride,
                                               ix->d_rows8.as<uint8_t>(), ix->d_rows8_meta.p, mism.as<uint32_t>(),
                                               ix->stream)) != SCANN_HIP_OK)
                    return s;
                uint32_t bad = 0;
                if (hipMemcpyAsync(&bad, mism.p, 4, hipMemcpyDeviceToHost, ix->stream) != hipSuccess ||
                    hipStreamSynchronize(ix->stream) != hipSuccess)
                    return fail(SCANN_HIP_INTERNAL, "fp8 row build failed");
                if (bad) return fail(SCANN_HIP_INTERNAL, "v_cvt_f32_fp8 decodes the reference's E4M3 codes differently");
                t.rows8_fmt = 1;
            } else {
                if ((s = launch_rows_i8_build(ix->d_rows.as<float>(), d->n_rows, d->dim, d->stride, ix->d_rows8.as<int8_t>(),
                                              ix->d_rows8_meta.p, ix->stream)) != SCANN_HIP_OK)
                    return s;
                if (hipStreamSynchronize(ix->stream) != hipSuccess) return fail(SCANN_HIP_INTERNAL, "int8 row build failed");
                // Rows of EQUAL magnitude (largest per-row scale within 2 % of the mean scale, every row finite): ONE
                // scale and ONE error bound (the largest ||x - x~||) for all rows, so that the filter pass gathers a
                // candidate's 128-byte row and nothing else -- the per-row {scale, error} pair is a second random
                // cache line per candidate, half of the pass's memory requests (C3, uniform data: 163 -> 128 us).  The
                // bound is strict because a coarser common scale widens every bracket: on the clustered 10M x 128 set
                // (per-row maxima 25 % apart, candidates nearly equidistant) the shortlists outgrew the fast path and
                // the step went from 1.43 to 1.86 ms.  SCANN_HIP_RERANK_UNIFORM=0: always per-row, 2: always one scale.
                const double spread = kn.rerank_uniform == 2 ? 1e30 : 1.02;
                if (kn.rerank_uniform != 0) {
                    std::vector<float> meta((size_t)d->n_rows * 2);
                    if (hipMemcpy(meta.data(), ix->d_rows8_meta.p, meta.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
                        return fail(SCANN_HIP_INTERNAL, "int8 row meta copy failed");
                    double sum = 0.0;
                    float smax = 0.0f;
                    bool finite = true;
                    for (uint64_t r = 0; r < d->n_rows; ++r) {
                        const float sc = meta[2 * r], E = meta[2 * r + 1];
                        finite = finite && E < INFINITY && sc < INFINITY;
                        smax = std::max(smax, sc);
                        sum += sc;
                    }
                    if (finite && d->n_rows > 0 && (double)smax <= spread * (sum / (double)d->n_rows)) {
                        if ((s = launch_rows_i8_build(ix->d_rows.as<float>(), d->n_rows, d->dim, d->stride, ix->d_rows8.as<int8_t>(),
                                                      ix->d_rows8_meta.p, ix->stream, smax)) != SCANN_HIP_OK)
                            return s;
                        if (hipMemcpy(meta.data(), ix->d_rows8_meta.p, meta.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
                            return fail(SCANN_HIP_INTERNAL, "int8 row meta copy failed");
                        float emax = 0.0f;
                        for (uint64_t r = 0; r < d->n_rows; ++r) emax = std::max(emax, meta[2 * r + 1]);
                        if (emax < INFINITY) {
                            t.rows8_uniform = 1;
                            t.rows8_scale = smax;
                            t.rows8_emax = emax;
                        }
                    }
                }
            }
            t.rows8 = ix->d_rows8.as<int8_t>();
            t.rows8_meta = ix->d_rows8_meta.p;
        }
    }
    // AH mode: CSR row == datapoint index.  Sharded: rows arrive in CSR order.
    t.rows_csr = (ah || d->data_is_csr_order) ? 1 : 0;
    t.codebook = exact ? nullptr : ix->d_codebook.as<float>();
    t.use_residuals = (!ah && d->use_residuals) ? 1 : 0;
    t.ah_mode = ah ? 1 : 0;
    ix->sharded = d->leaf_sizes_global != nullptr;
    ix->default_P = ah ? 1u : std::max(1u, d->partitions_to_search);
    ix->multiplier = d->pre_reorder_multiplier;
    return SCANN_HIP_OK;
}

extern "C" {

int scann_hip_txh_create(scann_hip_ctx *ctx, const scann_hip_txh_desc *d, scann_hip_index **out) {
    return scann::txh_create_checked(ctx, d, out, SCANN_HIP_INVALID_ARGUMENT);
}

}  // extern "C"

// What scann_hip_txh_create_quantized and the index-file loader ask of a descriptor and its quantized rows before
// the checks of scann_hip_txh_create.
int scann::txh_quantized_args(const scann_hip_txh_desc *d, const void *rows, int row_format, float inv_multiplier) {
    if (!d) return fail(SCANN_HIP_INVALID_ARGUMENT, "null ctx/desc/out_index");
    if (d->data) return fail(SCANN_HIP_INVALID_ARGUMENT, "quantized rows: desc.data must be NULL (the rows are the `rows` argument)");
    if (!rows) return fail(SCANN_HIP_INVALID_ARGUMENT, "quantized rows: rows is null");
    if (row_format != SCANN_HIP_ROWS_BF16 && row_format != SCANN_HIP_ROWS_FP8_E4M3 && row_format != SCANN_HIP_ROWS_INT8)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "quantized rows: unknown row format " + std::to_string(row_format));
    if (row_format == SCANN_HIP_ROWS_INT8 && !std::isfinite(inv_multiplier))
        return fail(SCANN_HIP_INVALID_ARGUMENT, "quantized rows: inv_multiplier is not finite");
    if (d->distance_measure == SCANN_HIP_L1 || d->distance_measure == SCANN_HIP_COSINE)
        return fail(SCANN_HIP_UNIMPLEMENTED, "quantized rows: SquaredL2, L2 and DotProduct only");
    if (d->leaf_sizes_global || (d->data_is_csr_order && d->num_partitions))
        return fail(SCANN_HIP_UNIMPLEMENTED, "quantized rows in a leaf-sharded index are not built");
    if (!d->codebook && !d->codes && d->num_subspaces == 0)
        return fail(SCANN_HIP_UNIMPLEMENTED, "quantized rows in SearchMode::Partitioned (no codes) are not built");
    return SCANN_HIP_OK;
}

extern "C" {

int scann_hip_txh_create_quantized(scann_hip_ctx *ctx, const scann_hip_txh_desc *d, const void *rows, int row_format,
                                   float inv_multiplier, scann_hip_index **out) {
    if (!ctx || !d || !out) return fail(SCANN_HIP_INVALID_ARGUMENT, "null ctx/desc/out_index");
    SCANN_TRY(scann::txh_quantized_args(d, rows, row_format, inv_multiplier));
    return scann::txh_create_checked(ctx, d, out, SCANN_HIP_INVALID_ARGUMENT, rows, row_format, inv_multiplier);
}

}  // extern "C"

// ---- projected handles (project.h) ------------------------------------------------------------------
extern "C" {

int scann_hip_txh_create_projected(scann_hip_ctx *ctx, const scann_hip_txh_desc *d, const scann_hip_projection *proj,
                                   const float *rows, uint64_t n_rows, uint32_t row_dim, uint32_t row_stride,
                                   scann_hip_index **out) {
    return scann::txh_create_projected_checked(ctx, d, proj, rows, n_rows, row_dim, row_stride, out, SCANN_HIP_INVALID_ARGUMENT);
}

}  // extern "C"

int scann::txh_create_projected_checked(scann_hip_ctx *ctx, const scann_hip_txh_desc *d, const scann_hip_projection *proj,
                                        const float *rows, uint64_t n_rows, uint32_t row_dim, uint32_t row_stride,
                                        scann_hip_index **out, int content_status) {
    if (!ctx || !d || !out) return fail(SCANN_HIP_INVALID_ARGUMENT, "null ctx/desc/out_index");
    if (!proj) return fail(SCANN_HIP_INVALID_ARGUMENT, "projected index: projection is null");
    const ProjDev &pd = proj->dev;
    if (d->data)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "projected index: desc.data must be NULL (the rows are the `rows` argument)");
    if (d->dim != pd.out_dim)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "projected index: desc.dim " + std::to_string(d->dim) +
                                                    " is not the projection's out_dim " + std::to_string(pd.out_dim));
    if (row_dim != pd.in_dim)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "projected index: row_dim " + std::to_string(row_dim) +
                                                    " is not the projection's in_dim " + std::to_string(pd.in_dim));
    if (row_stride < row_dim) return fail(SCANN_HIP_INVALID_ARGUMENT, "projected index: row_stride < row_dim");
    if (d->leaf_sizes_global || (d->data_is_csr_order && d->num_partitions))
        return fail(SCANN_HIP_UNIMPLEMENTED, "a projection in a leaf-sharded index is not built");
    if (!d->codebook && !d->codes && d->num_subspaces == 0)
        return fail(SCANN_HIP_UNIMPLEMENTED, "a projection in SearchMode::Partitioned (no codes) is not built");
    // the rows are validated as desc.data is (txh_create_checked skips these without desc.data)
    if (rows) {
        if (d->num_partitions == 0) {
            if (n_rows < d->n_local)
                return fail(content_status, "data has fewer rows than the index has points");
        } else if (d->leaf_ids) {
            for (uint64_t i = 0; i < d->n_local; ++i)
                if (d->leaf_ids[i] >= n_rows)
                    return fail(content_status, "leaf_ids entry " + std::to_string(i) + " >= n_rows");
        }
        if (n_rows > SIZE_MAX / 4 / row_stride) return fail(SCANN_HIP_OUT_OF_RANGE, "projected index: n_rows * row_stride overflows");
    }
    scann_hip_txh_desc dd = *d;
    dd.n_rows = rows ? n_rows : 0;
    dd.stride = d->dim;   // (index space; no row is read at it)
    scann_hip_index *ix = nullptr;
    SCANN_TRY(scann::txh_create_checked(ctx, &dd, &ix, content_status));
    auto bail = [&](int s) {
        scann_hip_index_destroy(ix);
        return s;
    };
    int s = SCANN_HIP_OK;
    ix->proj = pd;
    ix->proj.matrix = ix->proj.mean = nullptr;
    if (pd.kind != SCANN_HIP_PROJ_TRUNCATE) {
        if ((s = upload(ix->d_proj_matrix, proj->matrix.data(), proj->matrix.size() * 4)) != SCANN_HIP_OK) return bail(s);
        ix->proj.matrix = ix->d_proj_matrix.as<float>();
    }
    if (pd.kind == SCANN_HIP_PROJ_PCA) {
        if ((s = upload(ix->d_proj_mean, proj->mean.data(), proj->mean.size() * 4)) != SCANN_HIP_OK) return bail(s);
        ix->proj.mean = ix->d_proj_mean.as<float>();
    }
    if (rows) {
        if ((s = upload(ix->d_rows, rows, (size_t)n_rows * row_stride * 4)) != SCANN_HIP_OK) return bail(s);
        ix->tx.rows = ix->d_rows.as<float>();
        ix->n_rows = n_rows;
    }
    ix->tx.row_dim = row_dim;
    ix->tx.row_stride = row_stride;
    *out = ix;
    return SCANN_HIP_OK;
}

extern "C" {

int scann_hip_index_projection_info(const scann_hip_index *ix, uint32_t *out4) {
    if (!ix || !out4) return fail(SCANN_HIP_INVALID_ARGUMENT, "null index/output");
    out4[0] = (uint32_t)ix->proj.kind;
    out4[1] = ix->proj.in_dim;
    out4[2] = ix->proj.out_dim;
    out4[3] = ix->proj.start;
    return SCANN_HIP_OK;
}

}  // extern "C"

// ---- scalar quantizer over a handle's f32 rows (scalarq.h) ------------------------------------------
// The f32 rows scann_hip_index_quantization_stats and scann_hip_index_quantize_rows read, or why there are none.
struct SqSource {
    const float *rows = nullptr;
    uint64_t n = 0;
    uint32_t dim = 0, stride = 0;
    int measure = 0;
};

static int sq_source(const scann_hip_index *ix, SqSource *o) {
    if (!ix) return fail(SCANN_HIP_INVALID_ARGUMENT, "index is null");
    if (ix->kind == KIND_BF) {
        if (ix->bf.fmt) return fail(SCANN_HIP_INVALID_ARGUMENT, "the index already holds quantized rows");
        if (ix->bf.n == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "Cannot quantize empty dataset");
        if (ix->bf.measure == SCANN_HIP_L1 || ix->bf.measure == SCANN_HIP_COSINE)
            return fail(SCANN_HIP_UNIMPLEMENTED, "quantized rows: SquaredL2, L2 and DotProduct only");
        *o = SqSource{ix->bf.rows, ix->bf.n, ix->bf.dim, ix->bf.stride, ix->bf.measure};
        return SCANN_HIP_OK;
    }
    const TxhIndexDev &t = ix->tx;
    if (ix->proj.kind) return fail(SCANN_HIP_UNIMPLEMENTED, "quantized rows behind a projection are not built");
    if (t.qfmt) return fail(SCANN_HIP_INVALID_ARGUMENT, "the index already holds quantized rows");
    if (t.measure == SCANN_HIP_L1 || t.measure == SCANN_HIP_COSINE)
        return fail(SCANN_HIP_UNIMPLEMENTED, "quantized rows: SquaredL2, L2 and DotProduct only");
    if (ix->sharded || (t.rows_csr && !t.ah_mode))
        return fail(SCANN_HIP_UNIMPLEMENTED, "quantized rows in a leaf-sharded index are not built");
    if (t.exact_scan) return fail(SCANN_HIP_UNIMPLEMENTED, "quantized rows in SearchMode::Partitioned (no codes) are not built");
    if (!t.rows || ix->n_rows == 0) return fail(SCANN_HIP_FAILED_PRECONDITION, "the index stores no rows to quantize");
    *o = SqSource{t.rows, ix->n_rows, t.dim, t.stride, t.measure};
    return SCANN_HIP_OK;
}

extern "C" {

int scann_hip_index_quantization_stats(scann_hip_index *ix, float *out_stats4) {
    if (!ix || !out_stats4) return fail(SCANN_HIP_INVALID_ARGUMENT, "null index/output");
    SqSource src;
    SCANN_TRY(sq_source(ix, &src));
    SCANN_TRY(set_device(ix->ctx));
    SqPartial sums;
    {
        std::lock_guard<std::mutex> lock(ix->mu);
        SCANN_TRY(sq_stats_device(src.rows, src.n, src.dim, src.stride, ix->stream, &sums));
    }
    sq_stats_finish(sums, src.n * src.dim, out_stats4);
    return SCANN_HIP_OK;
}

int scann_hip_index_quantize_rows(scann_hip_index *src_ix, int row_format, uint32_t bits, int mode, float a, float b,
                                  scann_hip_index **out, float *out_params4, int32_t *out_zero_point) {
    if (!src_ix || !out) return fail(SCANN_HIP_INVALID_ARGUMENT, "null index/out_index");
    if (row_format != SCANN_HIP_ROWS_BF16 && row_format != SCANN_HIP_ROWS_FP8_E4M3 && row_format != SCANN_HIP_ROWS_INT8)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "unknown row format " + std::to_string(row_format));
    SqSource src;
    SCANN_TRY(sq_source(src_ix, &src));
    SCANN_TRY(set_device(src_ix->ctx));
    SqParams p{0.0f, 0.0f, 1.0f, 1.0f, 255};
    int32_t zp = 0;
    const size_t qbytes = (size_t)src.n * src.stride * (row_format == SCANN_HIP_ROWS_BF16 ? 2 : 1);
    DevBuf qrows;
    {
        std::lock_guard<std::mutex> lock(src_ix->mu);   // the source's primary stream runs both passes
        if (row_format == SCANN_HIP_ROWS_INT8) {
            // a bad mode / bits / range is refused before any device work
            const float probe[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            SqParams tmp{};
            int32_t tz = 0;
            SCANN_TRY(sq_calibrate(probe, bits, mode, a, b, &tmp, &tz));
            SqPartial sums;
            SCANN_TRY(sq_stats_device(src.rows, src.n, src.dim, src.stride, src_ix->stream, &sums));
            if (mode == SCANN_HIP_SQ_SIGNED && sums.nonfinite)
                return fail(SCANN_HIP_INVALID_ARGUMENT, "scalar quantizer: the signed mode needs finite values");
            float stats4[4];
            sq_stats_finish(sums, src.n * src.dim, stats4);
            SCANN_TRY(sq_calibrate(stats4, bits, mode, a, b, &p, &zp));
        }
        SCANN_TRY(qrows.ensure(qbytes));
        SCANN_TRY(launch_sq_quantize(src.rows, src.n, src.dim, src.stride, row_format, mode, p, qrows.p, src.stride,
                                     src_ix->stream));
        SCANN_HIP_CHECK(hipStreamSynchronize(src_ix->stream));
    }
    const float inv = row_format == SCANN_HIP_ROWS_INT8 ? p.scale : 1.0f;
    scann_hip_index *ix = nullptr;
    if (src_ix->kind == KIND_BF) {
        if (row_format == SCANN_HIP_ROWS_INT8 && !std::isfinite(inv))
            return fail(SCANN_HIP_INVALID_ARGUMENT, "inv_multiplier is not finite");
        ix = new scann_hip_index();
        ix->ctx = src_ix->ctx;
        ix->kind = KIND_BF;
        ix->bf_rows.take(qrows);
        int s = index_common_init(ix);
        if (s == SCANN_HIP_OK) s = bf_finish_quantized(ix, src.n, src.dim, src.stride, row_format, inv, src.measure);
        if (s != SCANN_HIP_OK) {
            scann_hip_index_destroy(ix);
            return s;
        }
    } else {
        IndexHostArrays arrays;   // centres, CSR, codes, codebook: small next to the rows, which stay on the device
        SCANN_TRY(index_download(src_ix, &arrays, false));
        SCANN_TRY(txh_quantized_args(&arrays.d, qrows.p, row_format, inv));
        SCANN_TRY(txh_create_checked(src_ix->ctx, &arrays.d, &ix, SCANN_HIP_INTERNAL, nullptr, row_format, inv, &qrows));
    }
    if (out_params4) {
        out_params4[0] = p.mn;
        out_params4[1] = p.mx;
        out_params4[2] = p.scale;
        out_params4[3] = p.inv_scale;
    }
    if (out_zero_point) *out_zero_point = zp;
    *out = ix;
    return SCANN_HIP_OK;
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

// ---- per-call planning --------------------------------------------------------------
static uint64_t max_stream(const scann_hip_index *ix, uint32_t P) {
    uint64_t s = 0;
    for (uint32_t i = 0; i < P && i < ix->local_sizes_desc.size(); ++i) s += ix->local_sizes_desc[i];
    return s;
}

// One-launch forms of the small and wide pipelines: stream positions per workgroup and workgroups per query.
static void plan_small_launch(const TxhIndexDev &t, const Knobs &kn, TxhPlan *p) {
    if (p->pipeline == TxhPipeline::Wide) {
        // 1024 x rep stream positions per workgroup, rep <= kWideRep chosen so that one wave of workgroups (256 CUs)
        // covers the stream.  (ADC scans only: an exact scan wants a row per thread and ~128 rows per workgroup --
        // hundreds of workgroups per query that would each repeat the leaf selection; Partitioned mode keeps the small
        // pipeline.)
        p->chunk = kFusedChunk * std::min<uint32_t>(kWideRep, std::max(1u, ceil_div_u32(p->cap, 256u * kFusedChunk)));
        p->grid = std::max(1u, ceil_div_u32(p->cap, p->chunk));
        p->fused = false;
        return;
    }
    // One launch when the grid stays small (SCANN_HIP_FUSED=0: always three).  Exact scans read a whole row per
    // thread, 64 cache lines per wave instruction: they are bound by the L1's line-request rate of ONE compute unit,
    // so their workgroups take only 128 positions each (more compute units share the rows); ADC scans read 16
    // coalesced code bytes per point and take 1024 -- but rebuild the tables per leaf one after the other, so tree
    // indexes with several leaves per query keep the three-launch form, whose scan builds every leaf's table in its
    // own workgroup.
    p->chunk = kFusedChunk;
    if (t.exact_scan) p->chunk = std::min(kFusedChunk, std::max(128u, (ceil_div_u32(p->cap, 256u) + 127u) & ~127u));
    p->grid = std::max(1u, ceil_div_u32(p->cap, p->chunk));
    p->fused = kn.fused && p->P <= kDecodeStage && (uint64_t)p->nq * p->grid <= kFusedMaxWgs &&
               (t.exact_scan || p->P == 1);
}

// Every path decision of a tree / AH search of nq queries.  retry: the host entry's second attempt after a
// threshold or buffer miss -- a candidate slot for every scanned point, and not the wide pipeline.  widest: the
// widest pipeline the caller takes (Staged for callers that only size buffers or run the local stage).
static int plan_txh_search(const scann_hip_index *ix, uint32_t k, const scann_hip_search_opts *o, uint32_t nq,
                           bool retry, TxhPipeline widest, const Knobs &kn, TxhPlan *out) {
    scann_hip_search_opts def;
    scann_hip_search_opts_default(&def);
    if (!o) o = &def;
    const TxhIndexDev &t = ix->tx;
    bool full_cap = retry;
    if (retry && widest == TxhPipeline::Wide) widest = TxhPipeline::Small;
    // rows stored quantized: the small and wide pipelines re-rank inside their finish kernels from f32 rows, so every
    // batch size takes the staged pipeline, whose re-rank is a kernel of its own
    if (t.qfmt) widest = TxhPipeline::Staged;
    // projected handles: the few-query pipelines re-rank inside kernels that read one query space
    if (ix->proj.kind) widest = TxhPipeline::Staged;
    uint32_t P = o->partitions_to_search ? o->partitions_to_search : ix->default_P;
    P = std::min(P, t.L);  // tree_partitioner.rs:214
    if (t.ah_mode) P = 1;
    if (P > kMaxPartitionsToSearch)
        return fail(SCANN_HIP_UNIMPLEMENTED, "partitions_to_search > 4096");
    const bool exact_reorder = o->exact_reorder && !t.exact_scan;   // the scan's distances ARE exact
    if (t.exact_scan) {
        full_cap = true;   // dense key lists: one slot per scanned row, no threshold
        if (o->allow_bitmap) return fail(SCANN_HIP_UNIMPLEMENTED, "the exact leaf scan takes no filter");
    }
    uint32_t m;
    if (!exact_reorder) {
        m = k;
    } else if (o->pre_reorder_k) {
        m = o->pre_reorder_k;
    } else {
        const float mf = (float)k * ix->multiplier;  // mod.rs:263 (saturating truncation)
        m = mf > 0.0f ? (mf >= 4294967295.0f ? 0xFFFFFFFFu : (uint32_t)mf) : 0u;
    }
    if (m > kMaxPreReorderK)
        return fail(SCANN_HIP_UNIMPLEMENTED,
                    "pre-reorder candidate count " + std::to_string(m) + " exceeds " +
                        std::to_string(kMaxPreReorderK));
    if (exact_reorder && !t.rows && !t.qrows)  // hasher.rs:194-197
        return fail(SCANN_HIP_FAILED_PRECONDITION, "Dataset not stored");
    const uint64_t stream = std::max<uint64_t>(1, max_stream(ix, P));
    const uint64_t ms = std::min<uint64_t>(stream, 0xFFFFFFFFull);
    TxhPlan p{};
    p.nq = nq;
    p.P = P;
    p.m = m;
    p.k = k;
    p.exact_reorder = exact_reorder;
    sample_plan(ms, P, &p.st, &p.scap);
    // A handful of queries over a short stream: three launches with dense candidate lists instead of
    // the batched pipeline (SCANN_HIP_SMALL=0 disables).  Unsharded indexes only: stream positions are
    // list slots, and a shard's local leaves leave holes in them.
    p.pipeline = TxhPipeline::Staged;
    if (widest != TxhPipeline::Staged && kn.small && nq <= kSmallBatch && !ix->sharded && m <= kSmallMaxCandidates &&
        k <= 64 && ms <= kSmallMaxStream && t.L <= 4096 && (!t.exact_scan || txh_exact_scan_fits(t)))
        p.pipeline = TxhPipeline::Small;
    // Fewer queries still, over a long stream: the wide pipeline (three launches, every stage spread over the chip).
    // Its scan rebuilds the tables per leaf inside a workgroup of 1024 stream positions: leaves of >= 512 points
    // (or one leaf); ADC scans only (Partitioned mode, 4 queries over 20 leaves of 1M x 128: 0.097 ms on the small-batch
    // pipeline, 0.147 through this one).  Streams of >= 8 m points: below that most of the stream is candidates anyway.
    // SCANN_HIP_WIDE: 0 = never, 2 = whenever the limits allow (tests), else from kWideMinStream points.
    {
        const bool limits = widest == TxhPipeline::Wide && kn.small && kn.wide != 0 && nq <= kWideBatch &&
                            !ix->sharded && m >= 1 && m <= kWideMaxCandidates && k <= 64 && ms <= kWideMaxStream &&
                            t.L <= 4096 && P <= 512 && !t.exact_scan;
        const bool long_leaves = P == 1 || t.n_local / std::max(1u, t.L) >= 512;
        const bool pays = ms >= kWideMinStream && ms >= 8ull * m && long_leaves;
        if (limits && (kn.wide == 2 || pays)) {
            p.pipeline = TxhPipeline::Wide;
            p.wide_cap2 = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(ms, 3ull * m + 1024), 16384);
        }
    }
    if (p.pipeline != TxhPipeline::Staged) full_cap = true;
    uint64_t cap = ms;
    if (!full_cap) {
        // upper bound of the survivors of the sampled threshold (rank j of a stride-st sample)
        const uint32_t j = sample_rank(m, p.st);
        cap = (uint64_t)((double)j + 8.0 * std::sqrt((double)j) + 16.0) * p.st + 256;
        cap = std::min(std::max<uint64_t>(cap, m), ms);
    }
    p.cap = (uint32_t)std::min<uint64_t>(cap, 0xFFFFFFFFull);
    p.no_threshold = full_cap;
    p.small_max_leaf = ix->local_sizes_desc.empty() ? 0u : ix->local_sizes_desc[0];
    if (p.pipeline != TxhPipeline::Staged) plan_small_launch(t, kn, &p);

    const uint32_t L = t.L;
    // sample tiles: enough of them to fill the chip (the sample pass is 1/st of the scan)
    const uint64_t quads = ((uint64_t)nq * P + 3) / 4;
    const uint32_t tp = scan_tile_points(t);
    const uint64_t chunks = std::max<uint64_t>(1, ((uint64_t)p.scap + tp - 1) / tp);
    p.sqpt = kScanQuadsPerTile;
    while (p.sqpt > 2 && chunks * ((quads + p.sqpt - 1) / p.sqpt) < 4096) p.sqpt >>= 1;
    // scan tiles: the largest quad group that still yields ~4 tiles per resident workgroup
    // (small shards and small batches would otherwise leave most of the chip idle)
    const uint64_t all_chunks = t.n_local / tp + L;
    const uint64_t quads_per_leaf = std::max<uint64_t>(1, quads / std::max(1u, L));
    p.qpt = kScanQuadsPerTile;
    while (p.qpt > 8 && all_chunks * ((quads_per_leaf + p.qpt - 1) / p.qpt) < 6144) p.qpt >>= 1;
    // long leaves scanned by many queries (AsymmetricHasher mode, few big partitions): tables
    // resident in LDS over a range of chunks (adc_scan_res_kernel); needs 4-bit codes with
    // S <= 32.  With few quads per leaf (typical Tree-X-Hybrid batches: measured at 10M / 1000
    // leaves) the per-chunk kernel is as fast or faster.
    const uint64_t rtp = (uint64_t)kResThreads * kScanPPT;
    const uint64_t res_chunks_per_leaf = std::max<uint64_t>(1, (t.n_local / std::max(1u, L)) / rtp);
    const uint64_t qgroups = std::max<uint64_t>(1, (quads_per_leaf + kResQuads - 1) / kResQuads);
    const uint64_t units = (t.n_local / rtp + L) * qgroups;       // (chunk, quad group) pairs
    // a tile must cover >= 8 chunks to amortise its table load, and there must be >= 2 tiles
    // per resident workgroup (small shards: measured at 125k-500k rows)
    p.res_cl = (uint32_t)std::min<uint64_t>(64, std::max<uint64_t>(8, units / 4096));
    const bool res_layout = t.code_bits == 4 && t.S <= 32;
    bool resident = res_layout && res_chunks_per_leaf >= 8 && quads_per_leaf >= 32 && units / p.res_cl >= 1536;
    // SCANN_HIP_RESIDENT: 0 = never, 2 = whenever the code layout allows (tests), else the heuristic
    if (kn.resident == 0) resident = false;
    if (kn.resident == 2) resident = res_layout;
    if (kn.res_cl) p.res_cl = kn.res_cl;
    // Integer-MFMA prefilter + exact refine (txh_prefilter.hip K6d): 4-bit codes, a filter bound to prove
    // against, and enough pairs per leaf to fill 32-column MFMA tiles (a leaf scanned by few
    // queries would leave most columns empty; the LDS-gather kernels take those).
    // Leaves scanned by 8-24 queries (2-5 quads: typical Tree-X-Hybrid batches) take the 16-column form
    // (adc_mfma16_kernel); fewer than that and the LDS-gather kernel wins.
    const bool mfma_ok = t.code_bits == 4 && !p.no_threshold && !t.exact_scan;
    // The prefilter pays while the wanted candidates are a small share of the scanned stream: every
    // survivor (~1.5-2.4 m) is staged, flushed and recomputed by the refine.  Measured: 1M x 128 flat,
    // m = 5000 (0.5 %): 2.7x faster than the gather scan; 10M x 128 / 1000 leaves, m / stream 0.1-0.6 %:
    // steps 1.1-1.4x faster; 1-3 % (P = 10 or 25 with m = 8192): 1.1-1.2x slower.
    const bool sparse = (uint64_t)m * 128 <= stream;
    TxhScan mfma = TxhScan::Gather;   // (Gather: no prefilter)
    if (mfma_ok && sparse) mfma = quads_per_leaf >= 6 ? TxhScan::Mfma32 : quads_per_leaf >= 2 ? TxhScan::Mfma16 : TxhScan::Gather;
    // SCANN_HIP_MFMA: 0 = never, 2 / 3 = the 32- / 16-column form whenever the code layout allows (tests),
    // else the heuristic
    if (kn.mfma == 0) mfma = TxhScan::Gather;
    if (kn.mfma == 2) mfma = mfma_ok ? TxhScan::Mfma32 : TxhScan::Gather;
    if (kn.mfma == 3) mfma = mfma_ok ? TxhScan::Mfma16 : TxhScan::Gather;
    // With the operand planes in the index the 32-pair form runs on the 2:4-sparse MFMA (SCANN_HIP_SMFMAC=0 at this
    // call keeps the dense instruction: tests compare the two) -- and takes over from 8 pairs per leaf, whatever
    // m / stream is: at 10M x 128, 1000 leaves, 1024 queries, P = 10 (10 pairs per leaf: tiles a third full)
    // m = 1000 / 4000 / 8192 run 0.68 / 0.95 / 1.29 ms per step on it against 0.88 / 1.09 / 1.61 ms on the 16-pair
    // dense form / the f32 gather scan the rules above pick (P = 25 / 50 / 100 at m = 1000: 0.94 / 1.11 / 1.44 ms
    // against round 2's 1.12 / 1.41 / 1.91).
    // (long leaves only -- an item is up to 2048 points of a leaf, and its fixed costs, the table fragments and the
    // flush, want most of that: at 1M x 128 / 1000 leaves of 1000 points the gather scan's 0.08 ms beats 0.13 ms)
    if (mfma_ok && t.codes_sp && quads_per_leaf >= 2 && t.n_local / std::max(1u, L) >= 4096 && kn.smfmac &&
        kn.mfma != 0 && kn.mfma != 3)
        mfma = TxhScan::Smfmac;
    if (mfma == TxhScan::Mfma32 && t.codes_sp && kn.smfmac) mfma = TxhScan::Smfmac;   // (forced 32-pair form, fewer pairs per leaf)
    p.scan = t.exact_scan ? TxhScan::Exact : mfma != TxhScan::Gather ? mfma : resident ? TxhScan::Resident : TxhScan::Gather;
    if (txh_scan_is_mfma(p.scan)) {
        // survivors of the integer bound: the f32 filter's (<= cap) plus the quantisation margin
        // (the margin's share is independent of m -- the points within 17 table steps above the bound -- and in
        // the dense nearest leaves of a tree index it can be several thousand: a generous floor)
        p.cap32 = (uint32_t)std::min<uint64_t>(ms, (uint64_t)p.cap * 4 + 16384);
    }
    // the sparse kernel's flush: lanes walk their own words on flat hashers, word-parallel on tree indexes
    p.sp_words = kn.sp_words < 0 ? !t.ah_mode : kn.sp_words != 0;
    // ... and its items: 64 pairs x 1024 points (two column tiles share every point tile's operands) where that form is
    // compiled -- S <= 32, lane-walk flush -- on flat hashers whose padding costs at most about one column tile in eight:
    // an even number of 32-pair tiles, or more than 224 queries.  SCANN_HIP_SP_PAIRS = 32 / 64 forces a form.
    {
        const bool compiled = p.scan == TxhScan::Smfmac && t.S <= 32 && !p.sp_words;
        const uint64_t tiles32 = (quads + 7) / 8;
        const bool flat = t.ah_mode && L == 1 && P == 1;
        p.sp_pairs64 = compiled && (kn.sp_pairs ? kn.sp_pairs == 64 : flat && (tiles32 % 2 == 0 || nq > 224));
    }
    // ... which, on a flat hasher, end by storing the item's survivor bitmap as it stands in LDS (128 bytes per query and
    // 1024 points) and leave the walk over its bits to the refine (adc_smfmac_bits_kernel64, adc_refine_bits_kernel): no
    // lists, no atomics and no gathers in the kernel that runs at two waves per SIMD.  The bitmap is rewritten whole by
    // every call, so its size is bounded: kSurvBytesMax covers a batch of 4096 queries over 1M points (489 MiB).
    // SCANN_HIP_SP_BITMAP = 0 keeps the flush inside the scan.  (A forced 64-pair form on a tree index keeps it too.)
    // Every batch size that runs 64-pair items takes the form: it won the sweep at 64, 256 and 1024 queries.
    {
        constexpr uint64_t kSurvBytesMax = 512ull << 20;
        const uint64_t nranges = ((uint64_t)t.n_local + kSpRange64 - 1) / kSpRange64;
        const uint64_t rows = ((uint64_t)nq + 63) / 64 * 64;
        const bool flat = t.ah_mode && L == 1 && P == 1;
        p.surv_stride = (uint32_t)(nranges * 32);
        p.sp_bitmap = p.sp_pairs64 && flat && kn.sp_bitmap && rows * nranges * 128 <= kSurvBytesMax;
    }
    // The survivors' codes travel with their positions for flat hashers: their ~12 k survivors per query
    // are spread over the whole code array (random 16-byte gathers from 16 MB: refine 145 -> 65 us at
    // C3).  In a tree index the survivors sit densely in the query's nearest leaves, the gathers hit
    // L2, and writing the codes only costs the scan (10M x 128, P = 25 / 50: step +3.5 %).
    p.codes_in_list = t.ah_mode != 0;
    p.thr_ties = kn.thr_ties;
    // a bound in the low tail of a long sample: threshold_tail_kernel
    p.thr_tail = kn.thr_tail && !p.no_threshold && sample_rank(m, p.st) <= kThrTailMaxRank && p.scap > 4096;
    // ... of a flat hasher in front of an MFMA prefilter: the sample as integer-MFMA sums over the plain quantised
    // tables, the exact f32 arithmetic only on its low tail (adc_sample_mfma_kernel, threshold_tail16_kernel)
    p.sample_mfma = kn.sample_mfma && p.thr_tail && p.thr_ties && txh_scan_is_mfma(p.scan) && t.ah_mode && t.L == 1 &&
                    P == 1 && t.code_bits == 4;
    p.select_direct = kn.select_direct;
    p.select_regs = kn.select_regs;
    // int8 re-rank filter: lists of a few hundred candidates and more
    p.use_i8 = t.rows8 && exact_reorder && m >= kn.rerank_i8_min && m > 4 * k;
    p.i8_expand = kn.rerank_expand;
    p.local_prune = kn.local_prune && !t.qfmt;
    *out = p;
    return SCANN_HIP_OK;
}

// The kernel scann_hip_index_last_kernel_ms names for a search run on `p` over `t`.  pinned: the host entry's small /
// wide pipeline with queries and results in pinned memory; every other call is named by its batched-pipeline scan
// (also when a device entry point or staged outputs run it on a small pipeline).
static const char *txh_kernel_name(const TxhIndexDev &t, const TxhPlan &p, bool pinned) {
    if (pinned) return p.pipeline == TxhPipeline::Wide ? "wide_scan_kernel" : "small_scan_kernel";
    switch (p.scan) {
        case TxhScan::Exact: return "leaf_exact_scan_kernel";
        case TxhScan::Mfma16: return "adc_mfma16_kernel";
        case TxhScan::Smfmac: return t.S > 32 ? "adc_smfmac_wide_kernel" : "adc_smfmac_kernel";
        case TxhScan::Mfma32: return "adc_mfma_kernel";
        case TxhScan::Resident: return "adc_scan_res_kernel";
        default: return "adc_scan_kernel";
    }
}

}  // extern "C"

int scann::txh_resolve_m(scann_hip_index *ix, uint32_t k, const scann_hip_search_opts *opts, uint32_t *out_m) {
    if (!ix || ix->kind != KIND_TXH) return fail(SCANN_HIP_INVALID_ARGUMENT, "not a tree index");
    if (ix->tx.qfmt) return fail(SCANN_HIP_UNIMPLEMENTED, "the leaf-sharded search over quantized rows is not built");
    if (ix->proj.kind) return fail(SCANN_HIP_UNIMPLEMENTED, "the leaf-sharded search through a projection is not built");
    scann_hip_search_opts o;
    if (opts) o = *opts; else scann_hip_search_opts_default(&o);
    o.exact_reorder = 1;
    TxhPlan p;
    SCANN_TRY(plan_txh_search(ix, k, &o, 0, false, TxhPipeline::Staged, read_knobs(), &p));
    *out_m = p.m;
    return SCANN_HIP_OK;
}

extern "C" {

// Buffers of the plan p (the arena re-places everything when one grows), bound into *w.
// allow_bytes: size of an allow-bitmap the caller will copy into s.allow (0 = none)
static int ensure_txh_workspace(scann_hip_index *ix, TxhWorkspace &s, const TxhPlan &p, bool own_queries,
                                uint32_t q_stride, bool own_outputs, TxhWork *w, size_t allow_bytes = 0) {
    const TxhIndexDev &t = ix->tx;
    const uint32_t nq = p.nq, L = t.L, P = p.P, m = std::max(1u, p.m), k = std::max(1u, p.k);
    const uint64_t max_slots64 = (uint64_t)nq * P + 3ull * L + 4;
    if (max_slots64 > 0xFFFFFFF0ull)
        return fail(SCANN_HIP_RESOURCE_EXHAUSTED, "batch x partitions_to_search exceeds the pair table (2^32 slots)");
    const uint32_t max_slots = (uint32_t)max_slots64;
    const uint32_t max_quads = max_slots / 4 + 1;
    const bool mfma = txh_scan_is_mfma(p.scan), small = p.pipeline != TxhPipeline::Staged,
               wide = p.pipeline == TxhPipeline::Wide;
    if (allow_bytes) s.want(s.allow, allow_bytes);
    if (own_queries) s.want(s.queries, (size_t)nq * q_stride * 4);
    if (!t.ah_mode) s.want(s.cdist, (size_t)nq * L * 4);
    s.want(s.tokens, (size_t)nq * P * 4);
    s.want(s.token_dists, (size_t)nq * P * 4);
    s.want(s.vbase, (size_t)nq * (P + 1) * 4);
    s.want(s.sbase, (size_t)nq * (P + 2) * 4);
    s.want(s.pair_sbase, (size_t)max_slots * 4);
    s.want(s.stile_off, (size_t)(L + 1) * 4);
    s.want(s.samp, (size_t)nq * p.scap * (p.sample_mfma ? 2 : 4));
    s.want(s.leaf_cnt, (size_t)L * 4);
    s.want(s.leaf_cursor, (size_t)L * 4);
    s.want(s.pair_off, (size_t)(L + 1) * 4);
    s.want(s.tile_off, (size_t)(L + 1) * 4);
    s.want(s.counters, CNT_WORDS * 4);
    s.want(s.pair_q, (size_t)max_slots * 4);
    s.want(s.pair_leaf, (size_t)max_slots * 4);
    s.want(s.pair_vbase, (size_t)max_slots * 4);
    s.want(s.pair_thr, (size_t)max_slots * 8);
    s.want(s.slot_of, (size_t)nq * P * 4);
    s.want(s.lutq, (size_t)max_quads * t.S * t.kp * 4 * 4);
    s.want(s.thr, (size_t)nq * 8);
    s.want(s.cand_cnt, (size_t)nq * 4);
    s.want(s.cand, (size_t)nq * p.cap * 8);
    s.want(s.cand_key, (size_t)nq * m * 8);
    s.want(s.cand_idx, (size_t)nq * m * 4);
    s.want(s.cand_dist, (size_t)nq * m * 4);
    s.want(s.cand_exact, (size_t)nq * m * 4);
    s.want(s.cand_row, (size_t)nq * m * 4);
    s.want(s.cand_count, (size_t)nq * 4);
    if (own_outputs) {
        s.want(s.out_idx, (size_t)nq * k * 4);
        s.want(s.out_dist, (size_t)nq * k * 4);
        s.want(s.out_count, (size_t)nq * 4);
    }
    if (p.use_i8) {
        s.want(s.rr_lb, (size_t)nq * m * 4);
        s.want(s.rr_ub, (size_t)nq * m * 4);
    }
    if (mfma) {
        s.want(s.lut8, (size_t)max_slots * t.S * 16 + 64);
        s.want(s.lut8_meta, (size_t)(max_slots + 4) * 16);
        s.want(s.mfma_thr1, (size_t)(max_slots + 4) * 4);
        if (p.sp_bitmap) {   // survivor bitmaps instead of lists
            s.want(s.surv, ((size_t)nq + 63) / 64 * 64 * p.surv_stride * 4);
        } else {
            s.want(s.cand32, (size_t)nq * p.cap32 * 4);
            // flat hashers: the survivors' packed codes (dense prefilter) or plane rows (sparse prefilter) travel with them
            if (t.ah_mode)
                s.want(s.cand32_codes, (size_t)nq * p.cap32 * std::max(t.S / 8, p.scan == TxhScan::Smfmac ? sp_words(t.S) : 0u) * 4);
            s.want(s.cand32_cnt, (size_t)nq * 4);
        }
    }
    if (small) s.want(s.small_tickets, 64 * 4);
    if (ix->proj.kind) s.want(s.proj_q, (size_t)nq * t.dim * 4);
    if (wide) {
        s.want(s.wide_min, (size_t)nq * p.cap * 4);
        s.want(s.wide_ckey, (size_t)nq * p.wide_cap2 * 8);
        s.want(s.wide_ceb, (size_t)nq * p.wide_cap2 * 4);
        s.want(s.wide_cidx, (size_t)nq * p.wide_cap2 * 4);
        s.want(s.wide_cnt, 64 * 4);
    }
    SCANN_TRY(s.commit());
    *w = TxhWork{};
    static_cast<TxhPlan &>(*w) = p;
    w->q_stride = q_stride;
    w->queries = s.queries.as<float>();
    w->cdist = s.cdist.as<float>();
    w->tokens = s.tokens.as<uint32_t>();
    w->token_dists = s.token_dists.as<float>();
    w->vbase = s.vbase.as<uint32_t>();
    if (p.use_i8) {
        w->rr_lb = s.rr_lb.as<uint32_t>();
        w->rr_ub = s.rr_ub.as<uint32_t>();
    }
    if (mfma) {
        w->lut8 = s.lut8.as<int8_t>();
        w->lut8_meta = s.lut8_meta.p;
        w->mfma_thr1 = s.mfma_thr1.as<int>();
        if (p.sp_bitmap) {
            w->surv = s.surv.as<uint32_t>();
        } else {
            w->cand32 = s.cand32.as<uint32_t>();
            w->cand32_codes = t.ah_mode ? s.cand32_codes.as<uint32_t>() : nullptr;
            w->cand32_cnt = s.cand32_cnt.as<uint32_t>();
        }
    }
    if (small) w->small_tickets = s.small_tickets.as<uint32_t>();
    if (ix->proj.kind) w->proj_q = s.proj_q.as<float>();
    if (wide) {
        w->wide_min = s.wide_min.as<uint32_t>();
        w->wide_ckey = s.wide_ckey.as<uint64_t>();
        w->wide_ceb = s.wide_ceb.as<uint32_t>();
        w->wide_cidx = s.wide_cidx.as<uint32_t>();
        w->wide_cnt = s.wide_cnt.as<uint32_t>();
    }
    w->sbase = s.sbase.as<uint32_t>();
    w->pair_sbase = s.pair_sbase.as<uint32_t>();
    w->stile_off = s.stile_off.as<uint32_t>();
    w->samp = s.samp.as<uint32_t>();
    w->leaf_cnt = s.leaf_cnt.as<uint32_t>();
    w->leaf_cursor = s.leaf_cursor.as<uint32_t>();
    w->pair_off = s.pair_off.as<uint32_t>();
    w->tile_off = s.tile_off.as<uint32_t>();
    w->counters = s.counters.as<uint32_t>();
    w->pair_q = s.pair_q.as<uint32_t>();
    w->pair_leaf = s.pair_leaf.as<uint32_t>();
    w->pair_vbase = s.pair_vbase.as<uint32_t>();
    w->pair_thr = s.pair_thr.as<uint64_t>();
    w->slot_of = s.slot_of.as<uint32_t>();
    w->max_slots = max_slots;
    w->max_quads = max_quads;
    w->lutq = s.lutq.as<float>();
    w->thr = s.thr.as<uint64_t>();
    w->cand_cnt = s.cand_cnt.as<uint32_t>();
    w->cand = s.cand.as<uint64_t>();
    w->cand_key = s.cand_key.as<uint64_t>();
    w->cand_idx = s.cand_idx.as<uint32_t>();
    w->cand_dist = s.cand_dist.as<float>();
    w->cand_exact = s.cand_exact.as<float>();
    w->cand_row = s.cand_row.as<uint32_t>();
    w->cand_count = s.cand_count.as<uint32_t>();
    w->out_idx = s.out_idx.as<uint32_t>();
    w->out_dist = s.out_dist.as<float>();
    w->out_count = s.out_count.as<uint32_t>();
    return SCANN_HIP_OK;
}

// txh_launch_search on a handle that may be projected.  A projected handle first writes qp = project(q) into the
// workspace's proj_q at the head of the stream; the pipeline then runs on qp at dim = out_dim, and the re-rank alone
// reads the caller's queries (w.rr_queries).  Any other handle: txh_launch_search as it was.
static int launch_txh(const scann_hip_index *ix, TxhWork &w, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
    if (ix->proj.kind && w.nq) {
        SCANN_TRY(launch_project(ix->proj, w.queries, w.nq, w.q_stride, w.proj_q, ix->tx.dim, st));
        w.rr_queries = w.queries;
        w.rr_q_stride = w.q_stride;
        w.queries = w.proj_q;
        w.q_stride = ix->tx.dim;
    }
    return txh_launch_search(ix->tx, w, false, st, ev0, ev1);
}

static void fill_empty(uint32_t nq, uint32_t k, uint32_t *out_idx, float *out_dist,
                       uint32_t *out_count) {
    for (size_t i = 0; i < (size_t)nq * k; ++i) {
        if (out_idx) out_idx[i] = 0xFFFFFFFFu;
        if (out_dist) out_dist[i] = INFINITY;
    }
    for (uint32_t i = 0; i < nq; ++i)
        if (out_count) out_count[i] = 0;
}

// ---- workspaces of the device entry points: one per caller stream (ix->mu held) ---------------------------------
static int device_slot_count() {
    static const int v = std::max(1, std::min((int)scann_hip_index::kMaxDeviceSlots, read_knobs().device_slots));
    return v;
}

// The workspace of a call that will be enqueued on `st`: the one bound to that stream, else an unused one, else the
// least recently used one -- ordered behind its previous stream's last call.
static int device_slot(scann_hip_index *ix, hipStream_t st, scann_hip_index::DeviceSlot **out) {
    auto &ds = ix->dslots;
    if (!ds[0].ws) {
        ds[0].ws = &ix->ws;
        ds[0].bfw = &ix->bfw;
        ds[0].crowd = &ix->crowd;
    }
    const int n = device_slot_count();
    scann_hip_index::DeviceSlot *pick = nullptr;
    for (int i = 0; i < n && !pick; ++i)
        if (ds[i].used && ds[i].key == st) pick = &ds[i];
    for (int i = 0; i < n && !pick; ++i)
        if (!ds[i].used) pick = &ds[i];
    if (!pick) {
        pick = &ds[0];
        for (int i = 1; i < n; ++i)
            if (ds[i].tick < pick->tick) pick = &ds[i];
    }
    if (!pick->ws) {
        pick->ws_own.reset(new TxhWorkspace());
        pick->bfw_own.reset(new BfWorkspace());
        pick->ws = pick->ws_own.get();
        pick->bfw = pick->bfw_own.get();
        pick->crowd_own.reset(new CrowdWorkspace());
        pick->crowd = pick->crowd_own.get();
    }
    if (!pick->done) SCANN_HIP_CHECK(hipEventCreateWithFlags(&pick->done, hipEventDisableTiming));
    if (pick->used && pick->key != st && pick->done_valid) SCANN_HIP_CHECK(hipStreamWaitEvent(st, pick->done, 0));
    pick->used = true;
    pick->key = st;
    pick->tick = ++ix->dslot_tick;
    *out = pick;
    return SCANN_HIP_OK;
}

// after the call's last enqueue on `st`
static int device_slot_done(scann_hip_index::DeviceSlot *sl, hipStream_t st) {
    SCANN_HIP_CHECK(hipEventRecord(sl->done, st));
    sl->done_valid = true;
    return SCANN_HIP_OK;
}

// Host-side users of the primary workspace (they run on ix->stream and synchronise before they return): wait for a
// device-entry call that may still be using it on another stream.
static int claim_primary_workspace(scann_hip_index *ix) {
    auto &d0 = ix->dslots[0];
    if (d0.used && d0.key != ix->stream) {
        if (d0.done_valid) SCANN_HIP_CHECK(hipStreamWaitEvent(ix->stream, d0.done, 0));
        d0.used = false;
        d0.done_valid = false;
        d0.key = nullptr;
    }
    return SCANN_HIP_OK;
}

// A search slot for a host-side call: the primary one if it is free, else a free extra slot (created
// up to SCANN_HIP_SEARCH_SLOTS, default 4, streams + workspaces in total), else wait for the primary.
struct SlotLock {
    std::unique_lock<std::mutex> lock;
    hipStream_t stream = nullptr;
    TxhWorkspace *ws = nullptr;
    BfWorkspace *bfw = nullptr;
    CrowdWorkspace *crowd = nullptr;
    PinBuf *pin = nullptr;
    bool primary = false;
};

static uint32_t max_slots() {
    static const uint32_t v = read_knobs().search_slots;
    return v;
}

static int acquire_slot(scann_hip_index *ix, SlotLock *out) {
    std::unique_lock<std::mutex> lk(ix->mu, std::try_to_lock);
    if (!lk.owns_lock()) {
        SearchSlot *slot = nullptr;
        {
            std::lock_guard<std::mutex> g(ix->slots_mu);
            for (auto &sl : ix->slots) {
                std::unique_lock<std::mutex> l2(sl->mu, std::try_to_lock);
                if (l2.owns_lock()) {
                    slot = sl.get();
                    out->lock = std::move(l2);
                    break;
                }
            }
            if (!slot && ix->slots.size() + 1 < max_slots()) {
                std::unique_ptr<SearchSlot> ns(new SearchSlot());
                SCANN_TRY(set_device(ix->ctx));
                SCANN_HIP_CHECK(hipStreamCreateWithFlags(&ns->stream, hipStreamNonBlocking));
                out->lock = std::unique_lock<std::mutex>(ns->mu);
                slot = ns.get();
                ix->slots.push_back(std::move(ns));
            }
        }
        if (slot) {
            out->stream = slot->stream;
            out->ws = &slot->ws;
            out->bfw = &slot->bfw;
            out->crowd = &slot->crowd;
            out->pin = &slot->pin;
            out->primary = false;
            return SCANN_HIP_OK;
        }
        lk.lock();   // every slot busy: queue on the primary
    }
    out->lock = std::move(lk);
    SCANN_TRY(claim_primary_workspace(ix));
    out->stream = ix->stream;
    out->ws = &ix->ws;
    out->bfw = &ix->bfw;
    out->crowd = &ix->crowd;
    out->pin = &ix->pin;
    out->primary = true;
    return SCANN_HIP_OK;
}

// Completion of a small-batch call whose last kernel stores `seq` into the nq pinned flag words after
// its result rows (system-scope release): the host polls the flags instead of paying the wake-up
// latency of hipStreamSynchronize for a 30-microsecond job.  Falls back to the stream synchronise after
// ~2 ms without completion (long jobs, or a launch that failed: the synchronise reports it).
static int wait_small_done(hipStream_t stream, const volatile uint32_t *flags, uint32_t nq, uint32_t seq) {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spin = 0;; ++spin) {
        bool all = true;
        for (uint32_t i = 0; i < nq; ++i)
            if (flags[i] != seq) {
                all = false;
                break;
            }
        if (all) {
            std::atomic_thread_fence(std::memory_order_acquire);
            return SCANN_HIP_OK;
        }
        if ((spin & 255u) == 255u &&
            std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(2000))
            break;
        __builtin_ia32_pause();
    }
    SCANN_HIP_CHECK(hipStreamSynchronize(stream));
    return SCANN_HIP_OK;
}

static int txh_search_host(scann_hip_index *ix, const float *queries, uint32_t nq,
                           uint32_t q_stride, uint32_t k, const scann_hip_search_opts *opts,
                           uint32_t *out_idx, float *out_dist, uint32_t *out_count) {
    SlotLock sl;
    SCANN_TRY(acquire_slot(ix, &sl));
    TxhWorkspace &ws = *sl.ws;
    const hipStream_t stream = sl.stream;
    SCANN_TRY(set_device(ix->ctx));
    const Knobs kn = read_knobs();
    SCANN_TRY(check_allow_stride(opts));
    for (int attempt = 0; attempt < 2; ++attempt) {
        TxhPlan p;
        SCANN_TRY(plan_txh_search(ix, k, opts, nq, /*retry=*/attempt == 1, TxhPipeline::Wide, kn, &p));
        if (p.m == 0) {  // nothing can be kept (reference panics on FastTopNeighbors::new(0))
            fill_empty(nq, k, out_idx, out_dist, out_count);
            if (opts && opts->cand_count) std::memset(opts->cand_count, 0, (size_t)nq * 4);
            return SCANN_HIP_OK;
        }
        TxhWork w;
        // (a filter of capacity 0 still binds a workspace bitmap -- of one word, read by no row -- so that it allows
        // nothing whatever an earlier call left in the workspace: a null bitmap would allow every row)
        const bool filtered = opts && opts->allow_bitmap;
        // (per-query bitmaps: nq of them, allow_bitmap_stride words apart; the repeat below uploads them again)
        const size_t allow_words = filtered ? allow_copy_words(opts, nq) : 0;
        SCANN_TRY(ensure_txh_workspace(ix, ws, p, true, q_stride, true, &w, filtered ? std::max<size_t>(allow_words, 1) * 8 : 0));
        // (cand_count alone also takes the staged pipeline: the small-batch one keeps no candidate counts)
        w.need_sorted_cands = (opts && (opts->cand_idx || opts->cand_dist || opts->cand_count)) ? 1 : 0;
        const bool stage_outputs = opts && (opts->tokens || opts->token_dists || opts->cand_idx || opts->cand_dist ||
                                            opts->cand_count);
        if (p.pipeline != TxhPipeline::Staged && !stage_outputs && !filtered) {
            // small batch: queries and result rows live in pinned host memory the kernels access in place
            const size_t qb = (size_t)nq * q_stride * 4, ob = (size_t)nq * k * 4;
            const size_t off_idx = (qb + 255) & ~(size_t)255, off_dist = off_idx + ((ob + 255) & ~(size_t)255),
                         off_cnt = off_dist + ((ob + 255) & ~(size_t)255);
            const size_t off_flag = off_cnt + (((size_t)nq * 4 + 255) & ~(size_t)255);
            SCANN_TRY(sl.pin->ensure(off_flag + (size_t)nq * 4 + 256));
            char *hp = static_cast<char *>(sl.pin->host), *dp = static_cast<char *>(sl.pin->dev);
            std::memcpy(hp, queries, qb);
            const uint32_t seq = ++sl.pin->seq ? sl.pin->seq : ++sl.pin->seq;   // (never 0)
            // The flag words sit wherever THIS call's layout puts them: an earlier call (other nq / k / stride) may
            // have left result words there, and any of those can equal seq.  Zero them before the launch.
            std::memset(hp + off_flag, 0, (size_t)nq * 4);
            w.queries = reinterpret_cast<const float *>(dp);
            w.out_idx = reinterpret_cast<uint32_t *>(dp + off_idx);
            w.out_dist = reinterpret_cast<float *>(dp + off_dist);
            w.out_count = reinterpret_cast<uint32_t *>(dp + off_cnt);
            w.small_done = reinterpret_cast<uint32_t *>(dp + off_flag);
            w.small_seq = seq;
            if (sl.primary) ix->next_events();
            SCANN_TRY(txh_launch_search(ix->tx, w, false, stream, sl.primary ? ix->ev0 : nullptr,
                                        sl.primary ? ix->ev1 : nullptr));
            if (sl.primary) {
                ix->timing_valid = ix->timing;
                ix->timed_kernel = txh_kernel_name(ix->tx, p, /*pinned=*/true);
            }
            SCANN_TRY(wait_small_done(stream, reinterpret_cast<const volatile uint32_t *>(hp + off_flag), nq, seq));
            if (p.pipeline == TxhPipeline::Wide) {   // the wide pipeline's compact arrays can overflow: count row 0xFFFFFFFF -> the batched pipeline
                bool overflow = false;
                for (uint32_t i = 0; i < nq; ++i) overflow = overflow || reinterpret_cast<const uint32_t *>(hp + off_cnt)[i] == 0xFFFFFFFFu;
                if (overflow) continue;
            }
            std::memcpy(out_idx, hp + off_idx, ob);
            std::memcpy(out_dist, hp + off_dist, ob);
            std::memcpy(out_count, hp + off_cnt, (size_t)nq * 4);
            return SCANN_HIP_OK;   // (dense candidate lists: the three-launch / one-launch forms have no overflow / retry case)
        }
        if (filtered) {   // search_with_filter(Some(allow-list))
            if (allow_words)
                SCANN_HIP_CHECK(hipMemcpyAsync(ws.allow.p, opts->allow_bitmap, allow_words * 8,
                                               hipMemcpyHostToDevice, stream));
            w.allow = ws.allow.as<uint64_t>();
            w.allow_bits = opts->allow_bitmap_bits;
            w.allow_stride = allow_stride_of(opts);
        }
        SCANN_HIP_CHECK(hipMemcpyAsync(ws.queries.p, queries, (size_t)nq * q_stride * 4,
                                       hipMemcpyHostToDevice, stream));
        if (sl.primary) ix->next_events();   // kernel timing follows the primary slot only
        SCANN_TRY(launch_txh(ix, w, stream, sl.primary ? ix->ev0 : nullptr, sl.primary ? ix->ev1 : nullptr));
        if (sl.primary) ix->timing_valid = ix->timing;
        if (sl.primary) ix->timed_kernel = txh_kernel_name(ix->tx, p, /*pinned=*/false);
        uint32_t counters[CNT_N];
        SCANN_HIP_CHECK(hipMemcpyAsync(counters, w.counters, sizeof(counters), hipMemcpyDeviceToHost,
                                       stream));
        SCANN_HIP_CHECK(hipMemcpyAsync(out_idx, w.out_idx, (size_t)nq * k * 4, hipMemcpyDeviceToHost,
                                       stream));
        SCANN_HIP_CHECK(hipMemcpyAsync(out_dist, w.out_dist, (size_t)nq * k * 4,
                                       hipMemcpyDeviceToHost, stream));
        SCANN_HIP_CHECK(hipMemcpyAsync(out_count, w.out_count, (size_t)nq * 4, hipMemcpyDeviceToHost,
                                       stream));
        if (opts) {
            if (opts->tokens)
                SCANN_HIP_CHECK(hipMemcpyAsync(opts->tokens, w.tokens, (size_t)nq * p.P * 4,
                                               hipMemcpyDeviceToHost, stream));
            if (opts->token_dists)
                SCANN_HIP_CHECK(hipMemcpyAsync(opts->token_dists, w.token_dists, (size_t)nq * p.P * 4,
                                               hipMemcpyDeviceToHost, stream));
            if (opts->cand_idx)
                SCANN_HIP_CHECK(hipMemcpyAsync(opts->cand_idx, w.cand_idx, (size_t)nq * p.m * 4,
                                               hipMemcpyDeviceToHost, stream));
            if (opts->cand_dist)
                SCANN_HIP_CHECK(hipMemcpyAsync(opts->cand_dist, w.cand_dist, (size_t)nq * p.m * 4,
                                               hipMemcpyDeviceToHost, stream));
            if (opts->cand_count)
                SCANN_HIP_CHECK(hipMemcpyAsync(opts->cand_count, w.cand_count, (size_t)nq * 4,
                                               hipMemcpyDeviceToHost, stream));
        }
        SCANN_HIP_CHECK(hipStreamSynchronize(stream));
        if (counters[CNT_STATUS] == SCANN_HIP_OK) return SCANN_HIP_OK;
        if ((counters[CNT_STATUS] != SCANN_HIP_RESOURCE_EXHAUSTED &&
             counters[CNT_STATUS] != SCANN_HIP_ABORTED) || attempt == 1)
            return fail((int)counters[CNT_STATUS], "device reported a search failure");
        // candidate buffer overflow, or a statistical threshold that kept fewer than m
        // points: retry once without a threshold and with a buffer for the whole stream
    }
    return fail(SCANN_HIP_INTERNAL, "unreachable");
}

}  // extern "C"

// scann_hip_search_opts.allow_bitmap of a brute-force search (no filter: bitmap null)
static BfFilter bf_filter_of(const scann_hip_search_opts *opts, const Knobs &kn) {
    BfFilter f;
    if (opts && opts->allow_bitmap) {
        f.bitmap = opts->allow_bitmap;
        f.bits = opts->allow_bitmap_bits;
    }
    f.mechanism = kn.bf_filter;
    f.compact_max_fraction = kn.bf_filter_compact_max;
    return f;
}

// BruteForceSearcher::search for a handful of queries over a small dataset: the three-launch pipeline of
// txh.hip ("Small batches") on the one-leaf exact-scan view of the rows -- every distance with the
// one-to-many kernels' arithmetic, the k smallest (distance, index) keys = TopK -- with queries and result
// rows in pinned host memory (no copy commands).
static int bf_small_search_host(scann_hip_index *ix, SlotLock &sl, const float *queries, uint32_t nq,
                                uint32_t q_stride, uint32_t k, const Knobs &kn, const BfFilter &flt, uint32_t *out_idx,
                                float *out_dist, uint32_t *out_count) {
    TxhWorkspace &ws = *sl.ws;
    const uint32_t n = (uint32_t)ix->bf.n, kk = std::min(k, n);
    ws.want(ws.tokens, (size_t)nq * 4);
    ws.want(ws.token_dists, (size_t)nq * 4);
    ws.want(ws.vbase, (size_t)nq * 2 * 4);
    ws.want(ws.sbase, (size_t)nq * 3 * 4);
    ws.want(ws.counters, CNT_WORDS * 4);
    ws.want(ws.cand, (size_t)nq * n * 8);
    ws.want(ws.small_tickets, 64 * 4);
    // allow-list: the scan writes SCANN_KEY_MAX for a rejected row, which the finish stage never selects
    const uint64_t allow_bits = std::min<uint64_t>(flt.bits, n);
    const size_t allow_words = flt.bitmap ? (size_t)((allow_bits + 63) / 64) : 0;
    if (flt.bitmap) ws.want(ws.allow, std::max<size_t>(allow_words, 1) * 8);
    SCANN_TRY(ws.commit());
    if (allow_words)
        SCANN_HIP_CHECK(hipMemcpyAsync(ws.allow.p, flt.bitmap, allow_words * 8, hipMemcpyHostToDevice, sl.stream));
    const size_t qb = (size_t)nq * q_stride * 4, ob = (size_t)nq * k * 4;
    const size_t off_idx = (qb + 255) & ~(size_t)255, off_dist = off_idx + ((ob + 255) & ~(size_t)255),
                 off_cnt = off_dist + ((ob + 255) & ~(size_t)255);
    const size_t off_flag = off_cnt + (((size_t)nq * 4 + 255) & ~(size_t)255);
    SCANN_TRY(sl.pin->ensure(off_flag + (size_t)nq * 4 + 256));
    char *hp = static_cast<char *>(sl.pin->host), *dp = static_cast<char *>(sl.pin->dev);
    std::memcpy(hp, queries, qb);
    const uint32_t seq = ++sl.pin->seq ? sl.pin->seq : ++sl.pin->seq;
    std::memset(hp + off_flag, 0, (size_t)nq * 4);   // (stale words of an earlier call's layout: see txh_search_host)
    TxhWork w{};
    w.nq = nq; w.q_stride = q_stride; w.P = 1; w.m = kk; w.k = k; w.cap = n; w.exact_reorder = false;
    w.no_threshold = true; w.need_sorted_cands = 0;
    w.allow = flt.bitmap ? ws.allow.as<uint64_t>() : nullptr; w.allow_bits = flt.bitmap ? allow_bits : 0;
    w.queries = reinterpret_cast<const float *>(dp);
    w.tokens = ws.tokens.as<uint32_t>(); w.token_dists = ws.token_dists.as<float>();
    w.vbase = ws.vbase.as<uint32_t>(); w.sbase = ws.sbase.as<uint32_t>(); w.st = 1;
    w.counters = ws.counters.as<uint32_t>(); w.cand = ws.cand.as<uint64_t>();
    w.out_idx = reinterpret_cast<uint32_t *>(dp + off_idx);
    w.out_dist = reinterpret_cast<float *>(dp + off_dist);
    w.out_count = reinterpret_cast<uint32_t *>(dp + off_cnt);
    w.pipeline = TxhPipeline::Small; w.scan = TxhScan::Exact; w.small_max_leaf = n;
    plan_small_launch(ix->bfx, kn, &w);
    w.small_tickets = ws.small_tickets.as<uint32_t>();
    w.small_done = reinterpret_cast<uint32_t *>(dp + off_flag);
    w.small_seq = seq;
    SCANN_TRY(txh_launch_search(ix->bfx, w, false, sl.stream, nullptr, nullptr));
    SCANN_TRY(wait_small_done(sl.stream, reinterpret_cast<const volatile uint32_t *>(hp + off_flag), nq, seq));
    std::memcpy(out_idx, hp + off_idx, ob);
    std::memcpy(out_dist, hp + off_dist, ob);
    std::memcpy(out_count, hp + off_cnt, (size_t)nq * 4);
    return SCANN_HIP_OK;
}

extern "C" {

int scann_hip_search_batched(scann_hip_index *ix, const float *queries, uint32_t nq,
                             uint32_t q_stride, uint32_t q_dim, uint32_t k,
                             const scann_hip_search_opts *opts, uint32_t *out_idx, float *out_dist,
                             uint32_t *out_count) {
    if (!ix) return fail(SCANN_HIP_INVALID_ARGUMENT, "index is null");
    if (nq == 0) return SCANN_HIP_OK;
    if (!queries || !out_count || (k > 0 && (!out_idx || !out_dist)))
        return fail(SCANN_HIP_INVALID_ARGUMENT, "null query/output pointer");
    if (ix->kind == KIND_BF) {
        SCANN_TRY(refuse_allow_stride(opts, "brute-force handles"));
        if (ix->bf.n == 0) {  // brute_force/searcher.rs:78-80: Ok(empty) before the dim check
            fill_empty(nq, k, out_idx, out_dist, out_count);
            return SCANN_HIP_OK;
        }
        if (q_dim != ix->bf.dim)  // searcher.rs:83-89
            return fail(SCANN_HIP_INVALID_ARGUMENT,
                        "Query dimensionality " + std::to_string(q_dim) +
                            " does not match dataset dimensionality " + std::to_string(ix->bf.dim));
        if (q_stride < q_dim) return fail(SCANN_HIP_INVALID_ARGUMENT, "q_stride < q_dim");
        if (k == 0) {
            fill_empty(nq, 0, nullptr, nullptr, out_count);
            return SCANN_HIP_OK;
        }
        SlotLock sl;
        SCANN_TRY(acquire_slot(ix, &sl));
        SCANN_TRY(set_device(ix->ctx));
        const Knobs kn = read_knobs();
        const BfFilter flt = bf_filter_of(opts, kn);
        // (past the pass kernels' dim the small pipeline is not taken either: the search below refuses at every nq)
        if (kn.small && ix->bfx.rows && nq <= kSmallBatch && k <= 64 && bf_pass_fits(ix->bf))
            return bf_small_search_host(ix, sl, queries, nq, q_stride, k, kn, flt, out_idx, out_dist, out_count);
        if (sl.primary) ix->next_events();
        const bool shortlist = !flt.bitmap && !(opts && opts->bf_exact) && bf_shortlist_eligible(ix->bf, nq, k, kn);
        int s = bf_search_host(ix->bf, *sl.bfw, queries, nq, q_stride, k, shortlist, kn.bf_shortlist_tail, flt, out_idx,
                               out_dist, out_count, sl.stream, sl.primary ? ix->ev0 : nullptr,
                               sl.primary ? ix->ev1 : nullptr);
        if (sl.primary) {
            ix->timing_valid = ix->timing && s == SCANN_HIP_OK;
            ix->timed_kernel = shortlist ? "bf_bf16_kernel" : bf_pass_kernel_name(ix->bf, nq);
        }
        return s;
    }
    if (q_dim != ix->tx.row_dim)  // tree_x_hybrid/mod.rs:251-253, hashes/hasher.rs:167-171 (projected handles: the rows' space)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "Query dimensionality mismatch");
    if (q_stride < q_dim) return fail(SCANN_HIP_INVALID_ARGUMENT, "q_stride < q_dim");
    if (k == 0) {
        fill_empty(nq, 0, nullptr, nullptr, out_count);
        return SCANN_HIP_OK;
    }
    return txh_search_host(ix, queries, nq, q_stride, k, opts, out_idx, out_dist, out_count);
}

int scann_hip_search_batched_params(scann_hip_index *ix, const float *queries, uint32_t nq, uint32_t q_stride,
                                    uint32_t q_dim, const uint32_t *k_per_query, const scann_hip_search_opts *opts,
                                    uint32_t out_pitch, uint32_t *out_idx, float *out_dist, uint32_t *out_count) {
    if (!ix) return fail(SCANN_HIP_INVALID_ARGUMENT, "index is null");
    if (nq == 0) return SCANN_HIP_OK;
    if (!queries || !k_per_query || !out_count) return fail(SCANN_HIP_INVALID_ARGUMENT, "null query/k/output pointer");
    if (q_stride < q_dim) return fail(SCANN_HIP_INVALID_ARGUMENT, "q_stride < q_dim");
    uint32_t kmax = 0;
    for (uint32_t i = 0; i < nq; ++i) kmax = std::max(kmax, k_per_query[i]);
    if (kmax > out_pitch) return fail(SCANN_HIP_INVALID_ARGUMENT, "out_pitch is smaller than the largest k");
    if (kmax > 0 && (!out_idx || !out_dist)) return fail(SCANN_HIP_INVALID_ARGUMENT, "null output pointer");
    for (size_t i = 0; i < (size_t)nq * out_pitch; ++i) {
        out_idx[i] = 0xFFFFFFFFu;
        out_dist[i] = INFINITY;
    }
    // one batch per distinct k, in order of first appearance
    std::vector<uint32_t> order(nq);
    for (uint32_t i = 0; i < nq; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return k_per_query[a] < k_per_query[b]; });
    std::vector<float> qbuf;
    // per-query bitmaps travel with their queries: bitmap row order[i] goes where query order[i] goes (packed at
    // the bitmap's own length; brute-force handles refuse the stride in the call below)
    SCANN_TRY(check_allow_stride(opts));
    const uint64_t astride = allow_stride_of(opts), awords = astride ? allow_words(opts->allow_bitmap_bits) : 0;
    std::vector<uint64_t> abuf;
    scann_hip_search_opts gopts;
    if (astride) gopts = *opts;
    std::vector<uint32_t> gi, gc;
    std::vector<float> gd;
    for (uint32_t a0 = 0; a0 < nq;) {
        const uint32_t k = k_per_query[order[a0]];
        uint32_t a1 = a0;
        while (a1 < nq && k_per_query[order[a1]] == k) ++a1;
        const uint32_t g = a1 - a0;
        qbuf.resize((size_t)g * q_stride);
        for (uint32_t j = 0; j < g; ++j)
            std::memcpy(&qbuf[(size_t)j * q_stride], queries + (size_t)order[a0 + j] * q_stride, (size_t)q_stride * 4);
        gi.assign((size_t)g * std::max(1u, k), 0xFFFFFFFFu);
        gd.assign((size_t)g * std::max(1u, k), INFINITY);
        gc.assign(g, 0u);
        if (astride && awords) {
            abuf.resize((size_t)g * awords);
            for (uint32_t j = 0; j < g; ++j)
                std::memcpy(&abuf[(size_t)j * awords], opts->allow_bitmap + (size_t)order[a0 + j] * astride, (size_t)awords * 8);
            gopts.allow_bitmap = abuf.data();
            gopts.allow_bitmap_stride = awords;
        }
        SCANN_TRY(scann_hip_search_batched(ix, qbuf.data(), g, q_stride, q_dim, k, astride ? &gopts : opts, gi.data(), gd.data(),
                                           gc.data()));
        for (uint32_t j = 0; j < g; ++j) {
            const uint32_t q = order[a0 + j];
            out_count[q] = gc[j];
            for (uint32_t r = 0; r < gc[j]; ++r) {
                out_idx[(size_t)q * out_pitch + r] = gi[(size_t)j * k + r];
                out_dist[(size_t)q * out_pitch + r] = gd[(size_t)j * k + r];
            }
        }
        a0 = a1;
    }
    return SCANN_HIP_OK;
}

}  // extern "C"

static int search_device_ws(scann_hip_index *ix, scann_hip_index::DeviceSlot *dsl, TxhWorkspace &ws, BfWorkspace &bfw,
                            TxhPipeline widest, const float *d_queries, uint32_t nq, uint32_t q_stride, uint32_t k,
                            const scann_hip_search_opts *opts, uint32_t *d_out_idx, float *d_out_dist,
                            uint32_t *d_out_count, hipStream_t st);

extern "C" {

int scann_hip_index_reserve(scann_hip_index *ix, uint32_t max_nq, uint32_t max_k,
                            const scann_hip_search_opts *opts) {
    if (!ix) return fail(SCANN_HIP_INVALID_ARGUMENT, "index is null");
    std::lock_guard<std::mutex> lock(ix->mu);
    SCANN_TRY(set_device(ix->ctx));
    if (ix->kind == KIND_BF) return bf_reserve(ix->bf, ix->bfw, max_nq, max_k, opts && opts->allow_bitmap);
    TxhPlan p;
    SCANN_TRY(plan_txh_search(ix, max_k, opts, max_nq, false, TxhPipeline::Staged, read_knobs(), &p));
    TxhWork w;
    // (a host call's copy of its bitmap, or of its max_nq bitmaps allow_bitmap_stride words apart)
    SCANN_TRY(check_allow_stride(opts));
    const size_t allow_bytes = opts && opts->allow_bitmap ? std::max<size_t>(allow_copy_words(opts, max_nq), 1) * 8 : 0;
    return ensure_txh_workspace(ix, ix->ws, p, false, 0, false, &w, allow_bytes);
}

int scann_hip_search_batched_device(scann_hip_index *ix, const float *d_queries, uint32_t nq,
                                    uint32_t q_stride, uint32_t k, const scann_hip_search_opts *opts,
                                    uint32_t *d_out_idx, float *d_out_dist, uint32_t *d_out_count,
                                    void *hip_stream) {
    if (!ix) return fail(SCANN_HIP_INVALID_ARGUMENT, "index is null");
    if (nq == 0) return SCANN_HIP_OK;
    if (k == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "k must be > 0 on the device path");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::lock_guard<std::mutex> lock(ix->mu);
    SCANN_TRY(set_device(ix->ctx));
    scann_hip_index::DeviceSlot *dsl = nullptr;
    SCANN_TRY(device_slot(ix, st, &dsl));
    return search_device_ws(ix, dsl, *dsl->ws, *dsl->bfw, TxhPipeline::Wide, d_queries, nq, q_stride, k, opts, d_out_idx,
                            d_out_dist, d_out_count, st);
}

}  // extern "C"

// The enqueue-only search in workspace (ws, bfw) on stream st, device pointers throughout.
// dsl != null: scann_hip_search_batched_device with ix->mu held and the stream's workspace chosen (kernel timing and
// the slot's completion event follow the call).  dsl == null: a host entry point that owns (ws, bfw) through its
// SlotLock and synchronises by itself; it touches none of the handle's primary-slot state.
static int search_device_ws(scann_hip_index *ix, scann_hip_index::DeviceSlot *dsl, TxhWorkspace &ws, BfWorkspace &bfw,
                            TxhPipeline widest, const float *d_queries, uint32_t nq, uint32_t q_stride, uint32_t k,
                            const scann_hip_search_opts *opts, uint32_t *d_out_idx, float *d_out_dist,
                            uint32_t *d_out_count, hipStream_t st) {
    const Knobs kn = read_knobs();
    if (ix->kind == KIND_BF) {
        SCANN_TRY(refuse_allow_stride(opts, "brute-force handles"));
        if (dsl) ix->next_events();
        const BfFilter flt = bf_filter_of(opts, kn);   // (a device pointer on this path)
        const bool shortlist = !flt.bitmap && !(opts && opts->bf_exact) && bf_shortlist_eligible(ix->bf, nq, k, kn);
        int s = bf_search_device(ix->bf, bfw, d_queries, nq, q_stride, k, shortlist, kn.bf_shortlist_tail, flt,
                                 d_out_idx, d_out_dist, d_out_count, st, dsl ? ix->ev0 : nullptr, dsl ? ix->ev1 : nullptr);
        if (!dsl) return s;
        if (s == SCANN_HIP_OK) s = device_slot_done(dsl, st);
        ix->timing_valid = ix->timing && s == SCANN_HIP_OK;
        ix->timed_kernel = shortlist ? "bf_bf16_kernel" : bf_pass_kernel_name(ix->bf, nq);
        return s;
    }
    TxhPlan p;
    SCANN_TRY(check_allow_stride(opts));
    SCANN_TRY(plan_txh_search(ix, k, opts, nq, false, widest, kn, &p));
    if (p.m == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "pre-reorder candidate count is 0");
    TxhWork w;
    SCANN_TRY(ensure_txh_workspace(ix, ws, p, false, q_stride, false, &w));
    w.queries = d_queries;
    w.out_idx = d_out_idx;
    w.out_dist = d_out_dist;
    w.out_count = d_out_count;
    if (opts && opts->allow_bitmap) {   // device pointer on this path
        w.allow = opts->allow_bitmap;
        w.allow_bits = opts->allow_bitmap_bits;
        w.allow_stride = opts->allow_bitmap_stride;
    }
    if (!dsl) return launch_txh(ix, w, st, nullptr, nullptr);
    ix->last_work = w;
    ix->next_events();
    SCANN_TRY(launch_txh(ix, w, st, ix->ev0, ix->ev1));
    SCANN_TRY(device_slot_done(dsl, st));
    ix->timing_valid = ix->timing;
    ix->timed_kernel = txh_kernel_name(ix->tx, p, /*pinned=*/false);
    return SCANN_HIP_OK;
}

extern "C" {

int scann_hip_index_last_device_status(scann_hip_index *ix, void *hip_stream) {
    if (!ix) return fail(SCANN_HIP_INVALID_ARGUMENT, "index is null");
    SCANN_TRY(set_device(ix->ctx));
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::lock_guard<std::mutex> lock(ix->mu);
    // the workspace bound to this stream (else the primary one)
    const TxhWorkspace *ws = &ix->ws;
    const BfWorkspace *bfw = &ix->bfw;
    for (auto &d : ix->dslots)
        if (d.used && d.key == st && d.ws) {
            ws = d.ws;
            bfw = d.bfw;
        }
    if (ix->kind == KIND_BF) return bf_last_status(*bfw, st);
    if (ix->kind != KIND_TXH || !ws->counters.p) return SCANN_HIP_OK;
    uint32_t counters[CNT_N];
    SCANN_HIP_CHECK(hipMemcpyAsync(counters, ws->counters.p, sizeof(counters),
                                   hipMemcpyDeviceToHost, st));
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    if (counters[CNT_STATUS] != SCANN_HIP_OK)
        return fail((int)counters[CNT_STATUS],
                    "candidate threshold/buffer miss on the device path (use the host entry "
                    "point, which retries without a threshold and with a full-size buffer)");
    return SCANN_HIP_OK;
}

int scann_hip_index_debug_filter_bounds(scann_hip_index *ix, void *hip_stream, uint32_t nq, uint64_t *out_bounds) {
    if (!ix || ix->kind != KIND_TXH) return fail(SCANN_HIP_INVALID_ARGUMENT, "not a tree / hasher index");
    if (nq && !out_bounds) return fail(SCANN_HIP_INVALID_ARGUMENT, "out_bounds is null");
    SCANN_TRY(set_device(ix->ctx));
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::lock_guard<std::mutex> lock(ix->mu);
    // the workspace bound to this stream (else the primary one)
    const TxhWorkspace *ws = &ix->ws;
    for (auto &d : ix->dslots)
        if (d.used && d.key == st && d.ws) ws = d.ws;
    if (!ws->thr.p || ws->thr.bytes < (size_t)nq * 8)
        return fail(SCANN_HIP_OUT_OF_RANGE, "no batched search of that many queries has run in this workspace");
    SCANN_HIP_CHECK(hipMemcpy(out_bounds, ws->thr.p, (size_t)nq * 8, hipMemcpyDeviceToHost));
    return SCANN_HIP_OK;
}

int scann_hip_index_debug_survivor_bitmap_bytes(scann_hip_index *ix, void *hip_stream, uint64_t *out_bytes) {
    if (!ix || ix->kind != KIND_TXH) return fail(SCANN_HIP_INVALID_ARGUMENT, "not a tree / hasher index");
    if (!out_bytes) return fail(SCANN_HIP_INVALID_ARGUMENT, "out_bytes is null");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::lock_guard<std::mutex> lock(ix->mu);
    const TxhWorkspace *ws = &ix->ws;
    for (auto &d : ix->dslots)
        if (d.used && d.key == st && d.ws) ws = d.ws;
    *out_bytes = ws->surv.need;
    return SCANN_HIP_OK;
}

int scann_hip_index_debug_rerank_brackets(scann_hip_index *ix, void *hip_stream, uint32_t nq, uint32_t m, uint32_t *out_lb,
                                          uint32_t *out_ub, uint32_t *out_rows, uint32_t *out_counts) {
    if (!ix || ix->kind != KIND_TXH) return fail(SCANN_HIP_INVALID_ARGUMENT, "not a tree / hasher index");
    if (ix->tx.qfmt)
        return fail(SCANN_HIP_UNIMPLEMENTED, "a handle over quantized rows has no re-rank row filter: no brackets to read");
    if (ix->proj.kind)
        return fail(SCANN_HIP_UNIMPLEMENTED, "a handle that searches through a projection has no re-rank row filter: no brackets to read");
    if (nq && m && (!out_lb || !out_ub || !out_rows || !out_counts))
        return fail(SCANN_HIP_INVALID_ARGUMENT, "an output is null");
    SCANN_TRY(set_device(ix->ctx));
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::lock_guard<std::mutex> lock(ix->mu);
    // the workspace bound to this stream (else the primary one)
    const TxhWorkspace *ws = &ix->ws;
    for (auto &d : ix->dslots)
        if (d.used && d.key == st && d.ws) ws = d.ws;
    const size_t list = (size_t)nq * m * 4;
    if (!ws->rr_lb.p || !ws->rr_ub.p || !ws->cand_row.p || !ws->cand_count.p || ws->rr_lb.bytes < list ||
        ws->rr_ub.bytes < list || ws->cand_row.bytes < list || ws->cand_count.bytes < (size_t)nq * 4)
        return fail(SCANN_HIP_OUT_OF_RANGE, "no filtered re-rank of that many queries and candidates has run in this workspace");
    SCANN_HIP_CHECK(hipMemcpy(out_lb, ws->rr_lb.p, list, hipMemcpyDeviceToHost));
    SCANN_HIP_CHECK(hipMemcpy(out_ub, ws->rr_ub.p, list, hipMemcpyDeviceToHost));
    SCANN_HIP_CHECK(hipMemcpy(out_rows, ws->cand_row.p, list, hipMemcpyDeviceToHost));
    SCANN_HIP_CHECK(hipMemcpy(out_counts, ws->cand_count.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
    return SCANN_HIP_OK;
}

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

}  // extern "C"

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
    CrowdWorkspace &cw = *sl.crowd;
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
    int s = search_device_ws(ix, nullptr, *sl.ws, *sl.bfw, TxhPipeline::Staged, cw.queries.as<float>(), nq, q_stride,
                             depth, &o, cw.idx.as<uint32_t>(), cw.dist.as<float>(), cw.cnt.as<uint32_t>(), st);
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
    if (ix->kind == KIND_BF) return bf_last_status(*sl.bfw, st);   // (synchronises)
    uint32_t counters[CNT_N] = {};
    if (sl.ws->counters.p)
        SCANN_HIP_CHECK(hipMemcpyAsync(counters, sl.ws->counters.p, sizeof(counters), hipMemcpyDeviceToHost, st));
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
    CrowdWorkspace &cw = *sl.crowd;
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
    scann_hip_index::DeviceSlot *dsl = nullptr;
    SCANN_TRY(device_slot(ix, st, &dsl));
    CrowdWorkspace &cw = *dsl->crowd;
    if (depth > sg.max_depth()) {   // past every handle's largest k: the plain search's own error where it has one
        if (ix->kind == KIND_TXH) {
            TxhPlan p;
            SCANN_TRY(plan_txh_search(ix, depth, opts, nq, false, TxhPipeline::Wide, read_knobs(), &p));
        }
        return stage_depth_error(sg);
    }
    SCANN_TRY(cw.ensure_rows(nq, depth));   // (no allocation after scann_hip_index_reserve_crowded / _mmr)
    SCANN_TRY(search_device_ws(ix, dsl, *dsl->ws, *dsl->bfw, TxhPipeline::Wide, d_queries, nq, q_stride, depth, opts,
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
    SCANN_TRY(ix->crowd.ensure_rows(max_nq, max_depth));
    return ix->crowd.ensure_out(max_nq, std::max(1u, max_k));
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

// ---- multi-GPU ------------------------------------------------------------------------
int scann_hip_txh_search_local_device(scann_hip_index *ix, const float *d_queries, uint32_t nq,
                                      uint32_t q_stride, uint32_t k,
                                      const scann_hip_search_opts *opts, uint64_t *d_keys,
                                      uint32_t *d_idx, float *d_exact, uint32_t *d_count,
                                      void *hip_stream) {
    if (!ix || ix->kind != KIND_TXH) return fail(SCANN_HIP_INVALID_ARGUMENT, "not a tree index");
    if (ix->tx.qfmt) return fail(SCANN_HIP_UNIMPLEMENTED, "the local stage of a sharded search over quantized rows is not built");
    if (ix->proj.kind) return fail(SCANN_HIP_UNIMPLEMENTED, "the local stage of a sharded search through a projection is not built");
    SCANN_TRY(refuse_allow_stride(opts, "the leaf-sharded search"));
    if (nq == 0) return SCANN_HIP_OK;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::lock_guard<std::mutex> lock(ix->mu);
    SCANN_TRY(set_device(ix->ctx));
    TxhPlan p;
    SCANN_TRY(plan_txh_search(ix, k, opts, nq, false, TxhPipeline::Staged, read_knobs(), &p));
    if (!p.exact_reorder) return fail(SCANN_HIP_INVALID_ARGUMENT, "local stage needs exact_reorder");
    if (p.m == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "pre-reorder candidate count is 0");
    scann_hip_index::DeviceSlot *dsl = nullptr;
    SCANN_TRY(device_slot(ix, st, &dsl));
    TxhWork w;
    SCANN_TRY(ensure_txh_workspace(ix, *dsl->ws, p, false, q_stride, false, &w));
    w.queries = d_queries;
    w.cand_key = d_keys;
    w.cand_idx = d_idx;
    w.cand_exact = d_exact;
    w.cand_count = d_count;
    if (opts && opts->allow_bitmap) {   // device pointer on this path
        w.allow = opts->allow_bitmap;
        w.allow_bits = opts->allow_bitmap_bits;
    }
    ix->last_work = w;
    ix->next_events();
    SCANN_TRY(txh_launch_search(ix->tx, w, true, st, ix->ev0,
                                ix->ev1));
    SCANN_TRY(device_slot_done(dsl, st));
    ix->timing_valid = ix->timing;
    ix->timed_kernel = txh_kernel_name(ix->tx, p, /*pinned=*/false);
    return SCANN_HIP_OK;
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
int scann_hip_txh_partition(scann_hip_index *ix, const float *queries, uint32_t nq,
                            uint32_t q_stride, uint32_t q_dim, uint32_t num_partitions,
                            uint32_t *out_tokens, float *out_dists, uint32_t *out_count) {
    if (!ix || ix->kind != KIND_TXH) return fail(SCANN_HIP_INVALID_ARGUMENT, "not a tree index");
    if (ix->tx.ah_mode)  // tree_partitioner.rs:197-198
        return fail(SCANN_HIP_FAILED_PRECONDITION, "Partitioner not built");
    if (q_dim != ix->tx.dim) return fail(SCANN_HIP_INVALID_ARGUMENT, "Query dimensionality mismatch");
    if (nq == 0) return SCANN_HIP_OK;
    std::lock_guard<std::mutex> lock(ix->mu);
    SCANN_TRY(set_device(ix->ctx));
    scann_hip_search_opts o;
    scann_hip_search_opts_default(&o);
    o.partitions_to_search = std::max(1u, num_partitions);
    o.exact_reorder = 0;
    TxhPlan p;
    SCANN_TRY(plan_txh_search(ix, 1, &o, nq, false, TxhPipeline::Staged, read_knobs(), &p));
    TxhWork w;
    SCANN_TRY(claim_primary_workspace(ix));
    SCANN_TRY(ensure_txh_workspace(ix, ix->ws, p, true, q_stride, true, &w));
    SCANN_HIP_CHECK(hipMemcpyAsync(ix->ws.queries.p, queries, (size_t)nq * q_stride * 4,
                                   hipMemcpyHostToDevice, ix->stream));
    SCANN_TRY(txh_launch_partition_only(ix->tx, w, ix->stream));
    const uint32_t P = num_partitions == 0 ? 0 : p.P;
    if (P) {
        SCANN_HIP_CHECK(hipMemcpyAsync(out_tokens, w.tokens, (size_t)nq * P * 4, hipMemcpyDeviceToHost,
                                       ix->stream));
        SCANN_HIP_CHECK(hipMemcpyAsync(out_dists, w.token_dists, (size_t)nq * P * 4,
                                       hipMemcpyDeviceToHost, ix->stream));
    }
    SCANN_HIP_CHECK(hipStreamSynchronize(ix->stream));
    if (out_count)
        for (uint32_t i = 0; i < nq; ++i) out_count[i] = P;
    return SCANN_HIP_OK;
}

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
    return bf_distances_host(ix->bf, ix->bfw, queries, nq, q_stride, out, ix->stream);
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
    return bf_search_radius_host(ix->bf, ix->bfw, query, q_dim, radius, bf_filter_of(opts, read_knobs()), out_idx,
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

static int kmeans_args(scann_hip_index *ix, uint32_t col_offset, uint32_t sub_dim, uint32_t k, const void *c) {
    if (!ix || ix->kind != KIND_BF) return fail(SCANN_HIP_INVALID_ARGUMENT, "not a brute-force index");
    if (ix->bf.fmt) return fail(SCANN_HIP_INVALID_ARGUMENT, "the index holds quantized rows, not f32 rows");
    if (ix->bf.n == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "Cannot cluster empty dataset");   // kmeans.rs:167-169
    if (!c || k == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "null centres / zero clusters");
    if (sub_dim == 0 || (uint64_t)col_offset + sub_dim > ix->bf.dim)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "column window outside the rows");
    return SCANN_HIP_OK;
}

int scann_hip_kmeans_init_pp(scann_hip_index *ix, uint32_t col_offset, uint32_t sub_dim, uint32_t k,
                             uint64_t seed, uint32_t simd_threshold, float *centers_out) {
    SCANN_TRY(kmeans_args(ix, col_offset, sub_dim, k, centers_out));
    std::lock_guard<std::mutex> lock(ix->mu);
    SCANN_TRY(set_device(ix->ctx));
    return bf_kmeans_init_pp_host(ix->bf, col_offset, sub_dim, k, seed, simd_threshold, centers_out, ix->stream);
}

void scann_hip_build_config_default(scann_hip_build_config *c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->kmeans_iterations = 100;         // tree_partitioner.rs:72
    c->kmeans_convergence = 1e-5;
    c->kmeans_seed = 42;
    c->training_iterations = 25;        // CodebookConfig.max_iterations
    c->convergence_threshold = 1e-5;
    c->seed = 42;
    c->simd_threshold = 128;            // KMeansConfig.simd_threshold
    c->use_residuals = 1;
    c->store_rows = 1;
    c->batched_codebook = 1;
    c->partitions_to_search = 10;
    c->pre_reorder_multiplier = 3.0f;
    c->distance_measure = SCANN_HIP_SQUARED_L2;
}

int scann_hip_txh_build(scann_hip_index *rows, const scann_hip_build_config *cfg, scann_hip_index **out_index,
                        scann_hip_build_report *out_report) {
    if (!rows || !cfg || !out_index) return fail(SCANN_HIP_INVALID_ARGUMENT, "null rows/config/out_index");
    *out_index = nullptr;
    if (out_report) std::memset(out_report, 0, sizeof(*out_report));
    if (rows->kind != KIND_BF) return fail(SCANN_HIP_INVALID_ARGUMENT, "not a brute-force index");
    std::lock_guard<std::mutex> lock(rows->mu);
    SCANN_TRY(set_device(rows->ctx));
    SCANN_TRY(build_check(rows->bf, *cfg));   // every refusal, before the first training launch
    BuildParts parts;
    SCANN_TRY(build_txh_device(rows->bf, *cfg, rows->stream, &parts, out_report));
    return index_build_txh(rows, *cfg, parts, out_index, out_report);
}

int scann_hip_txh_build_projected(scann_hip_index *rows, const scann_hip_projection *projection,
                                  const scann_hip_build_config *cfg, scann_hip_index **out_index,
                                  scann_hip_build_report *out_report) {
    if (!rows || !cfg || !out_index) return fail(SCANN_HIP_INVALID_ARGUMENT, "null rows/config/out_index");
    *out_index = nullptr;
    if (out_report) std::memset(out_report, 0, sizeof(*out_report));
    if (!projection) return fail(SCANN_HIP_INVALID_ARGUMENT, "projected build: projection is null");
    if (rows->kind != KIND_BF) return fail(SCANN_HIP_INVALID_ARGUMENT, "not a brute-force index");
    std::lock_guard<std::mutex> lock(rows->mu);
    SCANN_TRY(set_device(rows->ctx));
    const ProjDev &pd = projection->dev;
    // the rows' view in the index space: [n][out_dim] at stride out_dim (the temporary buffer below)
    BfIndexDev view = rows->bf;
    view.dim = view.stride = pd.out_dim;
    view.rows_b = view.rows_bl = nullptr;
    view.norm2 = nullptr;
    view.max_norm = 0.0f;
    SCANN_TRY(build_check(view, *cfg));   // every refusal of scann_hip_txh_build, judged on out_dim, before any launch
    if (rows->bf.dim != pd.in_dim)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "projected build: the rows' dim " + std::to_string(rows->bf.dim) +
                                                    " is not the projection's in_dim " + std::to_string(pd.in_dim));
    const uint64_t n = rows->bf.n;
    if (n > SIZE_MAX / 4 / pd.out_dim) return fail(SCANN_HIP_OUT_OF_RANGE, "projected build: n * out_dim overflows");
    const auto t0 = std::chrono::steady_clock::now();
    DevBuf projected;
    SCANN_TRY(projected.ensure((size_t)n * pd.out_dim * 4));
    SCANN_TRY(launch_project(pd, rows->bf.rows, n, rows->bf.stride, projected.as<float>(), pd.out_dim, rows->stream));
    SCANN_HIP_CHECK(hipStreamSynchronize(rows->stream));
    const float project_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    view.rows = projected.as<float>();
    BuildParts parts;
    SCANN_TRY(build_txh_device(view, *cfg, rows->stream, &parts, out_report));
    projected.release();
    if (out_report) out_report->stage_ms[0] += project_ms;
    return index_build_txh(rows, *cfg, parts, out_index, out_report, projection);
}

int scann_hip_pca_train(scann_hip_index *rows, uint32_t out_dim, uint64_t max_samples, uint64_t seed,
                        scann_hip_projection **out_projection, double *out_eigenvalues, double *out_covariance,
                        uint32_t *out_sweeps, int *out_converged) {
    if (!rows || !out_projection) return fail(SCANN_HIP_INVALID_ARGUMENT, "null rows/out_projection");
    *out_projection = nullptr;
    if (rows->kind != KIND_BF) return fail(SCANN_HIP_INVALID_ARGUMENT, "pca_train: not a brute-force index");
    std::lock_guard<std::mutex> lock(rows->mu);
    SCANN_TRY(set_device(rows->ctx));
    SCANN_TRY(pca_check(rows->bf, out_dim));   // every refusal, before the first launch
    return pca_train_device(rows->ctx, rows->bf, out_dim, max_samples, seed, rows->stream, out_projection, out_eigenvalues,
                            out_covariance, out_sweeps, out_converged);
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

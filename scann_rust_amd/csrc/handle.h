// handle.h -- the index handle behind the C ABI (scann_hip_ctx, scann_hip_index), the scratch of a search slot, and
// the few functions one api unit calls in another.  Internal to api.hip, api_create.hip, api_search.hip and
// api_stages.hip: every other source sees a handle through the views of mutable.h / index_arrays.h.
#pragma once
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "bf.h"
#include "common.h"
#include "knobs.h"
#include "project.h"
#include "txh.h"
#include "txh_arena.h"

struct scann_hip_ctx {
    int device = 0;
    int num_cus = 256;
};

namespace scann {

enum IndexKind { KIND_BF = 1, KIND_TXH = 2 };

// Per-call scratch of the Tree-X-Hybrid pipeline.  Every buffer lives in ONE device allocation: a call first states
// what it needs (want), then commit() rebuilds the arena if any buffer has to grow -- one hipFree (which waits for the
// device) + one hipMalloc, every buffer re-placed in the order of txh_arena.h at the largest size seen so far.  Placement
// is therefore a function of the sizes alone, never of the order in which a handle met its batch sizes and
// pre_reorder_k values: round 2 allocated every buffer separately, and a workspace that had grown buffer by buffer
// (free one, allocate it larger, next) left rerank_short_kernel 3x slower than a fresh one of the same sizes
// (txh_arena_place: the skew that keeps it so).
struct TxhWorkspace : TxhArenaBufs {
    void *arena = nullptr;
    size_t arena_bytes = 0;
    bool dirty = false;
    uint32_t rebuilds = 0;
    TxhWorkspace() = default;
    TxhWorkspace(const TxhWorkspace &) = delete;
    TxhWorkspace &operator=(const TxhWorkspace &) = delete;
    ~TxhWorkspace() { release_all(); }
    void want(WsBuf &b, size_t bytes) {
        if (bytes == 0) bytes = 16;
        if (bytes > b.need) b.need = bytes;
        if (b.need > b.bytes) dirty = true;
    }
    int commit() {
        if (!dirty) return SCANN_HIP_OK;
        size_t need[kTxhArenaCount], off[kTxhArenaCount], cap[kTxhArenaCount], i = 0;
        for_each([&](WsBuf &b) { need[i++] = b.need; });
        const size_t total = txh_arena_place(need, kTxhArenaCount, off, cap);
        if (arena) (void)hipFree(arena);   // (waits for the device: kernels of earlier calls may still read it)
        arena = nullptr;
        arena_bytes = 0;
        for_each([&](WsBuf &b) { b.p = nullptr; b.bytes = 0; });
        SCANN_HIP_CHECK(hipMalloc(&arena, total ? total : 256));
        arena_bytes = total;
        i = 0;
        for_each([&](WsBuf &b) {
            if (b.need) b.p = static_cast<char *>(arena) + off[i];
            b.bytes = cap[i++];
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

// The scratch of ONE search slot: whatever a call on that slot's stream may write.  (A PinBuf that no host call uses
// allocates nothing.)
struct SlotScratch {
    TxhWorkspace ws;
    BfWorkspace bfw;
    CrowdWorkspace crowd;
    PinBuf pin;
};

// An extra stream + scratch: host-side searches of concurrent caller threads (Searcher: Send +
// Sync, tests/stress_tests.rs:256-297) run side by side instead of queueing on one mutex.
struct SearchSlot {
    std::mutex mu;
    hipStream_t stream = nullptr;
    SlotScratch sc;
};

// Scratch of the `_device` entry points, one per CALLER STREAM (scann_hip.h "Device entry points"): slot 0 is the
// primary scratch, further ones are created on demand.  A slot that changes streams is ordered behind its previous
// stream's last call with an event.
struct DeviceSlot {
    hipStream_t key = nullptr;
    bool used = false, done_valid = false;
    hipEvent_t done = nullptr;
    uint64_t tick = 0;
    SlotScratch *sc = nullptr;
    std::unique_ptr<SlotScratch> own;   // slots above 0
};

// The event pair around the dominant kernel of a timed call (nulls: this call is not timed).
struct TimedEvents {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
};

}  // namespace scann

struct scann_hip_index {
    scann_hip_ctx *ctx = nullptr;
    int kind = 0;
    std::mutex mu;  // the primary slot (stream, primary below): device entry points and timing use it
    std::mutex slots_mu;
    std::vector<std::unique_ptr<scann::SearchSlot>> slots;   // created on demand, at most max_slots() - 1
    hipStream_t stream = nullptr;
    scann::SlotScratch primary;   // the primary slot's scratch
    // ring of HIP event pairs bracketing the dominant kernel of each search launch
    static constexpr int kEvRing = 64;
    hipEvent_t evs[kEvRing][2] = {};
    uint32_t ev_n = 0;      // launches recorded since timing was enabled
    bool timing = false;
    bool timing_valid = false;
    const char *timed_kernel = "";
    // Kernel timing follows the primary slot and the device slots only (timed = false: a call on an extra host slot, or
    // a host call that runs the enqueue-only search by itself).  Before the launch: the pair to record around the kernel.
    scann::TimedEvents timing_begin(bool timed) {
        if (!timed || !timing) return scann::TimedEvents{nullptr, nullptr, timed};
        hipEvent_t *pair = evs[ev_n++ % kEvRing];
        return scann::TimedEvents{pair[0], pair[1], true};
    }
    // ... and after it: whether scann_hip_index_last_kernel_ms has a time to report, and of which kernel.
    void timing_end(const scann::TimedEvents &t, bool ok, const char *kernel) {
        if (!t.timed) return;
        timing_valid = timing && ok;
        timed_kernel = kernel;
    }
    scann::DevBuf status_word;

    // ---- crowding (scann_hip_index_set_crowding_attributes): one u64 per datapoint index, may be shorter ----
    scann::DevBuf crowd_attrs;
    uint64_t n_crowd_attrs = 0;
    bool has_crowd_attrs = false;
    // multi-attribute crowding (scann_hip_index_set_crowding_attributes_md): [crowd_md_dims][n_crowd_md_attrs] u64,
    // dimension-major; crowd_md_dims == 0: none attached
    scann::DevBuf crowd_md_attrs;
    uint64_t n_crowd_md_attrs = 0;
    uint32_t crowd_md_dims = 0;

    // ---- brute force ----
    scann::BfIndexDev bf{};
    scann::DevBuf bf_rows, bf_rows_b, bf_rows_bl, bf_norm2, bf_leaf;
    scann::TxhIndexDev bfx{};        // the same rows as a one-leaf exact-scan index: the small-batch pipeline's view

    // ---- tree-x-hybrid / AH ----
    scann::TxhIndexDev tx{};
    scann::DevBuf d_centers, d_centers_t, d_leaf_off, d_leaf_gsize, d_leaf_ids, d_codes, d_codes_sp, d_rows, d_codebook, d_rows8, d_rows8_meta;
    scann::DevBuf d_qrows;    // scann_hip_txh_create_quantized: the re-rank rows as given (d_rows, d_rows8 stay empty)
    int q_fmt = 0;            // ... their SCANN_HIP_ROWS_* format (0: f32 rows or none) and the int8 inv_multiplier
    float q_inv = 1.0f;
    // scann_hip_txh_create_projected: the handle's own copy of the projection (kind 0: none).  tx.dim is then the
    // projection's out_dim, tx.row_dim / row_stride describe d_rows, and launch_txh projects every call's queries.
    scann::ProjDev proj;
    scann::DevBuf d_proj_matrix, d_proj_mean;
    std::vector<uint32_t> local_sizes_desc;  // local leaf sizes, descending, prefix-summed
    uint32_t default_P = 0;
    float multiplier = 3.0f;
    scann::TxhWork last_work{};
    static constexpr int kMaxDeviceSlots = 4;
    scann::DeviceSlot dslots[kMaxDeviceSlots];   // slot 0 aliases `primary`
    uint64_t dslot_tick = 0;
    bool sharded = false;     // created with leaf_sizes_global: local leaves are a subset of the global stream
    uint64_t n_rows = 0;      // rows of d_rows / d_qrows (0: the handle stores none)
};

namespace scann {

// A search slot held by a host-side call: the primary one if it is free, else a free extra slot (created
// up to SCANN_HIP_SEARCH_SLOTS, default 4, streams + scratch in total), else wait for the primary.
struct SlotLock {
    std::unique_lock<std::mutex> lock;
    hipStream_t stream = nullptr;
    SlotScratch *sc = nullptr;
    bool primary = false;
};

// ---- api.hip ----
int set_device(const scann_hip_ctx *ctx);
// scalar fields of the descriptor a tree / hasher handle was created from
void txh_desc_of(const scann_hip_index *ix, scann_hip_txh_desc *d);

// ---- api_search.hip ----
int acquire_slot(scann_hip_index *ix, SlotLock *out);
// host-side users of the primary scratch, ix->mu held: wait for a device-entry call that may still be using it
int claim_primary_workspace(scann_hip_index *ix);
// ix->mu held: the scratch of a call that will be enqueued on `st`; device_slot_done after the call's last enqueue
int device_slot(scann_hip_index *ix, hipStream_t st, DeviceSlot **out);
int device_slot_done(DeviceSlot *sl, hipStream_t st);
int plan_txh_search(const scann_hip_index *ix, uint32_t k, const scann_hip_search_opts *o, uint32_t nq, bool retry,
                    TxhPipeline widest, const Knobs &kn, TxhPlan *out);
int ensure_txh_workspace(scann_hip_index *ix, TxhWorkspace &s, const TxhPlan &p, bool own_queries, uint32_t q_stride,
                         bool own_outputs, TxhWork *w, size_t allow_bytes = 0);
int search_device_ws(scann_hip_index *ix, DeviceSlot *dsl, SlotScratch &sc, TxhPipeline widest, const float *d_queries,
                     uint32_t nq, uint32_t q_stride, uint32_t k, const scann_hip_search_opts *opts, uint32_t *d_out_idx,
                     float *d_out_dist, uint32_t *d_out_count, hipStream_t st);
BfFilter bf_filter_of(const scann_hip_search_opts *opts, const Knobs &kn);
void fill_empty(uint32_t nq, uint32_t k, uint32_t *out_idx, float *out_dist, uint32_t *out_count);

}  // namespace scann

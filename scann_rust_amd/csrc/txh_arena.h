// txh_arena.h -- the buffers of a tree / hasher search workspace, named once, and where the arena places them.
// Plain C++ (no HIP include): the placement is a function of the sizes alone and is tested on the host.
#pragma once
#include <cstddef>

namespace scann {

// A buffer of a search workspace: a range of the workspace's ARENA (one device allocation, sub-allocated at 256-byte
// granularity in the order of the list below).
struct WsBuf {
    void *p = nullptr;
    size_t bytes = 0;   // capacity assigned in the arena
    size_t need = 0;    // largest size any call has asked for
    template <typename T>
    T *as() const { return static_cast<T *>(p); }
};

// Every buffer of the arena, in placement order.  A new buffer goes at the END: the buffers before it keep their places
// (proj_q: [nq][dim] projected queries of a projected handle; surv: the sparse prefilter's survivor bitmaps).
#define SCANN_TXH_ARENA_BUFFERS(X)                                                                                    \
    X(queries) X(cdist) X(tokens) X(token_dists) X(vbase) X(leaf_cnt) X(leaf_cursor) X(pair_off) X(tile_off)          \
    X(counters) X(pair_q) X(pair_leaf) X(pair_vbase) X(pair_thr) X(slot_of) X(lutq) X(thr) X(cand_cnt) X(cand)        \
    X(cand_key) X(cand_idx) X(cand_dist) X(cand_exact) X(cand_row) X(cand_count) X(out_idx) X(out_dist) X(out_count)  \
    X(allow) X(sbase) X(pair_sbase) X(stile_off) X(samp) X(lut8) X(lut8_meta) X(cand32) X(cand32_codes) X(cand32_cnt) \
    X(mfma_thr1) X(rr_lb) X(rr_ub) X(small_tickets) X(wide_min) X(wide_ckey) X(wide_ceb) X(wide_cidx) X(wide_cnt)     \
    X(proj_q) X(surv)

struct TxhArenaBufs {
#define SCANN_X(name) WsBuf name;
    SCANN_TXH_ARENA_BUFFERS(SCANN_X)
#undef SCANN_X
    template <typename F>
    void for_each(F f) {
#define SCANN_X(name) f(name);
        SCANN_TXH_ARENA_BUFFERS(SCANN_X)
#undef SCANN_X
    }
};

#define SCANN_X(name) #name,
static constexpr const char *kTxhArenaNames[] = {SCANN_TXH_ARENA_BUFFERS(SCANN_X)};
#undef SCANN_X
static constexpr size_t kTxhArenaCount = sizeof(kTxhArenaNames) / sizeof(kTxhArenaNames[0]);

static constexpr size_t kArenaNoPlace = ~(size_t)0;

// need[i] of every buffer -> its offset in the arena and its capacity; returns the arena's size.
// Every buffer starts at its own skew inside a 128 KB window.  Back to back, the six per-candidate arrays of a
// batch ([nq][m] words each) lie exactly nq * m * 4 bytes apart -- 32 MB at nq = 1024, m = 8192 -- so that
// element (q, i) of ALL of them maps to the same HBM channel and bank: rerank_short_kernel, which walks
// several of them in step, ran 3x slower on such a layout (0.41 vs 0.14 ms; same instructions, same bytes:
// round 2's "workspace growth" slowdown was this aliasing, present or absent by the accident of which other
// buffers the handle had allocated in between).
// A buffer nobody asked for (need 0) gets no place (offset kArenaNoPlace, capacity 0); its skew still counts.
inline size_t txh_arena_place(const size_t *need, size_t n, size_t *offset, size_t *capacity) {
    size_t off = 0;
    for (size_t i = 0; i < n; ++i) {
        off += (((i + 1) * 37) % 509) * 256;
        capacity[i] = (need[i] + 255) & ~(size_t)255;
        offset[i] = need[i] ? off : kArenaNoPlace;
        off += capacity[i];
    }
    return off;
}

}  // namespace scann

// api_search.hip -- C ABI, searches: the plan of a tree / hasher search and its workspace, host and device search
// slots, the host and device search entry points, the local stage of a leaf-sharded search.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "allow.h"
#include "comm.h"
#include "handle.h"

using namespace scann;

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
int scann::plan_txh_search(const scann_hip_index *ix, uint32_t k, const scann_hip_search_opts *o, uint32_t nq,
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

// Buffers of the plan p (the arena re-places everything when one grows), bound into *w.
// allow_bytes: size of an allow-bitmap the caller will copy into s.allow (0 = none)
// A buffer the plan does not use is neither asked for nor bound: its field of *w stays null, which the launchers read
// as a switch (cand32_codes, surv against cand32, ...).  own_queries / own_outputs false: the caller binds its own.
int scann::ensure_txh_workspace(scann_hip_index *ix, TxhWorkspace &s, const TxhPlan &p, bool own_queries,
                                uint32_t q_stride, bool own_outputs, TxhWork *w, size_t allow_bytes) {
    const TxhIndexDev &t = ix->tx;
    const uint32_t nq = p.nq, L = t.L, P = p.P, m = std::max(1u, p.m), k = std::max(1u, p.k);
    const uint64_t max_slots64 = (uint64_t)nq * P + 3ull * L + 4;
    if (max_slots64 > 0xFFFFFFF0ull)
        return fail(SCANN_HIP_RESOURCE_EXHAUSTED, "batch x partitions_to_search exceeds the pair table (2^32 slots)");
    const uint32_t max_slots = (uint32_t)max_slots64;
    const uint32_t max_quads = max_slots / 4 + 1;
    const bool mfma = txh_scan_is_mfma(p.scan), small = p.pipeline != TxhPipeline::Staged,
               wide = p.pipeline == TxhPipeline::Wide;
    const bool lists = mfma && !p.sp_bitmap;   // the prefilter's survivors as lists (else as bitmaps: surv)
    // flat hashers: the survivors' packed codes (dense prefilter) or plane rows (sparse prefilter) travel with them
    const size_t code_words = std::max(t.S / 8, p.scan == TxhScan::Smfmac ? sp_words(t.S) : 0u);
    // every buffer of the plan, once: (buffer, bytes, whether the plan uses it, the field of *w it feeds).  Run twice:
    // first to ask for the sizes, then, when commit() has placed the arena, to bind the pointers.  (The first pass only
    // names the fields of *w, which is not initialised yet: it neither reads nor writes them.)
    const auto buffers = [&](auto use) {
        use(s.queries, (size_t)nq * q_stride * 4, own_queries, w->queries);
        use(s.cdist, (size_t)nq * L * 4, !t.ah_mode, w->cdist);
        use(s.tokens, (size_t)nq * P * 4, true, w->tokens);
        use(s.token_dists, (size_t)nq * P * 4, true, w->token_dists);
        use(s.vbase, (size_t)nq * (P + 1) * 4, true, w->vbase);
        use(s.sbase, (size_t)nq * (P + 2) * 4, true, w->sbase);
        use(s.pair_sbase, (size_t)max_slots * 4, true, w->pair_sbase);
        use(s.stile_off, (size_t)(L + 1) * 4, true, w->stile_off);
        use(s.samp, (size_t)nq * p.scap * (p.sample_mfma ? 2 : 4), true, w->samp);
        use(s.leaf_cnt, (size_t)L * 4, true, w->leaf_cnt);
        use(s.leaf_cursor, (size_t)L * 4, true, w->leaf_cursor);
        use(s.pair_off, (size_t)(L + 1) * 4, true, w->pair_off);
        use(s.tile_off, (size_t)(L + 1) * 4, true, w->tile_off);
        use(s.counters, CNT_WORDS * 4, true, w->counters);
        use(s.pair_q, (size_t)max_slots * 4, true, w->pair_q);
        use(s.pair_leaf, (size_t)max_slots * 4, true, w->pair_leaf);
        use(s.pair_vbase, (size_t)max_slots * 4, true, w->pair_vbase);
        use(s.pair_thr, (size_t)max_slots * 8, true, w->pair_thr);
        use(s.slot_of, (size_t)nq * P * 4, true, w->slot_of);
        use(s.lutq, (size_t)max_quads * t.S * t.kp * 4 * 4, true, w->lutq);
        use(s.thr, (size_t)nq * 8, true, w->thr);
        use(s.cand_cnt, (size_t)nq * 4, true, w->cand_cnt);
        use(s.cand, (size_t)nq * p.cap * 8, true, w->cand);
        use(s.cand_key, (size_t)nq * m * 8, true, w->cand_key);
        use(s.cand_idx, (size_t)nq * m * 4, true, w->cand_idx);
        use(s.cand_dist, (size_t)nq * m * 4, true, w->cand_dist);
        use(s.cand_exact, (size_t)nq * m * 4, true, w->cand_exact);
        use(s.cand_row, (size_t)nq * m * 4, true, w->cand_row);
        use(s.cand_count, (size_t)nq * 4, true, w->cand_count);
        use(s.out_idx, (size_t)nq * k * 4, own_outputs, w->out_idx);
        use(s.out_dist, (size_t)nq * k * 4, own_outputs, w->out_dist);
        use(s.out_count, (size_t)nq * 4, own_outputs, w->out_count);
        use(s.rr_lb, (size_t)nq * m * 4, p.use_i8, w->rr_lb);
        use(s.rr_ub, (size_t)nq * m * 4, p.use_i8, w->rr_ub);
        use(s.lut8, (size_t)max_slots * t.S * 16 + 64, mfma, w->lut8);
        use(s.lut8_meta, (size_t)(max_slots + 4) * 16, mfma, w->lut8_meta);
        use(s.mfma_thr1, (size_t)(max_slots + 4) * 4, mfma, w->mfma_thr1);
        use(s.surv, ((size_t)nq + 63) / 64 * 64 * p.surv_stride * 4, mfma && p.sp_bitmap, w->surv);
        use(s.cand32, (size_t)nq * p.cap32 * 4, lists, w->cand32);
        use(s.cand32_codes, (size_t)nq * p.cap32 * code_words * 4, lists && t.ah_mode, w->cand32_codes);
        use(s.cand32_cnt, (size_t)nq * 4, lists, w->cand32_cnt);
        use(s.small_tickets, 64 * 4, small, w->small_tickets);
        use(s.proj_q, (size_t)nq * t.dim * 4, ix->proj.kind != 0, w->proj_q);
        use(s.wide_min, (size_t)nq * p.cap * 4, wide, w->wide_min);
        use(s.wide_ckey, (size_t)nq * p.wide_cap2 * 8, wide, w->wide_ckey);
        use(s.wide_ceb, (size_t)nq * p.wide_cap2 * 4, wide, w->wide_ceb);
        use(s.wide_cidx, (size_t)nq * p.wide_cap2 * 4, wide, w->wide_cidx);
        use(s.wide_cnt, 64 * 4, wide, w->wide_cnt);
    };
    if (allow_bytes) s.want(s.allow, allow_bytes);
    buffers([&](WsBuf &b, size_t bytes, bool used, auto &) {
        if (used) s.want(b, bytes);
    });
    SCANN_TRY(s.commit());
    *w = TxhWork{};
    static_cast<TxhPlan &>(*w) = p;
    w->q_stride = q_stride;
    w->max_slots = max_slots;
    w->max_quads = max_quads;
    buffers([](WsBuf &b, size_t, bool used, auto &field) {
        if (used) field = static_cast<std::remove_reference_t<decltype(field)>>(b.p);
    });
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

void scann::fill_empty(uint32_t nq, uint32_t k, uint32_t *out_idx, float *out_dist,
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

// The scratch of a call that will be enqueued on `st`: the one bound to that stream, else an unused one, else the
// least recently used one -- ordered behind its previous stream's last call.
int scann::device_slot(scann_hip_index *ix, hipStream_t st, DeviceSlot **out) {
    auto &ds = ix->dslots;
    if (!ds[0].sc) ds[0].sc = &ix->primary;
    const int n = device_slot_count();
    DeviceSlot *pick = nullptr;
    for (int i = 0; i < n && !pick; ++i)
        if (ds[i].used && ds[i].key == st) pick = &ds[i];
    for (int i = 0; i < n && !pick; ++i)
        if (!ds[i].used) pick = &ds[i];
    if (!pick) {
        pick = &ds[0];
        for (int i = 1; i < n; ++i)
            if (ds[i].tick < pick->tick) pick = &ds[i];
    }
    if (!pick->sc) {
        pick->own.reset(new SlotScratch());
        pick->sc = pick->own.get();
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
int scann::device_slot_done(DeviceSlot *sl, hipStream_t st) {
    SCANN_HIP_CHECK(hipEventRecord(sl->done, st));
    sl->done_valid = true;
    return SCANN_HIP_OK;
}

// Host-side users of the primary scratch (they run on ix->stream and synchronise before they return): wait for a
// device-entry call that may still be using it on another stream.
int scann::claim_primary_workspace(scann_hip_index *ix) {
    auto &d0 = ix->dslots[0];
    if (d0.used && d0.key != ix->stream) {
        if (d0.done_valid) SCANN_HIP_CHECK(hipStreamWaitEvent(ix->stream, d0.done, 0));
        d0.used = false;
        d0.done_valid = false;
        d0.key = nullptr;
    }
    return SCANN_HIP_OK;
}

// ix->mu held: the scratch bound to caller stream `st`, else the primary one
static SlotScratch &scratch_of_stream(scann_hip_index *ix, hipStream_t st) {
    SlotScratch *sc = &ix->primary;
    for (auto &d : ix->dslots)
        if (d.used && d.key == st && d.sc) sc = d.sc;
    return *sc;
}

static uint32_t max_slots() {
    static const uint32_t v = read_knobs().search_slots;
    return v;
}

// A search slot for a host-side call (SlotLock, handle.h)
int scann::acquire_slot(scann_hip_index *ix, SlotLock *out) {
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
            out->sc = &slot->sc;
            out->primary = false;
            return SCANN_HIP_OK;
        }
        lk.lock();   // every slot busy: queue on the primary
    }
    out->lock = std::move(lk);
    SCANN_TRY(claim_primary_workspace(ix));
    out->stream = ix->stream;
    out->sc = &ix->primary;
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

// One small host call whose queries and result rows live in pinned host memory the kernels access in place:
// [queries | idx | dist | count | flags], each part 256-aligned.  begin() before the launch, wait() and copy_out() after.
struct PinnedCall {
    char *hp = nullptr;
    size_t ob = 0, off_idx = 0, off_dist = 0, off_cnt = 0, off_flag = 0;
    uint32_t nq = 0, seq = 0;
    // grows the buffer, copies the queries in and binds queries, out_* and the completion flags into *w
    int begin(PinBuf &pin, const float *queries, uint32_t nq_, uint32_t q_stride, uint32_t k, TxhWork *w) {
        nq = nq_;
        const size_t qb = (size_t)nq * q_stride * 4;
        ob = (size_t)nq * k * 4;
        off_idx = (qb + 255) & ~(size_t)255;
        off_dist = off_idx + ((ob + 255) & ~(size_t)255);
        off_cnt = off_dist + ((ob + 255) & ~(size_t)255);
        off_flag = off_cnt + (((size_t)nq * 4 + 255) & ~(size_t)255);
        SCANN_TRY(pin.ensure(off_flag + (size_t)nq * 4 + 256));
        hp = static_cast<char *>(pin.host);
        char *dp = static_cast<char *>(pin.dev);
        std::memcpy(hp, queries, qb);
        seq = ++pin.seq ? pin.seq : ++pin.seq;   // (never 0)
        // The flag words sit wherever THIS call's layout puts them: an earlier call (other nq / k / stride) may
        // have left result words there, and any of those can equal seq.  Zero them before the launch.
        std::memset(hp + off_flag, 0, (size_t)nq * 4);
        w->queries = reinterpret_cast<const float *>(dp);
        w->out_idx = reinterpret_cast<uint32_t *>(dp + off_idx);
        w->out_dist = reinterpret_cast<float *>(dp + off_dist);
        w->out_count = reinterpret_cast<uint32_t *>(dp + off_cnt);
        w->small_done = reinterpret_cast<uint32_t *>(dp + off_flag);
        w->small_seq = seq;
        return SCANN_HIP_OK;
    }
    int wait(hipStream_t stream) const {
        return wait_small_done(stream, reinterpret_cast<const volatile uint32_t *>(hp + off_flag), nq, seq);
    }
    // the [nq] count words as the kernels left them (the wide pipeline: 0xFFFFFFFF = its compact arrays overflowed)
    const uint32_t *counts() const { return reinterpret_cast<const uint32_t *>(hp + off_cnt); }
    void copy_out(uint32_t *out_idx, float *out_dist, uint32_t *out_count) const {
        std::memcpy(out_idx, hp + off_idx, ob);
        std::memcpy(out_dist, hp + off_dist, ob);
        std::memcpy(out_count, hp + off_cnt, (size_t)nq * 4);
    }
};

static int txh_search_host(scann_hip_index *ix, const float *queries, uint32_t nq,
                           uint32_t q_stride, uint32_t k, const scann_hip_search_opts *opts,
                           uint32_t *out_idx, float *out_dist, uint32_t *out_count) {
    SlotLock sl;
    SCANN_TRY(acquire_slot(ix, &sl));
    TxhWorkspace &ws = sl.sc->ws;
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
            PinnedCall pc;
            SCANN_TRY(pc.begin(sl.sc->pin, queries, nq, q_stride, k, &w));
            const TimedEvents tv = ix->timing_begin(sl.primary);   // kernel timing follows the primary slot only
            SCANN_TRY(txh_launch_search(ix->tx, w, false, stream, tv.ev0, tv.ev1));
            ix->timing_end(tv, true, txh_kernel_name(ix->tx, p, /*pinned=*/true));
            SCANN_TRY(pc.wait(stream));
            if (p.pipeline == TxhPipeline::Wide) {   // the wide pipeline's compact arrays can overflow: count row 0xFFFFFFFF -> the batched pipeline
                bool overflow = false;
                for (uint32_t i = 0; i < nq; ++i) overflow = overflow || pc.counts()[i] == 0xFFFFFFFFu;
                if (overflow) continue;
            }
            pc.copy_out(out_idx, out_dist, out_count);
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
        const TimedEvents tv = ix->timing_begin(sl.primary);
        SCANN_TRY(launch_txh(ix, w, stream, tv.ev0, tv.ev1));
        ix->timing_end(tv, true, txh_kernel_name(ix->tx, p, /*pinned=*/false));
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

// scann_hip_search_opts.allow_bitmap of a brute-force search (no filter: bitmap null)
BfFilter scann::bf_filter_of(const scann_hip_search_opts *opts, const Knobs &kn) {
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
    TxhWorkspace &ws = sl.sc->ws;
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
    TxhWork w{};
    w.nq = nq; w.q_stride = q_stride; w.P = 1; w.m = kk; w.k = k; w.cap = n; w.exact_reorder = false;
    w.no_threshold = true; w.need_sorted_cands = 0;
    w.allow = flt.bitmap ? ws.allow.as<uint64_t>() : nullptr; w.allow_bits = flt.bitmap ? allow_bits : 0;
    w.tokens = ws.tokens.as<uint32_t>(); w.token_dists = ws.token_dists.as<float>();
    w.vbase = ws.vbase.as<uint32_t>(); w.sbase = ws.sbase.as<uint32_t>(); w.st = 1;
    w.counters = ws.counters.as<uint32_t>(); w.cand = ws.cand.as<uint64_t>();
    w.pipeline = TxhPipeline::Small; w.scan = TxhScan::Exact; w.small_max_leaf = n;
    plan_small_launch(ix->bfx, kn, &w);
    w.small_tickets = ws.small_tickets.as<uint32_t>();
    PinnedCall pc;
    SCANN_TRY(pc.begin(sl.sc->pin, queries, nq, q_stride, k, &w));
    SCANN_TRY(txh_launch_search(ix->bfx, w, false, sl.stream, nullptr, nullptr));
    SCANN_TRY(pc.wait(sl.stream));
    pc.copy_out(out_idx, out_dist, out_count);
    return SCANN_HIP_OK;
}

// The enqueue-only search in scratch sc on stream st, device pointers throughout.
// dsl != null: scann_hip_search_batched_device with ix->mu held and the stream's scratch chosen (kernel timing and
// the slot's completion event follow the call).  dsl == null: a host entry point that owns sc through its
// SlotLock and synchronises by itself; it touches none of the handle's primary-slot state.
int scann::search_device_ws(scann_hip_index *ix, DeviceSlot *dsl, SlotScratch &sc, TxhPipeline widest,
                            const float *d_queries, uint32_t nq, uint32_t q_stride, uint32_t k,
                            const scann_hip_search_opts *opts, uint32_t *d_out_idx, float *d_out_dist,
                            uint32_t *d_out_count, hipStream_t st) {
    const Knobs kn = read_knobs();
    if (ix->kind == KIND_BF) {
        SCANN_TRY(refuse_allow_stride(opts, "brute-force handles"));
        const TimedEvents tv = ix->timing_begin(dsl != nullptr);
        const BfFilter flt = bf_filter_of(opts, kn);   // (a device pointer on this path)
        const bool shortlist = !flt.bitmap && !(opts && opts->bf_exact) && bf_shortlist_eligible(ix->bf, nq, k, kn);
        int s = bf_search_device(ix->bf, sc.bfw, d_queries, nq, q_stride, k, shortlist, kn.bf_shortlist_tail, flt,
                                 d_out_idx, d_out_dist, d_out_count, st, tv.ev0, tv.ev1);
        if (dsl && s == SCANN_HIP_OK) s = device_slot_done(dsl, st);
        ix->timing_end(tv, s == SCANN_HIP_OK, shortlist ? "bf_bf16_kernel" : bf_pass_kernel_name(ix->bf, nq));
        return s;
    }
    TxhPlan p;
    SCANN_TRY(check_allow_stride(opts));
    SCANN_TRY(plan_txh_search(ix, k, opts, nq, false, widest, kn, &p));
    if (p.m == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "pre-reorder candidate count is 0");
    TxhWork w;
    SCANN_TRY(ensure_txh_workspace(ix, sc.ws, p, false, q_stride, false, &w));
    w.queries = d_queries;
    w.out_idx = d_out_idx;
    w.out_dist = d_out_dist;
    w.out_count = d_out_count;
    if (opts && opts->allow_bitmap) {   // device pointer on this path
        w.allow = opts->allow_bitmap;
        w.allow_bits = opts->allow_bitmap_bits;
        w.allow_stride = opts->allow_bitmap_stride;
    }
    if (dsl) ix->last_work = w;
    const TimedEvents tv = ix->timing_begin(dsl != nullptr);
    SCANN_TRY(launch_txh(ix, w, st, tv.ev0, tv.ev1));
    if (dsl) SCANN_TRY(device_slot_done(dsl, st));
    ix->timing_end(tv, true, txh_kernel_name(ix->tx, p, /*pinned=*/false));
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
        const TimedEvents tv = ix->timing_begin(sl.primary);
        const bool shortlist = !flt.bitmap && !(opts && opts->bf_exact) && bf_shortlist_eligible(ix->bf, nq, k, kn);
        int s = bf_search_host(ix->bf, sl.sc->bfw, queries, nq, q_stride, k, shortlist, kn.bf_shortlist_tail, flt, out_idx,
                               out_dist, out_count, sl.stream, tv.ev0, tv.ev1);
        ix->timing_end(tv, s == SCANN_HIP_OK, shortlist ? "bf_bf16_kernel" : bf_pass_kernel_name(ix->bf, nq));
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

int scann_hip_index_reserve(scann_hip_index *ix, uint32_t max_nq, uint32_t max_k,
                            const scann_hip_search_opts *opts) {
    if (!ix) return fail(SCANN_HIP_INVALID_ARGUMENT, "index is null");
    std::lock_guard<std::mutex> lock(ix->mu);
    SCANN_TRY(set_device(ix->ctx));
    if (ix->kind == KIND_BF) return bf_reserve(ix->bf, ix->primary.bfw, max_nq, max_k, opts && opts->allow_bitmap);
    TxhPlan p;
    SCANN_TRY(plan_txh_search(ix, max_k, opts, max_nq, false, TxhPipeline::Staged, read_knobs(), &p));
    TxhWork w;
    // (a host call's copy of its bitmap, or of its max_nq bitmaps allow_bitmap_stride words apart)
    SCANN_TRY(check_allow_stride(opts));
    const size_t allow_bytes = opts && opts->allow_bitmap ? std::max<size_t>(allow_copy_words(opts, max_nq), 1) * 8 : 0;
    return ensure_txh_workspace(ix, ix->primary.ws, p, false, 0, false, &w, allow_bytes);
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
    DeviceSlot *dsl = nullptr;
    SCANN_TRY(device_slot(ix, st, &dsl));
    return search_device_ws(ix, dsl, *dsl->sc, TxhPipeline::Wide, d_queries, nq, q_stride, k, opts, d_out_idx, d_out_dist,
                            d_out_count, st);
}

int scann_hip_index_last_device_status(scann_hip_index *ix, void *hip_stream) {
    if (!ix) return fail(SCANN_HIP_INVALID_ARGUMENT, "index is null");
    SCANN_TRY(set_device(ix->ctx));
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::lock_guard<std::mutex> lock(ix->mu);
    const SlotScratch &sc = scratch_of_stream(ix, st);
    const TxhWorkspace *ws = &sc.ws;
    if (ix->kind == KIND_BF) return bf_last_status(sc.bfw, st);
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
    const TxhWorkspace *ws = &scratch_of_stream(ix, st).ws;
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
    *out_bytes = scratch_of_stream(ix, st).ws.surv.need;
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
    const TxhWorkspace *ws = &scratch_of_stream(ix, st).ws;
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
    DeviceSlot *dsl = nullptr;
    SCANN_TRY(device_slot(ix, st, &dsl));
    TxhWork w;
    SCANN_TRY(ensure_txh_workspace(ix, dsl->sc->ws, p, false, q_stride, false, &w));
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
    const TimedEvents tv = ix->timing_begin(true);
    SCANN_TRY(txh_launch_search(ix->tx, w, true, st, tv.ev0, tv.ev1));
    SCANN_TRY(device_slot_done(dsl, st));
    ix->timing_end(tv, true, txh_kernel_name(ix->tx, p, /*pinned=*/false));
    return SCANN_HIP_OK;
}

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
    SCANN_TRY(ensure_txh_workspace(ix, ix->primary.ws, p, true, q_stride, true, &w));
    SCANN_HIP_CHECK(hipMemcpyAsync(ix->primary.ws.queries.p, queries, (size_t)nq * q_stride * 4,
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

}  // extern "C"

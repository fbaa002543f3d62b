// txh.h -- device-side views + launchers of the Tree-X-Hybrid / AsymmetricHasher path.
#pragma once
#include "common.h"

namespace scann {

// Tunables of the scan decomposition (see DESIGN.md "Leaf scan").
constexpr uint32_t kScanThreads = 256;
#ifndef SCANN_SCAN_PPT
#define SCANN_SCAN_PPT 2
#endif
constexpr uint32_t kScanPPT = SCANN_SCAN_PPT;              // points per thread per chunk
constexpr uint32_t kScanTP = kScanThreads * kScanPPT;     // points per tile chunk
constexpr uint32_t kScanQuadsPerTile = 32;                // query quads per tile
#ifndef SCANN_SCAN_DEPTH
#define SCANN_SCAN_DEPTH 1
#endif
#ifndef SCANN_SCAN_WAVES
#define SCANN_SCAN_WAVES 6
#endif
constexpr uint32_t kScanDepth = SCANN_SCAN_DEPTH;         // gather software-pipeline depth (subspaces)
constexpr uint32_t kScanWaves = SCANN_SCAN_WAVES;         // workgroups per CU = waves per SIMD (S <= 32)
constexpr uint32_t kResThreads = 512;                     // resident-table scan: threads per workgroup
constexpr uint32_t kResQuads = 4;                         // ... quads whose tables stay in LDS
constexpr uint32_t kSortCap = 16384;                      // u64 keys sorted in LDS (select)
#ifndef SCANN_SAMPLE_TARGET
#define SCANN_SAMPLE_TARGET 32768
#endif
#ifndef SCANN_SAMPLE_MIN
#define SCANN_SAMPLE_MIN 4096
#endif
constexpr uint32_t kSampleTarget = SCANN_SAMPLE_TARGET;   // max sample points per query (LDS of the select)
constexpr uint32_t kSampleMin = SCANN_SAMPLE_MIN;         // min sample points per query
constexpr uint32_t kMaxPreReorderK = 8192;                // m limit of the LDS select
constexpr uint32_t kMaxPartitionsToSearch = 4096;
constexpr uint32_t kMaxLeavesSelect = 16384;              // L limit of the LDS leaf sort
constexpr uint32_t kSelectThreads = 1024;
constexpr uint32_t kInvalid = 0xFFFFFFFFu;
constexpr uint32_t kSmallBatch = 16;                      // queries per call the small-batch pipeline takes
constexpr uint32_t kSmallMaxStream = 262144;              // ... longest candidate stream (points) it takes
constexpr uint32_t kSmallMaxCandidates = 1024;            // ... largest pre_reorder_k
// the wide few-query pipeline (txh.hip "Few queries, long streams"): three launches, every stage spread over the chip
constexpr uint32_t kWideBatch = 4;                        // queries per call it takes
constexpr uint32_t kWideMaxStream = 4u << 20;             // ... longest candidate stream (points)
constexpr uint32_t kWideMaxCandidates = 8192;             // ... largest pre_reorder_k
constexpr uint32_t kWideMinStream = 16384;                // ... and the stream from which it replaces the pipeline above
constexpr int kWideRep = 4;                               // ... ADC stream positions per thread of its scan
constexpr uint32_t kFusedChunk = kSelectThreads;          // one-launch small pipeline: stream positions per workgroup
constexpr uint32_t kFusedMaxWgs = 512;                    // ... nq x workgroups per query above which three launches are used
// points per work item of the sparse prefilter's 64-pair form (adc_smfmac_body, CT = 2: two column tiles per point tile)
#ifndef SCANN_SP_RANGE64
#define SCANN_SP_RANGE64 1024
#endif
constexpr uint32_t kSpRange64 = SCANN_SP_RANGE64;
constexpr uint32_t kDecodeStage = 512;                    // selected leaves whose decode tables are staged in LDS
constexpr uint32_t kThrTailMaxRank = 384;                 // J above this takes threshold_select_kernel

// ---- threshold sampling plan (shared by host buffer sizing and the device kernels) ----
// Every st-th point of each selected leaf is scored ahead of the scan (adc_sample_kernel,
// the same tiled LUT16 gather as the scan); the threshold is the j-th smallest sample
// distance (threshold_select_kernel).  One stride per batch, so that all queries of a
// tile share the sampled points' codes.  j == m gives a deterministic bound (any
// subset's m-th smallest bounds the stream's m-th smallest); j < m is a 6-sigma
// statistical bound that select_rerank VERIFIES (>= m survivors, else the host entry
// retries without a threshold), so results stay exact either way.
__host__ __device__ static inline uint32_t sample_stride(uint32_t total) {
    uint32_t ns = total / 16u;
    if (ns < kSampleMin) ns = kSampleMin;
    if (ns > kSampleTarget) ns = kSampleTarget;
    uint32_t st = (total + ns - 1u) / ns;
    return st ? st : 1u;
}
// Stride and per-query sample capacity for a batch whose longest stream (sum of the P
// largest local leaves) is max_stream: capacity = max_stream / st + P <= kSampleTarget.
static inline void sample_plan(uint64_t max_stream, uint32_t P, uint32_t *st_out, uint32_t *scap_out) {
    const uint32_t ms = (uint32_t)(max_stream > 0xFFFFFFFFull ? 0xFFFFFFFFull : max_stream);
    uint32_t st = sample_stride(ms);
    for (;;) {
        const uint64_t scap = (((uint64_t)(ms + st - 1u) / st + P) + 3u) & ~3ull;   // rows 16-B aligned
        if (scap <= kSampleTarget || P >= kSampleTarget - 4) {
            *st_out = st;
            *scap_out = (uint32_t)(scap < 4 ? 4 : scap);
            return;
        }
        st += 1 + st / 8;
    }
}
// 0 = use no threshold.
__host__ __device__ static inline uint32_t sample_rank(uint32_t m, uint32_t st) {
    if (m == 0) return 0;
    const float r = (float)m / (float)st;
    const float s = 0.5f * (6.0f + sqrtf(36.0f + 4.0f * r));
    const float jp = s * s + 2.0f;
    uint32_t j = jp >= (float)m ? m : (uint32_t)jp;
    if (j > m) j = m;
    if (j == 0) j = 1;
    return j;
}

struct TxhIndexDev {
    uint32_t dim, stride, L, S, K, dsub, nw;
    uint32_t code_bits, kp;       // 4-bit codes / 16 table slots (K <= 16) or 8-bit / 256 slots
    uint64_t n_local;
    const float *centers;         // [L][dim]; nullptr in AsymmetricHasher mode
    const float *centers_t;       // [dim][centers_pitch] transposed copy (small-batch leaf selection), or nullptr
    uint32_t centers_pitch;
    const uint32_t *leaf_off;     // [L+1] local CSR offsets
    const uint32_t *leaf_gsize;   // [L] global leaf sizes (== local when unsharded)
    const uint32_t *leaf_ids;     // [n_local] datapoint index of CSR row; nullptr = identity
    const uint32_t *codes;        // [n_local][nw] packed 4-bit codes, 8 subspaces per word
    const uint32_t *codes_sp;     // [n_local][sp_words(S)] the same codes as operand planes of the 2:4-sparse MFMA prefilter
                                  // (txh_prefilter.hip K6e; 4-bit codes only), or nullptr
    const float *rows;            // re-rank rows; CSR order if rows_csr else by datapoint idx
    const int8_t *rows8;          // the same rows as int8 (per-row scale) for the re-rank filter, or nullptr
    int rows8_fmt;                // 0 = int8, 1 = the reference's FP8 E4M3 codes (quantization/fp8.rs)
    const void *rows8_meta;       // [n_rows] float2 {scale, ||x - s q||}
    int rows8_uniform;            // int8 store with ONE scale and ONE error bound for all rows (rows8_scale, rows8_emax)
    float rows8_scale, rows8_emax;
    int rows_csr;
    const float *codebook;        // [S][K][dsub]
    int use_residuals;
    int ah_mode;                  // single implicit leaf, no centroid stage
    int measure;                  // measure of the exact re-rank and of the exact leaf scan
    int exact_scan;               // SearchMode::Partitioned: no codes, rows of the leaves scored exactly
    // scann_hip_txh_create_quantized: the re-rank rows as the caller stores them (indexed as `rows` would be, `stride`
    // ELEMENTS apart); `rows` and `rows8` are then nullptr and the re-rank is rerank_quant_kernel (txh_rows.hip)
    const void *qrows;
    int qfmt;                     // SCANN_HIP_ROWS_BF16 / _FP8_E4M3 / _INT8; 0 = f32 rows or none
    float inv_mult;               // int8 rows: value = (float)i8 * inv_mult
    // the space of the re-rank rows: `rows` are row_dim wide and row_stride apart.  Equal to dim / stride on every
    // handle but a projected one (scann_hip_txh_create_projected), whose centres, codebook and tables live at `dim` =
    // the projection's out_dim while the rows keep the original dimensionality.  Read by the exact re-rank alone.
    uint32_t row_dim, row_stride;
};

// points of one scan tile chunk for this index's code layout (Codec<S, bits>::TP in txh_dev.h)
static inline uint32_t scan_tile_points(const TxhIndexDev &ix) {
    return kScanThreads * (ix.code_bits == 4 ? kScanPPT : 8u);
}

// counters[] slots
enum {
    CNT_TOTAL_QUADS = 0, CNT_TOTAL_TILES = 1, CNT_QUEUE_HEAD = 2, CNT_STATUS = 3,
    CNT_TOTAL_STILES = 4, CNT_SQUEUE_HEAD = 5, CNT_N = 8,
    // eight scan-tile queues, one 128-byte line each: WGs of XCD x (blockIdx % 8) pull tiles
    // t = x (mod 8) from queue x first and steal from the others when it runs dry.  One
    // shared counter made every tile grab a ~100 ns serialized cross-XCD atomic.
    CNT_XQ = 32, CNT_XQ_STRIDE = 32, CNT_XS = CNT_XQ + 8 * CNT_XQ_STRIDE /* sample pass */,
    CNT_WORDS = CNT_XS + 8 * CNT_XQ_STRIDE
};

// Pipeline of a search call: the batched one (sample, threshold, scan, select, re-rank), the small-batch one
// ("Small batches": three launches or one, dense candidate lists), the wide few-query one ("Few queries, long streams").
enum class TxhPipeline : uint8_t { Staged, Small, Wide };
// Scan kernel of the batched pipeline: the f32 LDS-gather scan, its resident-table form (long leaves), the
// integer-MFMA prefilter + exact refine on 32- or 16-pair dense tiles or 32-pair tiles of the 2:4-sparse MFMA, or the
// exact leaf scan (SearchMode::Partitioned).
enum class TxhScan : uint8_t { Gather, Resident, Mfma32, Mfma16, Smfmac, Exact };

// Every path decision of one search call and the sizes they were derived from (api_search.hip plan_txh_search).
struct TxhPlan {
    uint32_t nq, P, m, k;
    uint32_t cap;              // candidate slots per query
    bool exact_reorder;
    bool no_threshold;         // retry mode / dense lists: keep every scanned point as a candidate
    TxhPipeline pipeline;
    TxhScan scan;
    uint32_t st, scap, sqpt;   // sample stride, per-query sample capacity, quads per sample tile
    uint32_t qpt;              // quads per scan tile (gather scan)
    uint32_t res_cl;           // chunks per tile of the resident-table scan
    uint32_t cap32;            // survivors per query of the MFMA prefilter
    bool sp_words;             // sparse prefilter's survivor flush: word-parallel (else lanes walk their own words)
    bool sp_pairs64;           // sparse prefilter's items: 64 pairs x 1024 points (else 32 x 2048); S <= 32, lane-walk flush
    bool sp_bitmap;            // ... 64-pair items that end by storing their survivor bitmap (surv); the refine walks it
    uint32_t surv_stride;      // words per query of surv: ranges of kSpRange64 points x 32
    bool codes_in_list;        // prefilter survivors carry their packed codes / plane rows
    bool thr_ties;             // filter bound on (distance, stream position); false: on the distance alone
    bool thr_tail;             // filter bound by threshold_tail_kernel (else threshold_select_kernel)
    bool sample_mfma;          // flat hashers: the sample as integer-MFMA sums (u16), bound by threshold_tail16_kernel
    bool fused;                // small pipeline in one launch (small_fused_kernel)
    uint32_t chunk, grid;      // one-launch small / wide pipeline: stream positions per workgroup, workgroups per query
    uint32_t small_max_leaf;   // longest local leaf (grid of the three-launch small scan)
    uint32_t wide_cap2;        // wide pipeline: entries per query of the compact candidate arrays
    bool select_direct;        // the unsorted select of a long list may read it straight from global memory
    bool select_regs;          // ... and ranks it in registers after one read (select_regs_kernel)
    bool use_i8;               // int8 row filter in front of the exact re-rank (needs ix.rows8)
    bool i8_expand;            // its brackets by the expanded square, one epilogue per wave (else per dimension, per round)
    bool local_prune;          // local stage of a sharded search: the filter's prefix form (+inf for hopeless candidates)
};

// A plan bound to its buffers.
struct TxhWork : TxhPlan {
    uint32_t q_stride;
    int need_sorted_cands;     // the caller reads cand_* (parity outputs): keep them sorted
    const uint64_t *allow;     // device allow-bitmap (bit = datapoint index) or nullptr
    uint64_t allow_bits;       // bitmap capacity in bits; indices >= capacity are not allowed
    uint64_t allow_stride;     // 64-bit words from query i's bitmap to query i + 1's; 0 = one bitmap for the batch
    const float *queries;      // device
    // projected handles: the queries the re-rank reads (the caller's, row_dim wide; `queries` are then their
    // projections, written to proj_q at the head of the call).  nullptr: the re-rank reads `queries` / q_stride.
    const float *rr_queries;
    uint32_t rr_q_stride;
    float *proj_q;             // [nq][dim] projected queries of a projected handle
    float *cdist;              // [nq][L]
    uint32_t *tokens;          // [nq][P]
    float *token_dists;        // [nq][P]
    uint32_t *vbase;           // [nq][P+1] prefix of global leaf sizes in token order
    uint32_t *rr_lb, *rr_ub;   // [nq][m] ordered lower / upper bounds of the candidates' exact distances
    int8_t *lut8;              // [max_slots][S][16] quantised tables (value - 128)
    void *lut8_meta;           // [max_slots] {f64 bias_sum, f64 scale}
    int *mfma_thr1;            // [max_slots] integer pass bound + 1 of every pair slot
    uint32_t *cand32_cnt;      // [nq]
    uint32_t *cand32;          // [nq][cap32] stream positions of the prefilter's survivors
    uint32_t *cand32_codes;    // [nq][cap32][S/8] their packed codes (written next to the positions)
    uint32_t *surv;            // [nq rounded up to 64][surv_stride] survivor bitmaps (sp_bitmap; then no cand32*)
    uint32_t *small_done;      // small-batch host calls: [nq] pinned completion flags (or nullptr) ...
    uint32_t small_seq;        // ... and the value the finish kernel stores there after the result rows
    uint32_t *small_tickets;   // [kSmallBatch] ticket counters of the one-launch pipeline (zero between launches)
    // the wide few-query pipeline
    uint32_t *wide_min;        // [nq][cap] ordered approximate distance: minimum of each group of stream positions
    uint64_t *wide_ckey;       // [nq][wide_cap2] merge keys of the candidates under the pivot ...
    uint32_t *wide_ceb;        // ... their ordered exact distances (approximate ones without re-ordering) ...
    uint32_t *wide_cidx;       // ... and datapoint indices
    uint32_t *wide_cnt;        // [nq] entries appended
    uint32_t *sbase;           // [nq][P+2] prefix of per-leaf sample counts; [P]=samples, [P+1]=local points
    uint32_t *pair_sbase;      // [max_slots]
    uint32_t *stile_off;       // [L+1] tile table of the sample pass
    uint32_t *samp;            // [nq][scap] ordered(approx distance) of the sampled points; with sample_mfma
                               // [nq][scap] u16: their quantised sums (adc_sample_mfma_kernel)
    uint32_t *leaf_cnt;        // [L]
    uint32_t *leaf_cursor;     // [L]
    uint32_t *pair_off;        // [L+1] (slots, padded to quads)
    uint32_t *tile_off;        // [L+1]
    uint32_t *counters;        // [CNT_N]
    uint32_t *pair_q;          // [max_slots]
    uint32_t *pair_leaf;       // [max_slots]
    uint32_t *pair_vbase;      // [max_slots]
    uint32_t *slot_of;         // [nq][P]
    uint32_t max_slots, max_quads;
    float *lutq;               // [max_quads][S][16][4]
    uint64_t *thr;             // [nq]
    uint64_t *pair_thr;        // [max_slots] the same bound per (query, leaf) pair slot
    uint32_t *cand_cnt;        // [nq]
    uint64_t *cand;            // [nq][cap]
    uint64_t *cand_key;        // [nq][m] selected merge keys
    uint32_t *cand_idx;        // [nq][m]
    float *cand_dist;          // [nq][m] approximate
    float *cand_exact;         // [nq][m]
    uint32_t *cand_row;        // [nq][m] re-rank row of each candidate
    uint32_t *cand_count;      // [nq]
    uint32_t *out_idx;         // [nq][k]
    float *out_dist;           // [nq][k]
    uint32_t *out_count;       // [nq]
};

static inline bool txh_scan_is_mfma(TxhScan s) { return s == TxhScan::Mfma32 || s == TxhScan::Mfma16 || s == TxhScan::Smfmac; }

// Enqueue the whole search pipeline on `stream`.  local_only: stop after the local
// top-m + exact distances (multi-GPU local stage).
int txh_launch_search(const TxhIndexDev &ix, const TxhWork &w, bool local_only,
                      hipStream_t stream, hipEvent_t ev_scan_begin, hipEvent_t ev_scan_end);

// false where the batched exact leaf scan (Partitioned mode) refuses this dim for want of LDS: the small-batch
// pipeline is then not planned either, so that the dims a search refuses do not depend on the batch size
bool txh_exact_scan_fits(const TxhIndexDev &ix);

int txh_launch_partition_only(const TxhIndexDev &ix, const TxhWork &w, hipStream_t stream);

int txh_launch_merge(uint32_t world, uint32_t nq, uint32_t m_local, uint32_t m, uint32_t k,
                     size_t rank_stride_bytes, const uint64_t *d_keys, const uint32_t *d_idx, const float *d_exact,
                     const uint32_t *d_count, uint32_t *d_out_idx, float *d_out_dist,
                     uint32_t *d_out_count, uint32_t *d_status, hipStream_t stream,
                     const uint32_t *d_qoff = nullptr /* compact lists: [world][nq] element offsets */);

int txh_launch_pack_blocks(uint32_t world, uint32_t nq, uint32_t m_local, const uint64_t *d_keys,
                           const uint32_t *d_idx, const float *d_exact, const uint32_t *d_count,
                           void *d_out, size_t block_bytes, hipStream_t stream);

int txh_launch_lut_from_query(const TxhIndexDev &ix, const float *d_queries, uint32_t nq,
                              uint32_t q_stride, const uint32_t *d_leaf_for_query,
                              float *d_out_lut, hipStream_t stream);

int txh_launch_adc_distances(const TxhIndexDev &ix, const float *d_luts, uint32_t nq,
                             float *d_out, hipStream_t stream);

int launch_lut16_u8_batch(const uint8_t *d_packed, const uint8_t *d_lut8, uint32_t S,
                          uint64_t n, float bias, float mult, float *d_out,
                          hipStream_t stream);

// Lut16SimdTables::from_float_tables (hashes/lut16_simd.rs:39-90); d_bias_mult = {bias, multiplier}
// int8 copy of n rows (per-row scale = max|x| / 127) + {scale, error norm} per row
int launch_transpose_centers(const float *d_centers, uint32_t L, uint32_t dim, uint32_t pitch, float *d_out,
                             hipStream_t st);
int launch_rows_fp8_build(const float *d_rows, uint64_t n, uint32_t dim, uint32_t stride, uint8_t *d_rows8,
                          void *d_meta, uint32_t *d_mismatch, hipStream_t st);
int launch_fp8_quantize(const float *d_values, uint64_t n, float scale, int format, uint8_t *d_out, hipStream_t st);
int launch_fp8_dequantize(const uint8_t *d_bits, uint64_t n, float scale, int format, float *d_out, hipStream_t st);
int launch_fp8_one_to_many(const float *d_query, uint32_t dim, const uint8_t *d_db, uint64_t stride, uint64_t n,
                           int dot, float *d_out, hipStream_t st);
int launch_rows_i8_build(const float *d_rows, uint64_t n, uint32_t dim, uint32_t stride, int8_t *d_rows8,
                         void *d_meta, hipStream_t stream, float uni_scale = 0.0f);

int launch_lut16_quantize(const float *d_tables, uint32_t S, uint8_t *d_lut8, float *d_bias_mult,
                          hipStream_t stream);

// Operand planes of the sparse-MFMA prefilter (txh_prefilter.hip K6e) from the packed 4-bit codes: words per point and the
// build kernel.
static inline uint32_t sp_words(uint32_t S) { return 4u * ((((S - 4u) / 4u + 1u) + 7u) / 8u); }
int launch_codes_sp_build(const uint32_t *d_codes, uint64_t n, uint32_t S, uint32_t *d_codes_sp, hipStream_t stream);

int launch_encode(const float *d_codebook, uint32_t S, uint32_t K, uint32_t dsub,
                  const float *d_rows, uint64_t n, uint32_t stride, const float *d_centers,
                  const uint32_t *d_leaf_of_row, uint8_t *d_out, hipStream_t stream);

}  // namespace scann

// bf.h -- brute-force path (BruteForceSearcher, brute_force/searcher.rs:77-208).
#pragma once
#include "common.h"
#include "knobs.h"

namespace scann {

struct BfIndexDev {
    const float *rows;   // [n][stride]; nullptr when the rows are quantized (fmt != 0)
    uint64_t n;
    uint32_t dim, stride;
    int measure;         // scann_hip_measure
    // quantized rows (scann_hip_bf_create_quantized): fmt = SCANN_HIP_ROWS_BF16 / _FP8_E4M3 / _INT8, qrows =
    // [n][stride] elements of that format; every pass takes bf_quant_kernel.  fmt 0 = f32 rows above.
    int fmt;
    const void *qrows;
    float inv_mult;      // INT8: value = (float)i8 * inv_mult
    // bf16 shortlist (bf_shortlist_*): a bf16 copy of the rows [n][dim], f32 squared norms and the
    // largest row norm; nullptr when the index does not qualify (dim % 16, size)
    const uint16_t *rows_b, *rows_bl;   // hi and lo halves of the split bf16 copy
    const float *norm2;
    float max_norm;
};

struct BfWorkspace {
    DevBuf queries, sample, thr, cand_cnt, cand, counters, out_idx, out_dist, out_count;
    DevBuf q_b, q_bl, q_n2, sl_idx, sl_approx, sl_cnt, sl_exact, sl_fail;   // bf16 shortlist path
    DevBuf allow, ids, allow_sums;   // filtered search: bitmap copy, compacted id list, per-block popcounts
};

// Allow-list of one search (scann_hip_search_opts.allow_bitmap / allow_bitmap_bits); bitmap == nullptr: none.
// A filtered search answers as an unfiltered search over the allowed rows alone, indices mapped back.
struct BfFilter {
    const uint64_t *bitmap = nullptr;   // host pointer in the host entries, device pointer in bf_search_device
    uint64_t bits = 0;
    int mechanism = 0;                  // Knobs::bf_filter: 0 by the rule below, 1 compacted id list, 2 bit test
    double compact_max_fraction = 0.0;  // Knobs::bf_filter_compact_max: compacted up to this allowed fraction
};

// Allowed rows of an n-row index: set bits below min(bits, n).  The host mirror of the device compaction.
uint64_t bf_allowed_count(const uint64_t *bitmap, uint64_t bits, uint64_t n);

// bf16 copy + squared norms of the rows (index creation); *max_norm = largest row norm.
int bf_build_shortlist_data(const BfIndexDev &ix, DevBuf &rows_b, DevBuf &rows_bl, DevBuf &norm2,
                            float *max_norm, hipStream_t stream);
// true if searches on this index may take the bf16-shortlist path for (nq, k)
bool bf_shortlist_eligible(const BfIndexDev &ix, uint32_t nq, uint32_t k, const Knobs &kn);

constexpr uint32_t kBfSampleRows = 8192;   // rows of the threshold sample (== LDS sort size)

// filtered: also what a filtered host search needs (the device entry reads the caller's bitmap in place)
int bf_reserve(const BfIndexDev &ix, BfWorkspace &w, uint32_t max_nq, uint32_t max_k, bool filtered);

const char *bf_pass_kernel_name(const BfIndexDev &ix, uint32_t nq);
// true if the pass kernels accept this index's dim at EVERY batch size (the last resort's queries fit the LDS): a
// caller with a path of its own for some batch sizes must not take it past this ceiling, or the dims it refuses
// would depend on the batch size
bool bf_pass_fits(const BfIndexDev &ix);

// Host-pointer entry (copies in/out, synchronises).  shortlist: take the bf16-shortlist path first
// (bf_shortlist_eligible), whose bound misses with probability `tail`; queries it cannot verify are repeated exactly.
int bf_search_host(const BfIndexDev &ix, BfWorkspace &w, const float *queries, uint32_t nq,
                   uint32_t q_stride, uint32_t k, bool shortlist, double tail, const BfFilter &flt, uint32_t *out_idx,
                   float *out_dist, uint32_t *out_count, hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1);

// Device-pointer entry (enqueue only).
// shortlist: the bf16-shortlist path (status Aborted in the counters if a query's result could not be verified:
// repeat without it).  A filtered search takes the bit test at the emit (the allowed count is not known without a
// synchronisation) and never the shortlist; a filter that leaves fewer than k allowed rows in the 8192-row sample
// yields no bound, and the candidate buffer may overflow: status ResourceExhausted, out_count 0 for those queries.
int bf_search_device(const BfIndexDev &ix, BfWorkspace &w, const float *d_queries, uint32_t nq,
                     uint32_t q_stride, uint32_t k, bool shortlist, double tail, const BfFilter &flt,
                     uint32_t *d_out_idx, float *d_out_dist, uint32_t *d_out_count, hipStream_t stream, hipEvent_t ev0,
                     hipEvent_t ev1);
// OK, or the status the last enqueued search left in the workspace counters (synchronises).
int bf_last_status(const BfWorkspace &w, hipStream_t stream);

// half::bf16::from_f32 over n values (scann_hip_bf16_quantize), host in / host out.
int bf16_quantize_host(const float *values, uint64_t n, uint16_t *out_bits, hipStream_t stream);

// Dense [nq][n] distance matrix to host memory.
int bf_distances_host(const BfIndexDev &ix, BfWorkspace &w, const float *queries, uint32_t nq,
                      uint32_t q_stride, float *out, hipStream_t stream);

// BruteForceSearcher::search_radius for one query: all rows with distance <= radius, sorted by
// (distance, index).  At most `capacity` rows are written; *out_count = number found.
int bf_search_radius_host(const BfIndexDev &ix, BfWorkspace &w, const float *query, uint32_t q_stride,
                          float radius, const BfFilter &flt, uint32_t *out_idx, float *out_dist, uint64_t capacity,
                          uint64_t *out_count, hipStream_t stream);

// Nearest of k centres for every row of the index (sequential-scalar SquaredL2, lowest index on
// ties): TreePartitioner::partition(x, 1) / KMeans::assign_clusters.
int bf_assign_nearest_host(const BfIndexDev &ix, const float *centers, uint32_t k, uint32_t *out_idx,
                           float *out_dist, hipStream_t stream);
// The same with centres, assignments and (optional) distances on the device; enqueue only.  Reads ix.rows, n, dim, stride.
int bf_assign_nearest_device(const BfIndexDev &ix, const float *d_centers, uint32_t k, uint32_t *d_out_idx,
                             float *d_out_dist, hipStream_t stream);

// K-means over the rows of the index (optionally the column window [col_offset, col_offset +
// sub_dim)): k-means++ seeding (trees/kmeans.rs:295-349, splitmix64 stream) and the Lloyd loop of
// KMeans::fit_single (:210-263) from caller-supplied centres [k][sub_dim] (updated in place).
int bf_kmeans_init_pp_host(const BfIndexDev &ix, uint32_t col_offset, uint32_t sub_dim, uint32_t k,
                           uint64_t seed, uint32_t simd_threshold, float *centers_out, hipStream_t stream);
int bf_kmeans_lloyd_host(const BfIndexDev &ix, uint32_t col_offset, uint32_t sub_dim, float *centers,
                         uint32_t k, uint32_t max_iterations, double convergence_threshold,
                         uint32_t simd_threshold, uint32_t *out_assign, uint32_t *out_sizes,
                         double *out_inertia, uint32_t *out_iterations, int *out_converged,
                         hipStream_t stream);

// ---- the same two with centres and assignment resident on the device (the host forms above wrap them; build.hip) ----
// Grow-only scratch of the cores: one object serves any number of calls, so a loop over subspaces allocates once.
struct KmScratch {
    DevBuf dmin, dpart, dtotal, dpicks, ddist, dkeys, dsorted, dtmp, doff, dgrows;
};
// d_centers_out [k][sub_dim]; complete on return
int bf_kmeans_init_pp_device(const BfIndexDev &ix, uint32_t col_offset, uint32_t sub_dim, uint32_t k, uint64_t seed,
                             uint32_t simd_threshold, float *d_centers_out, KmScratch &sc, hipStream_t stream);
// d_centers [k][sub_dim] and d_assign [n] updated in place.  final_assign false: no assignment of the final centres
// (kmeans.rs:248-255) -- d_assign is then the one the last update was made from and *out_inertia the last one computed.
int bf_kmeans_lloyd_device(const BfIndexDev &ix, uint32_t col_offset, uint32_t sub_dim, float *d_centers, uint32_t k,
                           uint32_t max_iterations, double convergence_threshold, uint32_t simd_threshold,
                           uint32_t *d_assign, bool final_assign, KmScratch &sc, double *out_inertia,
                           uint32_t *out_iterations, int *out_converged, hipStream_t stream);
// sc.dsorted [n]: the keys (cluster << 32 | index) of an assignment in ascending order, i.e. every cluster's members in
// ascending datapoint index; sc.doff [k + 1]: where each cluster starts.  Enqueue only.
int bf_kmeans_csr_device(const uint32_t *d_assign, uint64_t n, uint32_t k, KmScratch &sc, hipStream_t stream);

// ---- the reductions and the centre update of the cores, launched once for a batch of lists / column windows ----
// (the kernels are the primitives' own, so a batched codebook takes the same sums in the same trees)
uint64_t km_seed_stream_next(uint64_t &state);   // splitmix64, the seeding's random stream
bool km_tree_sum_is_exact(double total, uint32_t min_pos_bits);
// list y of `lists`: d_vals + y * n -> d_partials + y * ceil(n / 256), smallest positive term into
// d_min_pos[y * min_pos_stride] (atomicMin; null: none); skipped where d_skip[y * skip_stride] != 0
int km_sums_batched(const float *d_vals, uint64_t n, uint32_t lists, double *d_partials, uint32_t *d_min_pos,
                    uint32_t min_pos_stride, const uint32_t *d_skip, uint32_t skip_stride, hipStream_t stream);
// list y: partials -> d_totals[y * total_stride]; with d_picks, the k-means++ pick over d_min_d + y * n with the draw
// (d_u_tab[y], d_fallback_tab[y]) into d_picks[y * pick_stride]
int km_totals_batched(const double *d_partials, uint64_t n, uint32_t lists, const float *d_min_d, const double *d_u_tab,
                      const uint32_t *d_fallback_tab, double *d_totals, uint32_t total_stride, uint32_t *d_picks,
                      uint32_t pick_stride, hipStream_t stream);
// list y where d_need[y * need_stride] != 0: the sum in datapoint order into d_totals[y * total_stride]
int km_sequential_sums_batched(const float *d_vals, uint64_t n, uint32_t lists, double *d_totals, uint32_t total_stride,
                               const uint32_t *d_need, uint32_t need_stride, hipStream_t stream);
// window y of `windows` (columns y * window0.dim .. of window0's rows): cluster c's members are the positions
// d_offsets[y * k_stride + c] .. [+ 1] of d_grows ([position][window0.dim], member order); centres into
// d_centers[(y * k_stride + c) * dim]; skipped where d_skip[y * skip_stride] != 0
int km_update_batched(const BfIndexDev &window0, const float *d_grows, const uint32_t *d_offsets, float *d_centers,
                      uint32_t k, uint32_t k_stride, uint32_t windows, const uint32_t *d_skip, uint32_t skip_stride,
                      hipStream_t stream);

}  // namespace scann

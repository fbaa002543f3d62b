/*
 * scann_hip.h -- C ABI of libscann_hip.so: the MI355X (gfx950) implementation
 * of the sunbains/scann-rust Tree-X-Hybrid / brute-force hot path.
 *
 * The reference crate has no FFI of its own (pure Rust); the
 * drop-in boundary is its Rust API.  Each entry point below names the Rust
 * item(s) whose body it replaces (paths relative to /root/reference/src); the
 * Rust-side `extern "C"` block a maintainer would add is in INTEGRATION.md.
 *
 * Conventions
 *  - plain pointers and sizes only; no C++/torch types.
 *  - every function returns a scann_hip_status (== ErrorCode discriminant in
 *    declaration order, error.rs:10-45); scann_hip_last_error() returns the
 *    thread-local message of the last failure on the calling thread.
 *  - *_create copies host arrays to the device; the caller keeps ownership of
 *    its host memory and may free it on return.  Handles own device memory until
 *    scann_hip_index_destroy.
 *  - host entry points are synchronous (outputs filled on return).  The *_device
 *    variants take device pointers + a hipStream_t (passed as void*), enqueue
 *    only, and never synchronise: inputs already resident in HBM.
 *  - result rows are ascending by distance; rows shorter than k are reported via
 *    out_count (the reference returns shorter Vecs: brute_force/searcher.rs:91,
 *    tree_x_hybrid/mod.rs:360-363).  Unused slots: idx 0xFFFFFFFF, dist +inf.
 *  - any thread may call search functions concurrently on one handle (Searcher:
 *    Send + Sync, searcher.rs:148): host-side searches draw a stream + workspace from a small
 *    per-handle pool (SCANN_HIP_SEARCH_SLOTS, default 4) and run side by side.  create/destroy need
 *    external synchronisation.
 *  - device entry points and streams: every *_device search call works in a per-handle workspace that is
 *    bound to the CALLER'S STREAM (SCANN_HIP_DEVICE_SLOTS workspaces per handle, default 2, at most 4; the
 *    first one is the handle's primary workspace).  Calls enqueued on the same stream reuse its workspace in
 *    stream order; calls on different streams use different workspaces and may overlap on the device -- a
 *    caller alternating two streams runs batch i+1's scan under batch i's re-rank.  With more streams than
 *    workspaces the least recently used workspace changes hands, and the library orders the new call behind
 *    the old stream's last call with an event (correct, no overlap for that pair).
 *    scann_hip_index_last_device_status(index, stream) reports the calls enqueued on that stream.
 */
#ifndef SCANN_HIP_H
#define SCANN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* error.rs:10-45 (ErrorCode, declaration order) */
typedef enum {
    SCANN_HIP_OK = 0,
    SCANN_HIP_CANCELLED = 1,
    SCANN_HIP_UNKNOWN = 2,
    SCANN_HIP_INVALID_ARGUMENT = 3,
    SCANN_HIP_DEADLINE_EXCEEDED = 4,
    SCANN_HIP_NOT_FOUND = 5,
    SCANN_HIP_ALREADY_EXISTS = 6,
    SCANN_HIP_PERMISSION_DENIED = 7,
    SCANN_HIP_RESOURCE_EXHAUSTED = 8,
    SCANN_HIP_FAILED_PRECONDITION = 9,
    SCANN_HIP_ABORTED = 10,
    SCANN_HIP_OUT_OF_RANGE = 11,
    SCANN_HIP_UNIMPLEMENTED = 12,
    SCANN_HIP_INTERNAL = 13,
    SCANN_HIP_UNAVAILABLE = 14,
    SCANN_HIP_DATA_LOSS = 15,
    SCANN_HIP_UNAUTHENTICATED = 16
} scann_hip_status;

/* distance_measures/mod.rs:32-66: the measures the hot path dispatches on
 * (brute_force/searcher.rs:119-138). */
typedef enum {
    SCANN_HIP_SQUARED_L2 = 0,
    SCANN_HIP_L2 = 1,
    SCANN_HIP_DOT_PRODUCT = 2, /* distance = -dot (simd/x86.rs:247-250) */
    /* The two measures below go through DistanceMeasure::distance one pair at a time in the reference
     * (brute_force/searcher.rs:131-137, scann.rs:238-246, utils/reordering.rs:35-44).  They are valid for
     * brute-force handles and as the distance_measure of Scann-facade indexes (SearchMode::Partitioned,
     * exact reordering); TreeXHybridSearcher / AsymmetricHasher re-rank by squared L2 regardless. */
    SCANN_HIP_L1 = 3,          /* l1_distance_avx2, simd/x86.rs:103-132 */
    SCANN_HIP_COSINE = 4       /* 1 - cosine similarity, one_to_one.rs:559-612; its horizontal sums are the
                                * third-party wide::f32x8::reduce_add (wide 0.7, non-AVX build): restated,
                                * parity unpinned by the reference */
} scann_hip_measure;

typedef struct scann_hip_ctx scann_hip_ctx;     /* one device + stream/workspace pool */
typedef struct scann_hip_index scann_hip_index; /* one searcher */

/* ---- context ------------------------------------------------------------ */
int scann_hip_init(int device_id, scann_hip_ctx **out_ctx);
void scann_hip_shutdown(scann_hip_ctx *ctx);
const char *scann_hip_last_error(void);
const char *scann_hip_version(void);
/* ABI guard for bindings written by hand (Rust #[repr(C)], ctypes): fills out[0..n) with
 * { sizeof(scann_hip_txh_desc), offsetof(.., distance_measure), sizeof(scann_hip_search_opts),
 *   offsetof(.., bf_exact), sizeof(scann_hip_file_info), offsetof(.., has_data),
 *   sizeof(scann_hip_build_config), offsetof(.., distance_measure), sizeof(scann_hip_build_report),
 *   offsetof(.., stage_ms) } and returns the number of values defined (10; the first 6 are those of earlier
 * versions, in place).  A binding asserts these against its own layout once at start-up. */
uint32_t scann_hip_abi_layout(uint32_t *out, uint32_t n);
/* data_format/dataset.rs:90-96 (DenseDataset::compute_stride for f32) */
uint32_t scann_hip_compute_stride(uint32_t dim);

/* ---- brute force --------------------------------------------------------- */
/* Replaces BruteForceSearcher::new / with_shared_dataset
 * (brute_force/searcher.rs:34-54).  data: n rows of `stride` floats, the
 * DenseDataset::raw_data() buffer (data_format/dataset.rs:176-179, 228-230).
 * n == 0 is legal (searches return empty rows, searcher.rs:78-80). */
int scann_hip_bf_create(scann_hip_ctx *ctx, const float *data, uint64_t n, uint32_t dim,
                        uint32_t stride, int measure, scann_hip_index **out_index);

/* Brute force over rows the caller already stores quantized: ScalarQuantizedBruteForceSearcher
 * (brute_force/scalar_quantized.rs:168-296) and its siblings over bf16 / FP8 rows.  rows: n rows of
 * `stride` ELEMENTS of row_format:
 *   SCANN_HIP_ROWS_BF16      half::bf16 bits (u16); distances = one_to_many_bf16_float_{dot_product,squared_l2}
 *                            (distance_measures/one_to_many_asymmetric.rs:267-314): to_f32 (exact), then ONE
 *                            sequential f32 sum per row, no FMA (dot: sum += q*x; SquaredL2: d = q - x, sum += d*d).
 *                            BFloat16Dataset::{dot_product, squared_l2_distance} use other SIMD code and are not
 *                            what this reproduces.
 *   SCANN_HIP_ROWS_FP8_E4M3  the reference's Fp8Value E4M3 codes (quantization/fp8.rs, u8); distances =
 *                            one_to_many_fp8_float_* (:327-377), the same sequential loops over to_f32_e4m3 as
 *                            scann_hip_fp8_distances.  Not OCP e4m3fn: exponent field 0 with mantissa m != 0
 *                            decodes to 2^-8 * (1 + m/8), 0x7F / 0xFF to +-480.
 *   SCANN_HIP_ROWS_INT8      i8, value = (float)i8 * inv_multiplier (rounded); distances = one_to_many_int8_float_*
 *                            in the AVX2 form the reference runs on x86 hosts (:78-142, :208-257): 8 lane chains
 *                            of fma over full 8-element chunks, horizontal sum (lo + hi, then (t0+t1)+(t2+t3)), an
 *                            unfused scalar tail -- the f32 brute-force arithmetic on the dequantized rows.
 *                            inv_multiplier is ScalarQuantizedBruteForceSearcher's quantizer.scale()
 *                            (scalar_quantized.rs:198-225), which reads the quantizer's offset-binary bytes
 *                            (scalar.rs:162-172) as SIGNED and ignores min_value: such bytes passed here give
 *                            exactly that reading.  inv_multiplier is ignored for the other formats.
 * Dot products are negated; L2 = sqrtf(SquaredL2), applied before selection (scalar_quantized.rs:217-224), so
 * ties it creates are broken by TopK's (distance, index) rule.  L1 / Cosine -> Unimplemented.
 * Searches: k = min(k, n), TopK over all rows in index order, drained sorted; n == 0 gives empty rows; radius
 * search = every d <= radius, stable-sorted by distance.  The handle works with scann_hip_search_batched(_params),
 * scann_hip_index_reserve, scann_hip_search_batched_device / scann_hip_index_last_device_status,
 * scann_hip_bf_search_radius, scann_hip_bf_distances, the introspection and timing calls, from concurrent
 * threads as any brute-force handle.  Entry points that read rows as f32 (scann_hip_kmeans_*,
 * scann_hip_bf_assign_nearest, Tree-X-Hybrid calls) return InvalidArgument.  opts.allow_bitmap is honoured with
 * the brute-force contract stated at scann_hip_search_opts (distances stay those of the row format).  opts.bf_exact has the f32 contract: large batches on large indexes (the dims and
 * sizes of the f32 shortlist, stride % 8 == 0) take the bf16-shortlist path, whose row operand is the stored
 * value itself (exact in bf16 for all three formats: only the query is split); a query it cannot prove sets
 * status Aborted, which the host entry point repeats by itself and *_device callers repeat with bf_exact = 1.
 * The device holds the rows as given (2 or 1 byte per element), no f32 or bf16 copy, plus one f32 squared
 * norm per row when the index qualifies for the shortlist.
 * Errors: stride < dim, dim == 0 with n > 0, unknown row_format, rows == NULL with n > 0, non-finite
 * inv_multiplier for INT8 -> InvalidArgument; n >= 2^32 - 1 -> OutOfRange; measure L1 / Cosine -> Unimplemented. */
#define SCANN_HIP_ROWS_BF16 1
#define SCANN_HIP_ROWS_FP8_E4M3 2
#define SCANN_HIP_ROWS_INT8 3
int scann_hip_bf_create_quantized(scann_hip_ctx *ctx, const void *rows, uint64_t n, uint32_t dim,
                                  uint32_t stride, int row_format, float inv_multiplier, int measure,
                                  scann_hip_index **out_index);
/* f32_slice_to_bf16 / half::bf16::from_f32 (quantization/bfloat16.rs:13-30) on the device: round to nearest
 * even, +-inf stay +-inf, finite values past the largest bf16 round to inf, a NaN stays a NaN
 * ((bits >> 16) | 0x40). */
int scann_hip_bf16_quantize(scann_hip_ctx *ctx, const float *values, uint64_t n, uint16_t *out_bits);

/* ---- scalar quantizer: quantized handles from f32 handles, on the device ------------------------------------
 * QuantizationStats::from_dataset (quantization/mod.rs:75-110), ScalarQuantizer::calibrate / quantize_value /
 * dequantize_value (quantization/scalar.rs:103-172) and ScalarQuantizedBruteForceSearcher::new(&dataset, config)
 * (brute_force/scalar_quantized.rs).  All f32 arithmetic is unfused.
 *
 * Modes (the reference's ScalarQuantizerConfig, and one of this library's own):
 *   SCANN_HIP_SQ_STDDEV     the default config; a = num_std_devs (3.0): r = a * std_dev,
 *                           min = max(mean - r, stats.min), max = min(mean + r, stats.max)
 *   SCANN_HIP_SQ_SYMMETRIC  symmetric(): abs_max = max(|stats.min|, |stats.max|), range [-abs_max, abs_max]
 *   SCANN_HIP_SQ_RANGE      with_range(a, b): min = a, max = b
 *   SCANN_HIP_SQ_SIGNED     this library's: m = max|x|, s = (float)((double)m / 127.0) (1 when m == 0),
 *                           code = clip(rintf(x / s), -127, 127) with a correctly rounded division; params4 =
 *                           {-m, m, s, 1 / s}, zero_point 0; bits must be 8; non-finite values are InvalidArgument.
 * For the three reference modes, with levels = (1 << bits) - 1, bits 4 or 8, and range = max - min:
 *   range > 1e-10: scale = range / levels, inv_scale = levels / range, zero_point = roundf(-min * inv_scale) as i32;
 *   otherwise scale = inv_scale = 1, zero_point = 0.  min > max or a NaN bound -> InvalidArgument.
 *   code = clamp(roundf((clamp(v, min, max) - min) * inv_scale) as i32, 0, levels) stored as i8 with wrap (128..255
 *   become -128..-1, the reference's offset-binary bytes); a NaN value gives code 0.
 *   dequantize = (float)(uint8_t)code * scale + min.  (SCANN_HIP_SQ_SIGNED: (float)code * scale.)
 * WHAT THE SEARCHERS READ: a quantized handle reads int8 bytes as SIGNED, value = i8 * inv_multiplier, and knows no
 * min_value -- exactly ScalarQuantizedBruteForceSearcher (scalar_quantized.rs:198-225).  Rows quantized in one of
 * the three reference modes therefore reproduce the reference INCLUDING that reading of its offset-binary bytes;
 * SCANN_HIP_SQ_SIGNED is the mode whose codes mean what the searcher reads.
 *
 * params4 = {min, max, scale, inv_scale}; stats4 = {min, max, mean, std_dev}. */
#define SCANN_HIP_SQ_STDDEV 0
#define SCANN_HIP_SQ_SYMMETRIC 1
#define SCANN_HIP_SQ_RANGE 2
#define SCANN_HIP_SQ_SIGNED 3
/* Stats over the n * dim logical values of the f32 rows resident in `index` (stride padding is never read): min and
 * max fold with fminf / fmaxf from f32::MAX / f32::MIN (a NaN operand is ignored; which of -0.0 and +0.0 wins a tie is
 * the platform's choice, as in the reference); sum and sum of squares in f64 in a FIXED order that depends on
 * (n, dim) only -- the same run to run, on any grid, at any stride; mean = (sum / count) as f32,
 * variance = ((sum_sq - sum * sum / count) / (count - 1)) as f32 (0 when count == 1), std_dev = sqrtf(variance).
 * Sources and errors: those of scann_hip_index_quantize_rows. */
int scann_hip_index_quantization_stats(scann_hip_index *index, float *out_stats4);
/* Host arithmetic, no GPU and no context needed.  Nothing is written on an error.  a, b: see the modes. */
int scann_hip_scalar_quantizer_calibrate(const float *stats4, uint32_t bits, int mode, float a, float b,
                                         float *out_params4, int32_t *out_zero_point);
int scann_hip_scalar_quantize(const float *values, uint64_t n, uint32_t bits, int mode, const float *params4,
                              int8_t *out);
int scann_hip_scalar_dequantize(const int8_t *codes, uint64_t n, int mode, const float *params4, float *out);
/* The quantize pass on device memory: n rows of dim f32 values at `stride` -> n rows of out_stride codes; columns
 * dim .. out_stride - 1 are written as 0; nothing past n * out_stride bytes is written.  One kernel is enqueued on
 * hip_stream, nothing is synchronised.  SCANN_HIP_SQ_SIGNED here maps NaN to 0 and +-inf to +-127 (a stream-ordered
 * call cannot refuse them).  out_stride < dim, stride < dim, dim == 0, a bad mode / bits / range -> InvalidArgument. */
int scann_hip_scalar_quantize_device(scann_hip_ctx *ctx, const float *d_rows, uint64_t n, uint32_t dim, uint32_t stride,
                                     uint32_t bits, int mode, const float *params4, int8_t *d_out, uint32_t out_stride,
                                     void *hip_stream);
/* A NEW handle over the rows of `src` stored as row_format (SCANN_HIP_ROWS_*), made on the device from the f32 rows
 * resident in src: no row visits the host.  src is left untouched and stays usable; destroy it to reclaim its memory.
 * INT8: stats, calibrate(bits, mode, a, b), quantize; the handle's inv_multiplier is the calibrated scale.  BF16 /
 * FP8_E4M3: the arithmetic of scann_hip_bf16_quantize / scann_hip_fp8_quantize(scale 1); bits, mode, a, b are
 * ignored and out_params4 / out_zero_point are written as {0, 0, 1, 1} / 0.  Output rows keep src's stride in
 * ELEMENTS, pad columns 0.  out_params4 / out_zero_point may be NULL.
 * A brute-force src gives what scann_hip_bf_create_quantized builds from the same bytes, measure and inv_multiplier;
 * a Tree-X-Hybrid / AsymmetricHasher src with f32 rows gives what scann_hip_txh_create_quantized builds from the same
 * descriptor and bytes (its small arrays -- centres, CSR, codes, codebook -- are read back and uploaded again; the
 * rows are not).  Every search entry point, every refusal and scann_hip_index_device_bytes are those of that twin.
 * Errors (*out_index is not written): n == 0 ("Cannot quantize empty dataset", scalar.rs:199-201), src already
 * quantized, unknown row_format, a bad mode / bits / range, non-finite rows in SCANN_HIP_SQ_SIGNED -> InvalidArgument;
 * a tree handle without rows -> FailedPrecondition; L1 / Cosine, leaf-sharded, SearchMode::Partitioned and
 * CSR-ordered rows with partitions -> Unimplemented. */
int scann_hip_index_quantize_rows(scann_hip_index *src, int row_format, uint32_t bits, int mode, float a, float b,
                                  scann_hip_index **out_index, float *out_params4, int32_t *out_zero_point);

/* ---- Tree-X-Hybrid / AsymmetricHasher ------------------------------------ */
/* The trained index TreeXHybridSearcher::build (tree_x_hybrid/mod.rs:131-209)
 * or AsymmetricHasher::build (hashes/hasher.rs:109-134) produced, flattened:
 *   centers       [num_partitions][dim]  TreePartitioner.centers (tree_partitioner.rs:29)
 *   leaf_offsets  [num_partitions+1]     CSR over PartitionData.indices (mod.rs:81-90)
 *   leaf_ids      [n_local]              datapoint index of CSR row i
 *   codebook      [S][K][dsub]           Codebook.subspaces[s].centroids (codebook.rs:59-67)
 *   codes         CSR row order; unpacked [n_local][S] u8 (PartitionData.encoded) or
 *                 packed 4-bit [n_local][ceil(S/2)] (PackedCodes4Bit, lut16.rs:43-61)
 *   data          [n_rows][stride] original rows indexed by DATAPOINT index (re-rank,
 *                 mod.rs:342-364); may be NULL (AsymmetricHasher::build_no_store,
 *                 hasher.rs:137-159): exact re-ordering then fails FailedPrecondition.
 * num_partitions == 0 selects AsymmetricHasher mode: one implicit leaf holding all
 * n points in datapoint order (leaf_offsets / leaf_ids / centers ignored).
 *
 * Multi-GPU leaf sharding (one process per GPU): each rank passes only the leaves
 * it owns (unowned leaves have zero local length) plus leaf_sizes_global, so every
 * rank derives identical merge keys; data then holds only the local rows in CSR row
 * order (data_is_csr_order = 1).  leaf_sizes_global == NULL means unsharded.
 *
 * Scann facade modes (scann.rs:181-294) are configurations of the same index:
 *   SearchMode::TreeAH       use_residuals = 0, codebook trained on the raw rows, searched with
 *                            pre_reorder_k = k (and exact_reorder = 0, or 1 for the exact
 *                            reordering of the k-truncated list, scann.rs:199-209);
 *   SearchMode::Hashed       num_partitions = 0, same options;
 *   SearchMode::Partitioned  codebook == NULL && codes == NULL && num_subspaces == 0: every row
 *                            of the selected leaves is scored exactly with distance_measure
 *                            (search_partitioned, scann.rs:213-252); needs data, unsharded.
 * distance_measure (SCANN_HIP_SQUARED_L2 = 0 / L2 / DOT_PRODUCT / L1 / COSINE) is the measure of the exact
 * re-ordering (ReorderingHelper, utils/reordering.rs:23-54) and of the Partitioned scan;
 * TreeXHybridSearcher and AsymmetricHasher always re-rank by squared L2 (mod.rs:350-358). */
typedef struct {
    const float *data;
    uint64_t n_rows;
    uint32_t dim;
    uint32_t stride;
    int32_t data_is_csr_order;
    const float *centers;
    uint32_t num_partitions;
    const uint32_t *leaf_offsets;
    const uint32_t *leaf_ids;
    const uint32_t *leaf_sizes_global;
    uint64_t n_local;
    const float *codebook;
    uint32_t num_subspaces;      /* S */
    uint32_t num_codes;          /* K <= 16: LUT16 (4-bit codes, S in {8,16,24,32,48,64});
                                  * 16 < K <= 256: byte codes (S in {4,8,16}) */
    uint32_t dims_per_subspace;  /* dsub; S * dsub must equal dim (codebook.rs:154-159) */
    const uint8_t *codes;
    int32_t codes_packed4;
    int32_t use_residuals;            /* TreeXHybridConfig.use_residuals (mod.rs:31) */
    uint32_t partitions_to_search;    /* TreeXHybridConfig.partitions_to_search (mod.rs:27) */
    float pre_reorder_multiplier;     /* TreeXHybridConfig.pre_reorder_multiplier (mod.rs:33) */
    int32_t distance_measure;         /* ScannConfig.distance_measure (config.rs:32-36); 0 = SquaredL2 */
} scann_hip_txh_desc;

/* Replaces the search side of TreeXHybridSearcher::build / AsymmetricHasher::build.
 * Errors: n_local == 0 -> InvalidArgument (mod.rs:132-134, hasher.rs:110-112);
 * dim % S != 0 -> InvalidArgument (codebook.rs:154-159).
 * The arrays' CONTENTS are validated too, so that no search can read out of bounds: leaf_offsets
 * monotone and spanning [0, n_local]; every leaf_ids[i] < n_rows when data is indexed by datapoint
 * (data != NULL, data_is_csr_order == 0); n_rows >= n_local when rows are read in CSR order
 * (AsymmetricHasher mode with data); leaf_sizes_global[l] >= the local length of leaf l; every code
 * < num_codes (packed or not).  Violations -> InvalidArgument here, DataLoss from
 * scann_hip_index_load_file (a file whose sizes are consistent but whose contents are not). */
int scann_hip_txh_create(scann_hip_ctx *ctx, const scann_hip_txh_desc *desc,
                         scann_hip_index **out_index);

/* A Tree-X-Hybrid / AsymmetricHasher index whose re-rank rows the caller stores quantized: the reordering stage of
 * ScalarQuantizedBruteForceSearcher and its bf16 / FP8 siblings behind the tree or the hasher.  desc->data must be
 * NULL; `rows` holds desc->n_rows rows of desc->stride ELEMENTS of row_format (SCANN_HIP_ROWS_BF16, _FP8_E4M3 or
 * _INT8), indexed as desc->data would be (by datapoint index; AsymmetricHasher mode: datapoint = CSR order); elements
 * past dim are never read.  inv_multiplier has the meaning documented at scann_hip_bf_create_quantized.
 * Every stage before the re-rank is that of scann_hip_txh_create.  The merged candidates of a query then each get the
 * distance a scann_hip_bf_create_quantized handle gives the same query and stored row under the same format,
 * distance_measure and inv_multiplier, bit for bit (bf16 / FP8: one sequential f32 sum, no FMA; int8: 8 FMA lane
 * chains, the fixed horizontal sum, an unfused tail; DotProduct negated, L2 = sqrtf of the squared sum), are stably
 * sorted by it in merged order and truncated to k.  NaN and infinite distances order as on an f32 handle;
 * exact_reorder = 0 returns approximate distances and reads no rows.
 * The device holds the rows as given: no f32 copy and no 8-bit shadow store of the re-rank filter.  Every batch size
 * takes the batched pipeline (the few-query pipelines re-rank from f32 rows).
 * Works unchanged: scann_hip_search_batched(_params), scann_hip_index_reserve, scann_hip_search_batched_device,
 * scann_hip_index_last_device_status, the crowded searches, allow-bitmaps per call and per query, the stage outputs,
 * timing, scann_hip_index_write_file / scann_hip_index_load_file (sections "rows_q" and "rows_q_meta" = {format,
 * inv_multiplier bits} in place of "data"; scann_hip_file_info.has_data is 0).
 * Unimplemented on such a handle, each message naming quantized rows: scann_hip_search_mmr*, scann_hip_mutable_create /
 * _rebase onto it, scann_hip_txh_search_local_device / _sharded_device, scann_hip_index_debug_rerank_brackets.
 * Errors: all of scann_hip_txh_create's; desc->data != NULL, rows == NULL, unknown row_format, non-finite
 * inv_multiplier for INT8 -> InvalidArgument; distance_measure L1 / Cosine, leaf_sizes_global != NULL,
 * data_is_csr_order with partitions, SearchMode::Partitioned (no codes) -> Unimplemented. */
int scann_hip_txh_create_quantized(scann_hip_ctx *ctx, const scann_hip_txh_desc *desc, const void *rows,
                                   int row_format, float inv_multiplier, scann_hip_index **out_index);

/* ---- projections (src/projection/: PcaProjection, RandomOrthogonalProjection, GaussianRandomProjection,
 * OpqProjection, TruncateProjection) ------------------------------------------------------------------------------
 * Every dense projection of the reference is one loop (pca.rs:156-180, random.rs:82-92, 157-167, opq.rs:179-194):
 *     out[j] = 0.0f;  for i in 0..in_dim (ascending):  out[j] += (in[i] - mean[i]) * M[(i, j)]
 * an f32 sum, a multiply and then an add per step (no FMA), the subtraction PCA's alone.  The device computes exactly
 * that chain for every output: a projected row equals the reference's bit for bit, subnormals kept,
 * NaN and infinities propagated as the chain propagates them.  TRUNCATE (and an untrained PcaProjection) copies the
 * window in[start .. start + out_dim).
 * `matrix` is [out_dim][in_dim]: column j of the reference's column-major DMatrix is row j here.  `mean` is [in_dim].
 * The object copies its arrays at create and is immutable afterwards; project calls on one object may run
 * concurrently.  The trained matrix is an input (the reference's eigen-solver and RNG are not reproducible here:
 * SURVEY F2, F4, F10), as centres and codebooks are; scann_hip_pca_train ("PCA training on the device", below) trains
 * one by the project's own rule. */
typedef struct scann_hip_projection scann_hip_projection;
#define SCANN_HIP_PROJ_MATRIX   1   /* random orthogonal / gaussian / OPQ rotation: no mean */
#define SCANN_HIP_PROJ_PCA      2   /* matrix + mean */
#define SCANN_HIP_PROJ_TRUNCATE 3   /* out = in[start .. start + out_dim) */
/* Errors (InvalidArgument): unknown kind; in_dim == 0 or out_dim == 0; matrix == NULL (MATRIX, PCA); mean == NULL
 * (PCA); TRUNCATE with start + out_dim > in_dim.  `start` is read for TRUNCATE only, matrix / mean are not. */
int scann_hip_projection_create(scann_hip_ctx *ctx, int kind, uint32_t in_dim, uint32_t out_dim, const float *matrix,
                                const float *mean, uint32_t start, scann_hip_projection **out_projection);
void scann_hip_projection_destroy(scann_hip_projection *projection);
/* out4 = kind, in_dim, out_dim, start */
int scann_hip_projection_info(const scann_hip_projection *projection, uint32_t *out4);
/* n rows of row_dim floats, row_stride apart -> n rows of out_dim floats, out_stride apart; host pointers.  Elements of
 * `out` between out_dim and out_stride are not written.  Errors (InvalidArgument): row_dim != in_dim, row_stride <
 * row_dim, out_stride < out_dim, NULL rows / out with n > 0. */
int scann_hip_project(const scann_hip_projection *projection, const float *rows, uint64_t n, uint32_t row_stride,
                      uint32_t row_dim, float *out, uint32_t out_stride);
/* The same on device pointers: one kernel enqueued on hip_stream, no synchronisation, no allocation.  The rows are
 * in_dim wide.  Errors: as above. */
int scann_hip_project_device(const scann_hip_projection *projection, const float *d_rows, uint64_t n, uint32_t row_stride,
                             float *d_out, uint32_t out_stride, void *hip_stream);

/* A Tree-X-Hybrid / AsymmetricHasher index that partitions, hashes and scans in a PROJECTED space and re-ranks against
 * the original rows.  desc->data must be NULL.  `desc` describes the index in the projected space: desc->dim ==
 * projection.out_dim, centres [L][out_dim], codebook S * dsub == out_dim, codes as always (desc->stride is not read).
 * `rows` holds n_rows (desc->n_rows is not read) original f32 rows of row_dim == projection.in_dim floats, row_stride
 * apart, indexed by datapoint (AsymmetricHasher mode: datapoint = CSR order) and validated against leaf_ids as desc->data
 * is; NULL = no exact re-ordering (build_no_store).  The handle
 * copies the projection to the device: the caller may destroy `projection` afterwards.
 * A search takes queries of row_dim floats (the q_dim check compares against row_dim, and
 * scann_hip_index_dimensionality reports it):
 *   1. qp = project(q) on the device, at the head of the call's stream, into a workspace buffer [nq][out_dim] (reserved
 *      with the others by scann_hip_index_reserve; one per stream on the _device entry points);
 *   2. every stage up to the merged candidate list is that of a scann_hip_txh_create handle of dim out_dim given qp,
 *      bit for bit;
 *   3. the re-rank scores the original q against the original rows with desc->distance_measure: exact distance, stable
 *      sort in merged order, truncate to k -- today's rule;
 *   4. exact_reorder = 0 returns the approximate distances of step 2 and reads no rows.
 * Every batch size takes the batched pipeline (the few-query pipelines re-rank inside kernels that read one query
 * space); the handle builds no 8-bit shadow store, so the re-rank row filter is off (it changes no result).
 * Works unchanged: scann_hip_search_batched(_params), scann_hip_index_reserve, scann_hip_search_batched_device,
 * scann_hip_index_last_device_status, allow-bitmaps per call and per query, token-map searches, the crowded searches,
 * the stage outputs, timing, scann_hip_index_write_file / scann_hip_index_load_file (the header's dim / stride keep
 * describing the index space; new sections "proj_meta" = u32 {kind, in_dim, out_dim, start, row_stride}, "proj_matrix" =
 * f32 [out_dim][in_dim], "proj_mean" = f32 [in_dim] (PCA only); "data" holds the original rows at row_stride; a
 * proj_meta that disagrees with the header or the section sizes -> DataLoss).  Timing: scann_hip_index_last_kernel_ms
 * brackets the dominant kernel, the scan, as on every handle; the query projection is outside that bracket, like the
 * partition, table, select and re-rank kernels.  The stage functions scann_hip_txh_partition, scann_hip_lut_from_query and
 * scann_hip_adc_distances stay in INDEX space on such a handle: they take queries of out_dim floats.
 * Unimplemented, each message naming projection: scann_hip_search_mmr*, scann_hip_mutable_create / _rebase / fold onto
 * it, scann_hip_txh_search_local_device / _sharded_device, scann_hip_index_quantize_rows and
 * scann_hip_index_quantization_stats from it, scann_hip_index_debug_rerank_brackets; at create: leaf_sizes_global, data_is_csr_order with partitions, SearchMode::Partitioned (no codes).
 * InvalidArgument: a NULL projection, desc->data != NULL, desc->dim != out_dim, row_dim != in_dim, row_stride <
 * row_dim; and all of scann_hip_txh_create's errors. */
int scann_hip_txh_create_projected(scann_hip_ctx *ctx, const scann_hip_txh_desc *desc,
                                   const scann_hip_projection *projection, const float *rows, uint64_t n_rows,
                                   uint32_t row_dim, uint32_t row_stride, scann_hip_index **out_index);
/* out4 = kind, in_dim, out_dim, start of the projection a handle searches through; kind 0 (and zeros) on every other
 * handle. */
int scann_hip_index_projection_info(const scann_hip_index *index, uint32_t *out4);

typedef struct {
    /* 0 = the index default.  SearchParameters.num_leaves_to_search is ignored by
     * the reference searcher; this knob exists for sweeps. */
    uint32_t partitions_to_search;
    /* candidates kept by approximate distance before re-ranking.
     * 0 = (k as f32 * pre_reorder_multiplier) as usize (mod.rs:263). */
    uint32_t pre_reorder_k;
    /* 1 (default for Tree-X-Hybrid; AsymmetricHasher::search_with_reordering,
     * hasher.rs:188-229): exact SquaredL2 re-rank of the pre_reorder_k candidates.
     * 0: return the k best by APPROXIMATE distance (AsymmetricHasher::search,
     * hasher.rs:162-185); pre_reorder_k is then ignored. */
    int32_t exact_reorder;
    /* optional per-stage outputs for parity checks (host pointers or NULL):
     *   tokens/token_dists [nq][P]      TreePartitioner::partition result (tree_partitioner.rs:196-229)
     *   cand_idx/cand_dist [nq][m], cand_count [nq]   merged candidates before re-rank (mod.rs:283-290) */
    uint32_t *tokens;
    float *token_dists;
    uint32_t *cand_idx;
    float *cand_dist;
    uint32_t *cand_count;
    /* TreeXHybridSearcher::search_with_filter(query, k, Some(filter)) for allow-list filters
     * (tree_x_hybrid/mod.rs:245-250, 327-332; restricts/allowlist.rs): bit i set = datapoint i
     * may be returned; disallowed points are skipped before scoring.  NULL = no filter.  Host
     * pointer in the host entry points, DEVICE pointer in the *_device entry points.
     * allow_bitmap_bits = the bitmap's capacity: ceil(bits / 64) words are read, bits at or past
     * the capacity in the last word are ignored, and datapoint indices >= capacity are not allowed
     * (allowlist.rs:97-100) -- capacity 0 allows nothing (empty rows).  Any other
     * `dyn RestrictFilter` is served by materialising is_allowed(0..n) into such a bitmap
     * (what scann.hpp's search_with_filter does).
     * Brute-force handles (f32, bf16, FP8 E4M3, int8 rows; every measure the handle serves): the reference's
     * BruteForceSearcher has no filter argument, so the contract is stated here.  A filtered search answers
     * exactly as an unfiltered search over a handle built from the allowed rows alone, taken in ascending
     * datapoint order, with each returned index mapped back to its datapoint index:
     *   - k = min(k, number of allowed rows); out_count reports it; slots past it hold 0xFFFFFFFF / +inf;
     *   - distances are bit-identical to the unfiltered arithmetic of the same handle;
     *   - ties are broken by TopK's (distance, index) rule (the mapping is monotone, so tie order is kept); a
     *     disallowed row that ties with the k-th allowed row never appears and never displaces one;
     *   - the bitmap rules above hold unchanged; NULL takes exactly the unfiltered code path.
     * Two mechanisms, chosen per call from the allowed fraction (SCANN_HIP_BF_FILTER_COMPACT_MAX, default 1: host
     * calls always take the first; forced by SCANN_HIP_BF_FILTER = 1 / 2): a compacted, ascending id list of the allowed rows that the kernels gather
     * (only allowed rows are read), or the unfiltered stream with a bit test where a row becomes a candidate.
     * Filtered calls never take the bf16-shortlist path: its acceptance proof bounds the rows OUTSIDE the
     * shortlist, disallowed ones included, so it would have to be restated over allowed rows only; they are
     * routed to the exact kernels (the cost: a filtered large batch runs at the bf_exact = 1 rate of its
     * allowed rows; not measured yet).  The few-query host pipeline applies the bit test in its scan.
     * The *_device entry point cannot learn the allowed count without a synchronisation: it takes the bit test
     * and documents its failure mode at scann_hip_index_last_device_status. */
    const uint64_t *allow_bitmap;
    uint64_t allow_bitmap_bits;
    /* Brute-force handles.  0 (default): large batches on large indexes take the bf16-shortlist
     * path (bf16 MFMA scores shortlist 4k rows per query, the reference's f32 arithmetic re-scores
     * them, and an error bound proves that no other row can enter the top k; results are
     * bit-identical to the exact kernels).  A query whose result cannot be proven sets status
     * Aborted: the host entry point repeats the batch on the exact kernels by itself, callers of the
     * *_device entry point repeat it with bf_exact = 1.  1: exact kernels only. */
    int32_t bf_exact;
    /* Per-query allow-lists: the distance, in 64-bit words, from the bitmap of query i of the call to the bitmap of
     * query i + 1.  0 (default): allow_bitmap is ONE bitmap for the whole batch -- exactly the behaviour and the code
     * path described at allow_bitmap.  Non-zero: query i reads words [i * stride, i * stride + ceil(allow_bitmap_bits
     * / 64)) of allow_bitmap, so a batch carries one filter per query (per-user ACLs, per-tenant subsets).  All
     * bitmaps of a call share the capacity allow_bitmap_bits and every rule stated at allow_bitmap holds per query,
     * unchanged: bits at or past the capacity are ignored, datapoint indices at or past it are not allowed, capacity
     * 0 allows nothing.  Words between one query's last word and the next query's first are never read.  A
     * non-zero stride below ceil(allow_bitmap_bits / 64) is InvalidArgument; with allow_bitmap = NULL the field is
     * ignored (there is no filter).  The host entry points copy nq * stride words to the device
     * (scann_hip_index_reserve sizes that copy from allow_bitmap_bits, the stride and max_nq when its opts carry a
     * non-NULL bitmap); the *_device entry points read them in place.  scann_hip_search_batched_params carries
     * bitmap row i with query i into its per-k groups; crowded, multi-attribute crowded and MMR searches forward
     * the field.  scann_hip_allow_bitmaps_from_ids[_device] builds such a block from id lists.
     * Unimplemented with a non-zero stride (and a non-NULL bitmap): brute-force handles (their filtered
     * k = min(k, allowed rows) and their compaction are per bitmap), scann_hip_mutable_search,
     * scann_hip_txh_search_local_device / scann_hip_txh_search_sharded_device, radius search. */
    uint64_t allow_bitmap_stride;
} scann_hip_search_opts;

void scann_hip_search_opts_default(scann_hip_search_opts *opts);

/* ---- search ---------------------------------------------------------------- */
/* Replaces, per index kind:
 *   BruteForceSearcher::{search, search_batched}       brute_force/searcher.rs:77-208
 *   AsymmetricHasher::{search, search_with_reordering, search_batched}  hashes/hasher.rs:162-238
 *   TreeXHybridSearcher::{search, search_with_filter(None)} + Searcher::search_batched_with_params
 *                                                       tree_x_hybrid/mod.rs:240-294, 382-409
 * queries: nq rows, row i at queries + i*q_stride, q_dim valid floats each.
 * q_dim != index dim -> InvalidArgument (searcher.rs:83-89, hasher.rs:167-171,
 * mod.rs:251-253).  out_idx/out_dist: [nq][k]; out_count: [nq]. */
int scann_hip_search_batched(scann_hip_index *index, const float *queries, uint32_t nq,
                             uint32_t q_stride, uint32_t q_dim, uint32_t k,
                             const scann_hip_search_opts *opts, uint32_t *out_idx,
                             float *out_dist, uint32_t *out_count);

/* Searcher::search_batched_with_params (searcher.rs:148-186; tree_x_hybrid/mod.rs:383-409, hashes/hasher.rs,
 * brute_force/searcher.rs: one SearchParameters per query, of which the searchers on this path read
 * num_neighbors): query i is searched with k_per_query[i] -- and therefore with ITS OWN pre-reorder candidate
 * count k_i * pre_reorder_multiplier when opts->pre_reorder_k is 0 -- exactly as a single search(query, k_i)
 * would.  Queries that share a k travel as one batch.  Row i of out_idx / out_dist starts at i * out_pitch
 * (out_pitch >= the largest k); slots past out_count[i] hold idx 0xFFFFFFFF, dist +inf. */
int scann_hip_search_batched_params(scann_hip_index *index, const float *queries, uint32_t nq,
                                    uint32_t q_stride, uint32_t q_dim, const uint32_t *k_per_query,
                                    const scann_hip_search_opts *opts, uint32_t out_pitch,
                                    uint32_t *out_idx, float *out_dist, uint32_t *out_count);

/* Same, all pointers device-resident, enqueued on `hip_stream`, no sync.  The caller
 * must first reserve workspace for the largest batch it will submit. */
int scann_hip_index_reserve(scann_hip_index *index, uint32_t max_nq, uint32_t max_k,
                            const scann_hip_search_opts *opts);
int scann_hip_search_batched_device(scann_hip_index *index, const float *d_queries,
                                    uint32_t nq, uint32_t q_stride, uint32_t k,
                                    const scann_hip_search_opts *opts, uint32_t *d_out_idx,
                                    float *d_out_dist, uint32_t *d_out_count,
                                    void *hip_stream);
/* Device status word of the last *_device call on this index (0 = ok, else a
 * scann_hip_status), synchronising the stream.  The device entry point does not retry; the
 * queries it could not finish have out_count 0:
 *   ResourceExhausted  a candidate buffer overflowed (more points tied at or passed the sampled
 *                      bound than the buffer sized from it holds) -- e.g. an allow-bitmap that
 *                      allows none of the points the bound's sample reads: no bound, and every
 *                      allowed point of a long stream is a candidate;
 *   Aborted            the sampled bound kept fewer than pre_reorder_k points for some query --
 *                      e.g. an allow-bitmap that allows the points the bound's sample reads but
 *                      few of the others.
 * Remedy for both: search those queries again through scann_hip_search_batched (the host entry
 * point repeats such a batch once without a bound and with a buffer for the whole stream).
 * Brute-force handles with an allow-bitmap: the device entry point streams every row and tests the bitmap
 * where a row becomes a candidate, with the bound taken over the ALLOWED rows of its 8192-row sample.  A
 * bitmap that leaves fewer than k allowed rows in that sample gives no bound; every allowed row is then a
 * candidate, and with more of them than the buffer sized from k holds the status is ResourceExhausted
 * (out_count 0 for those queries, never wrong rows).  Same remedy: the host entry point counts the allowed
 * rows and repeats over the compacted allowed rows.  A reserved handle does not allocate on such a call
 * (pass the opts with the bitmap to scann_hip_index_reserve so that host calls do not either). */
int scann_hip_index_last_device_status(scann_hip_index *index, void *hip_stream);
/* Debugging aid of the batched Tree-X-Hybrid / AsymmetricHasher pipeline: copies the filter bounds thr[0 .. nq) of
 * the last batched search enqueued on hip_stream (its workspace, else the primary one) to out_bounds.  A bound is
 * the merge key (ordered approximate distance << 32 | stream position) at or under which a scanned point becomes a
 * candidate, UINT64_MAX = no bound.  The CALLER synchronises hip_stream first; the copy itself is synchronous.
 * OutOfRange when the workspace has never held nq bounds. */
int scann_hip_index_debug_filter_bounds(scann_hip_index *index, void *hip_stream, uint32_t nq, uint64_t *out_bounds);
/* Debugging aid of the sparse prefilter's plan: the bytes of survivor bitmaps that the searches enqueued on hip_stream
 * (its workspace, else the primary one) have asked for so far -- 0 while every one of them flushed its survivors into
 * lists inside the scan, else the size of the largest [queries rounded up to 64][ranges of 1024 points][32] u32 array a
 * call of the bitmap form (SCANN_HIP_SP_BITMAP) wanted.  No device work. */
int scann_hip_index_debug_survivor_bitmap_bytes(scann_hip_index *index, void *hip_stream, uint64_t *out_bytes);
/* Debugging aid of the 8-bit row filter in front of the exact re-rank: copies what the last batched search enqueued on
 * hip_stream (its workspace, else the primary one) left there for nq queries of pre_reorder_k = m: the ordered lower
 * and upper bounds of every candidate's exact distance (out_lb, out_ub: [nq][m] u32, the order-preserving image of
 * an f32), the candidates' re-rank rows (out_rows: [nq][m]) and their number per query (out_counts: [nq]; 0x80000000 for a
 * query whose result rows the shortlist kernel wrote itself: its candidates are still in place, their number is not
 * kept); entries at and beyond a query's count are unspecified.  The bounds are those of the last search that ran the filter.  The
 * CALLER synchronises hip_stream first; the copies are synchronous.  OutOfRange when the workspace has never held a
 * filtered re-rank of that size. */
int scann_hip_index_debug_rerank_brackets(scann_hip_index *index, void *hip_stream, uint32_t nq, uint32_t m, uint32_t *out_lb,
                                          uint32_t *out_ub, uint32_t *out_rows, uint32_t *out_counts);

/* ---- crowding: at most per_crowd_limit results per attribute (restricts/crowding.rs) --------
 * CrowdingConstraint::apply (crowding.rs:81-104) behind every search, on the device.  For every handle kind
 * that scann_hip_search_batched serves (f32 and quantized brute force, flat hasher, Tree-X-Hybrid, Partitioned):
 *
 *   crowded(query, k, depth, limit)  ==  CrowdingConstraint::apply(search(query, depth), k)
 *
 * where search(query, depth) is exactly what scann_hip_search_batched returns for k = depth under the same opts
 * (allow_bitmap, pre_reorder_k, partitions_to_search, exact_reorder and bf_exact apply to it unchanged).  The rule:
 * walk that row in order and keep entry i iff fewer than per_crowd_limit EARLIER entries of the row carry the same
 * attribute; stop at k kept entries.  (The reference counts earlier KEPT entries; with one attribute per datapoint
 * the two counts decide alike.)  The rule is greedy and online, hence the prefix property: if the crowded result
 * over the first `depth` neighbours holds k entries, it is the crowded result over every deeper list that extends
 * them -- for a brute-force handle, over the whole database.
 *   - attributes: one u64 per DATAPOINT index, held on the device with the handle
 *     (scann_hip_index_set_crowding_attributes).  The array may be shorter than the index: an index at or past
 *     n_attrs has attribute 0 (get_attribute(idx).unwrap_or(0), crowding.rs:90) and crowds together with the rows
 *     whose attribute really is 0.
 *   - per_crowd_limit = 0 keeps nothing (empty rows, count 0); per_crowd_limit >= depth returns the first k of the row.
 *   - a row shorter than depth (fewer rows, fewer allowed rows, fewer candidates) is walked to its count; its
 *     sentinel slots are never looked up.
 *   - out_count[i] = number kept; slots past it hold 0xFFFFFFFF / +inf; distances are the bits the plain search
 *     returns.
 *   - depth = 0 means depth = k.
 * Errors: depth < k -> InvalidArgument; no attributes attached -> FailedPrecondition; a depth the handle does not
 * accept as k -> the error the plain search gives for that k (brute force: k > 2048 -> Unimplemented; on the device
 * path k > n -> InvalidArgument; hashed handles: a candidate count above 8192 -> Unimplemented); depth > 8192 ->
 * Unimplemented in any case.
 * CrowdingMultidimensional and MmrDiversifier (crowding.rs:123-268) are the two sections below.  Not built for any of
 * the three: a per-query k (the _params entry point), the leaf-sharded multi-GPU entry point.
 *
 * The stage is one kernel launch behind the handle's final select: one wave per query walks the [nq][depth] rows in
 * chunks of 64 with an open-addressed LDS table keyed on the full 64-bit attribute (a hash collision costs probes,
 * never a wrong count) and leaves the loop once k entries are kept.  scann_hip_crowd_table_slots(depth) is the
 * table's slot count, clamp(next_pow2(2 * depth), 128, SCANN_HIP_CROWD_MAX_SLOTS), 12 bytes each (at most 144 KB of
 * the workgroup's 160 KB); the home slot of a key is mulhi32(splitmix64-finaliser(key) >> 32, slots). */
#define SCANN_HIP_CROWD_MAX_DEPTH 8192
#define SCANN_HIP_CROWD_MAX_SLOTS 12288
uint32_t scann_hip_crowd_table_slots(uint32_t depth);
/* Copies attrs[0..n_attrs) to the device.  Calling again replaces the array; n_attrs = 0 detaches it (crowded
 * searches then fail FailedPrecondition).  Waits for the device; needs the same external synchronisation as
 * create / destroy (no search may run on the handle meanwhile). */
int scann_hip_index_set_crowding_attributes(scann_hip_index *index, const uint64_t *attrs, uint64_t n_attrs);
/* Host entry point (synchronous, host pointers; opts->allow_bitmap is a host pointer).  Queries (and the bitmap) go
 * up, the [nq][depth] rows stay in the slot's workspace between the search's final select and the crowding kernel,
 * and only the [nq][k] answer comes back.  The search is the enqueue-only batched pipeline of the *_device entry
 * point (not the polled pinned-staging pipeline of batches of <= 16 queries).  Where that search cannot serve the
 * call as scann_hip_search_batched would -- its status word reports a sampled bound that missed or a candidate buffer
 * that overflowed, a bf16-shortlist result could not be verified, a brute-force depth exceeds the index, opts asks
 * for per-stage outputs -- the call is answered through scann_hip_search_batched itself at k = depth (with its
 * repeats), whose rows are then sent back to the device for the crowding kernel.  Both routes give the same bits. */
int scann_hip_search_crowded(scann_hip_index *index, const float *queries, uint32_t nq, uint32_t q_stride,
                             uint32_t q_dim, uint32_t k, uint32_t depth, uint32_t per_crowd_limit,
                             const scann_hip_search_opts *opts, uint32_t *out_idx, float *out_dist,
                             uint32_t *out_count);
/* Device entry point: device pointers, enqueued on hip_stream, never synchronises, no host round trip: the search's
 * final select writes its [nq][depth] rows into the stream's workspace and the crowding kernel reads them there.
 * Same stream / workspace rules and status reporting (scann_hip_index_last_device_status) as
 * scann_hip_search_batched_device; a query the search could not finish has out_count 0.
 * scann_hip_index_reserve_crowded = scann_hip_index_reserve for k = max_depth plus the rows of the crowding stage
 * (max_depth = 0 means max_k); a call within the reserved sizes on the primary workspace does not allocate.  The
 * multi-attribute stage below needs nothing more: scann_hip_index_reserve_crowded reserves for it as well. */
int scann_hip_index_reserve_crowded(scann_hip_index *index, uint32_t max_nq, uint32_t max_k, uint32_t max_depth,
                                    const scann_hip_search_opts *opts);
int scann_hip_search_crowded_device(scann_hip_index *index, const float *d_queries, uint32_t nq, uint32_t q_stride,
                                    uint32_t k, uint32_t depth, uint32_t per_crowd_limit,
                                    const scann_hip_search_opts *opts, uint32_t *d_out_idx, float *d_out_dist,
                                    uint32_t *d_out_count, void *hip_stream);

/* ---- multi-attribute crowding: CrowdingMultidimensional::apply (restricts/crowding.rs:166-200) --------
 *
 *   crowded_md(query, k, depth, limits)  ==  CrowdingMultidimensional::apply(search(query, depth), k)
 *
 * with search(query, depth) as in the crowding section above.  Every datapoint carries one u64 attribute in each of
 * n_dims dimensions ("seller", "brand", ...).  The row is walked in order; entry i is kept iff, for EVERY dimension j,
 * fewer than limits[j] EARLIER KEPT entries carry its attribute in dimension j; the walk stops at k kept.  (Here the
 * kept count cannot be replaced by a count of earlier entries: an entry one dimension rejects does not count in the
 * others.)
 *   - attributes: a [n_dims][n_attrs] u64 array, dimension-major, held on the device with the handle
 *     (scann_hip_index_set_crowding_attributes_md); separate from the one-attribute array, setting one does not touch
 *     the other.  n_dims <= SCANN_HIP_CROWD_MAX_DIMS.  An index at or past n_attrs has attribute 0 in every dimension.
 *   - limits: exactly n_dims values (n_limits != n_dims -> InvalidArgument; the reference indexes limits[dim] and
 *     panics on a short vector).  A limit of 0 in any dimension keeps nothing.
 *   - depth <= 8192, depth = 0 means depth = k, short rows, the sentinel fill and out_count: as for the one-attribute
 *     stage.  k = 0 returns no entry (the reference returns one: it tests the length after the push).
 *   - n_dims * min(k, depth) > 6144 -> Unimplemented: the LDS table counts accepted entries only, at most that many
 *     keys, and 6144 is half of the SCANN_HIP_CROWD_MAX_SLOTS slots that fit the workgroup's LDS.
 *   - with n_dims = 1 the result equals scann_hip_search_crowded bit for bit.
 * Errors: depth < k -> InvalidArgument; no multi-attribute array attached -> FailedPrecondition; n_dims 0 or above
 * SCANN_HIP_CROWD_MAX_DIMS -> InvalidArgument; a depth the handle does not accept as k -> the plain search's error.
 * One kernel launch behind the search: one wave per query, chunks of 64 entries; per chunk the lanes of equal attribute
 * are found per dimension with ballots, and the chunk's accept decisions are the fixed point of "accepted for certain /
 * rejected for certain / undecided" over two ballots (each iteration decides at least the lowest undecided lane).
 * Host entry, device entry, fall-back rules, stream / workspace rules and status reporting are those of the crowded
 * entry points; scann_hip_crowd_md_apply runs the stage alone over the caller's rows (host pointers, [nq][depth] at
 * pitch depth, rows_count[i] <= depth else InvalidArgument). */
#define SCANN_HIP_CROWD_MAX_DIMS 8
/* Copies attrs[0 .. n_dims * n_attrs) to the device.  Calling again replaces the array; n_attrs = 0 detaches it.
 * Waits for the device; same external synchronisation as scann_hip_index_set_crowding_attributes. */
int scann_hip_index_set_crowding_attributes_md(scann_hip_index *index, const uint64_t *attrs, uint32_t n_dims,
                                               uint64_t n_attrs);
int scann_hip_search_crowded_md(scann_hip_index *index, const float *queries, uint32_t nq, uint32_t q_stride,
                                uint32_t q_dim, uint32_t k, uint32_t depth, const uint32_t *limits, uint32_t n_limits,
                                const scann_hip_search_opts *opts, uint32_t *out_idx, float *out_dist,
                                uint32_t *out_count);
/* limits is a HOST pointer (read during the call); everything else as scann_hip_search_crowded_device. */
int scann_hip_search_crowded_md_device(scann_hip_index *index, const float *d_queries, uint32_t nq, uint32_t q_stride,
                                       uint32_t k, uint32_t depth, const uint32_t *limits, uint32_t n_limits,
                                       const scann_hip_search_opts *opts, uint32_t *d_out_idx, float *d_out_dist,
                                       uint32_t *d_out_count, void *hip_stream);
int scann_hip_crowd_md_apply(scann_hip_index *index, const uint32_t *rows_idx, const float *rows_dist,
                             const uint32_t *rows_count, uint32_t nq, uint32_t depth, uint32_t k, const uint32_t *limits,
                             uint32_t n_limits, uint32_t *out_idx, float *out_dist, uint32_t *out_count);

/* ---- MMR: MmrDiversifier::apply (restricts/crowding.rs:203-268) ------------------------------------
 *
 *   mmr(query, k, depth, lambda)  ==  MmrDiversifier::new(lambda).apply(search(query, depth), k, sim)
 *
 * with search(query, depth) as in the crowding section and sim(a, b) = -DistanceMeasure::distance(row[a], row[b]) under
 * the handle's own measure (DotProduct: the dot product; SquaredL2 / L2 / L1: the negated distance; Cosine: cos - 1), in
 * the reference's pair arithmetic (bitwise symmetric in a and b).  Selection: entry 0 of the row first; every later
 * round scores the entries not yet selected, in row order, as
 *     score = lambda * (-dist) - (1 - lambda) * max_sim          (f32; two products and a subtraction, each rounded)
 * where max_sim is the f32::max fold of sim(entry, s) over the selected entries starting from f32::MIN (a NaN similarity
 * is ignored, a -inf one leaves f32::MIN).  The winner is the first entry whose score is strictly greater than every
 * earlier one, the running best starting at f32::MIN; if no score exceeds f32::MIN (all NaN, -inf or <= MIN) the
 * lowest-position remaining entry is taken.  Rounds continue until min(k, row count) entries are selected.
 *   - entries are written in SELECTION order, not distance order; distances are the plain search's bits;
 *     out_count = min(k, count); slots past it hold 0xFFFFFFFF / +inf; a short row is walked to its count.
 *   - lambda outside [0, 1] is clamped (as new() does); NaN -> InvalidArgument.  k = 0: empty rows (host entry).
 *   - depth = 0 means depth = k; depth < k -> InvalidArgument; depth > SCANN_HIP_MMR_MAX_DEPTH -> Unimplemented.
 *   - served: handles whose f32 rows are addressable by datapoint index: f32 brute force; Tree-X-Hybrid, flat-hasher
 *     and Partitioned handles created with `data` in datapoint order.  Unimplemented: quantized brute-force handles,
 *     handles whose rows are held only in CSR order (data_is_csr_order), shards (leaf_sizes_global).
 *     FailedPrecondition: a hashed handle without `data`.
 * One kernel launch behind the search: one 256-thread workgroup per query; per round every thread folds its entries'
 * max_sim against the LAST selected row only (a running max), then the workgroup reduces to the winner by (score,
 * lowest position).  Candidate rows are read from global memory: k re-reads of depth rows per query, L2 traffic after
 * the first round.  Host entry, device entry, fall-back rules, stream / workspace rules and status reporting are those
 * of the crowded entry points; scann_hip_index_reserve_mmr is scann_hip_index_reserve_crowded with MMR's depth limit.
 * scann_hip_mmr_apply runs the stage alone over the caller's rows (host pointers, [nq][depth] at pitch depth):
 * rows_count[i] <= depth and every rows_idx below the row's count < the index size, else InvalidArgument. */
#define SCANN_HIP_MMR_MAX_DEPTH 2048
int scann_hip_search_mmr(scann_hip_index *index, const float *queries, uint32_t nq, uint32_t q_stride, uint32_t q_dim,
                         uint32_t k, uint32_t depth, float lambda, const scann_hip_search_opts *opts, uint32_t *out_idx,
                         float *out_dist, uint32_t *out_count);
int scann_hip_search_mmr_device(scann_hip_index *index, const float *d_queries, uint32_t nq, uint32_t q_stride,
                                uint32_t k, uint32_t depth, float lambda, const scann_hip_search_opts *opts,
                                uint32_t *d_out_idx, float *d_out_dist, uint32_t *d_out_count, void *hip_stream);
int scann_hip_index_reserve_mmr(scann_hip_index *index, uint32_t max_nq, uint32_t max_k, uint32_t max_depth,
                                const scann_hip_search_opts *opts);
int scann_hip_mmr_apply(scann_hip_index *index, const uint32_t *rows_idx, const float *rows_dist,
                        const uint32_t *rows_count, uint32_t nq, uint32_t depth, uint32_t k, float lambda,
                        uint32_t *out_idx, float *out_dist, uint32_t *out_count);

/* ---- multi-GPU: leaf-sharded Tree-X-Hybrid ------------------- */
/* Local stage: this rank's best-m candidates per query by approximate distance, with
 * their exact distances, as (merge key u64, datapoint idx u32, exact f32) triples
 * [nq][m] (+ count [nq]).  The merge key orders candidates exactly as the reference's
 * flatten + stable sort does (mod.rs:283-290) and is identical on every rank.
 * A candidate that provably cannot be among the k best exact distances of ANY prefix of
 * this rank's list (k candidates with smaller merge keys are nearer: int8 row brackets,
 * lists of > 512 candidates, SquaredL2) carries exact = +inf instead of its distance; it
 * still counts as one of the m candidates.  Merging (scann_hip_txh_merge_device, with a
 * num_neighbors <= the k of this call) returns the same rows as with every distance filled in. */
int scann_hip_txh_search_local_device(scann_hip_index *index, const float *d_queries,
                                      uint32_t nq, uint32_t q_stride, uint32_t k,
                                      const scann_hip_search_opts *opts, uint64_t *d_keys,
                                      uint32_t *d_idx, float *d_exact, uint32_t *d_count,
                                      void *hip_stream);
/* Merge stage on the gathered triples of `world` ranks ([world][nq][m_local] each):
 * stable sort by key -> truncate m -> stable sort by exact -> truncate k
 * (mod.rs:289-290, 360-361).  m_local is the per-rank pre_reorder_k of the local stage.
 * m_local == m is exact by construction.  m_local < m (a random shard holds ~m/world of the
 * global best m) is verified: if a truncated rank could have held more members,
 * *d_status (caller-zeroed device word, may be NULL) is raised to Aborted and the caller
 * re-runs with m_local = m.
 * rank_stride_bytes: 0 for dense arrays; otherwise the four pointers address rank 0's
 * sections of a packed per-rank buffer and rank g's sections lie g * rank_stride_bytes
 * further (one all_gather of [keys | idx | exact | count] instead of four). */
int scann_hip_txh_merge_device(scann_hip_ctx *ctx, uint32_t world, uint32_t nq, uint32_t m_local,
                               uint32_t m, uint32_t k, uint64_t rank_stride_bytes,
                               const uint64_t *d_keys,
                               const uint32_t *d_idx, const float *d_exact,
                               const uint32_t *d_count, uint32_t *d_out_idx, float *d_out_dist,
                               uint32_t *d_out_count, uint32_t *d_status, void *hip_stream);
/* Exchange by all_to_all instead of all_gather (xGMI is point-to-point: every rank sends each peer
 * only the candidates of the queries that peer merges).  Repacks the local stage's arrays
 * [nq][m_local] into `world` destination blocks, block d = the queries [d*nq/world, (d+1)*nq/world):
 * [keys u64 | idx u32 | exact f32 | count u32], block_bytes apart (>= (nq/world)*(16*m_local + 4),
 * multiple of 8).  After all_to_all_single (equal splits) a rank holds one block per source rank
 * and calls scann_hip_txh_merge_device with nq/world queries and rank_stride_bytes = block_bytes.
 * nq must be a multiple of world. */
int scann_hip_txh_pack_blocks_device(scann_hip_ctx *ctx, uint32_t world, uint32_t nq, uint32_t m_local,
                                     const uint64_t *d_keys, const uint32_t *d_idx, const float *d_exact,
                                     const uint32_t *d_count, void *d_out, uint64_t block_bytes,
                                     void *hip_stream);

/* Greedy size-balanced leaf->rank assignment used by the harness (not in the reference). */
int scann_hip_assign_leaves(const uint32_t *leaf_sizes, uint32_t num_partitions,
                            uint32_t world, uint32_t *out_owner);

/* ---- multi-GPU exchange inside the library: RCCL over xGMI --------------------
 * One process per GPU; every process holds a communicator.  A host that is not Python needs
 * nothing else: rank 0 calls scann_hip_comm_unique_id and hands the 128 bytes to the other ranks
 * over any side channel (a file, a socket, MPI, torch.distributed ...), every rank then calls
 * scann_hip_comm_create (collective).  librccl.so.1 is loaded on first use; without it these entry
 * points return Unavailable and everything else in the library keeps working.
 *
 * scann_hip_txh_search_sharded_device = the whole north-star step for a leaf-sharded index
 * (every rank created its shard with leaf_sizes_global set and data_is_csr_order = 1):
 *   local stage (this rank's best m_local candidates per query by merge key + their exact
 *   distances) -> one block per destination rank -> ONE all-to-all as grouped ncclSend/ncclRecv
 *   (xGMI is point-to-point: each peer receives only the candidates of the nq/world queries it
 *   merges) -> merge of this rank's queries (stable sort by key, truncate m, stable sort by exact,
 *   truncate k: tree_x_hybrid/mod.rs:283-293, 360-361) -> ncclAllGather of the k result rows.
 * All ranks pass the same queries, nq, k and options; every rank receives all nq result rows
 * ([nq][k] / [nq], device pointers).  m_local = 0 means m with destination blocks sized for the worst
 * case (exact by construction); m_local > 0 sends compact blocks (scann_hip_comm_layout) and is verified
 * by the merge -- a too-short list or an overflowing block gives scann_hip_comm_last_status -> Aborted on
 * every rank: repeat the batch with 0.
 * The exchange runs on the communicator's own stream; `hip_stream` carries the local stage and,
 * at the end of the call, waits for the results.  Internal buffers are double-buffered and ordered
 * with events, so a caller that alternates between two streams (and two sets of output buffers)
 * overlaps one step's exchange with the next step's local stage. */
typedef struct scann_hip_comm scann_hip_comm;
#define SCANN_HIP_UNIQUE_ID_BYTES 128
int scann_hip_comm_unique_id(void *out_id /* SCANN_HIP_UNIQUE_ID_BYTES */);
int scann_hip_comm_create(scann_hip_ctx *ctx, const void *unique_id, int rank, int world,
                          scann_hip_comm **out_comm);
void scann_hip_comm_destroy(scann_hip_comm *comm);
int scann_hip_txh_search_sharded_device(scann_hip_index *index, scann_hip_comm *comm,
                                        const float *d_queries, uint32_t nq, uint32_t q_stride,
                                        uint32_t k, const scann_hip_search_opts *opts,
                                        uint32_t m_local, uint32_t *d_out_idx, float *d_out_dist,
                                        uint32_t *d_out_count, void *hip_stream);
/* Byte layout of one sharded step for nq queries (no GPU needed; for hosts that size their own
 * buffers and for the protocol tests): out[0..16) = { qr = queries merged per rank (the batch is
 * padded to qr * world), nq_pad, block_bytes (one destination block = the bytes a rank sends each peer
 * over its xGMI link per step), offset of idx, of exact, of count inside a block, bytes of
 * the local-stage arrays [nq][m_local] and the offsets of idx, exact, count inside them, bytes of
 * the result rows ([nq_pad][k] idx | dist | [nq_pad] count | [world] status) and the offset of dist,
 * offset of keys inside a block, cap = entries a block has room for, offset of the block's overflow flag,
 * offset of the status words inside the result rows }.
 * A destination block is COMPACT: [count u32[qr] | overflow flag u32 | pad to 16 | keys u64[cap] | idx u32[cap] |
 * exact f32[cap]], the entries of the block's queries one behind the other.  cap = min(qr * m_local, max(m_local,
 * ceil(fill * qr * m_local / world))) with fill = SCANN_HIP_COMM_FILL (default 2.5): the candidates of one query total
 * about m over ALL ranks, so a peer's share averages m_local / world per query.  A block that overflows is flagged,
 * scann_hip_comm_last_status then returns Aborted on EVERY rank (the status words are gathered with the rows), and
 * the caller repeats the batch with m_local = 0, which sizes the blocks for the worst case (cap = qr * m).
 * This function reports the layout of calls with m_local > 0. */
int scann_hip_comm_layout(uint32_t nq, uint32_t world, uint32_t m_local, uint32_t k, uint64_t *out16);
/* Status of the merges since the last call of this function (0 = ok, Aborted = an m_local < m list
 * was too short or a compact block overflowed -- the same answer on every rank); synchronises the
 * communicator's stream and clears the word. */
int scann_hip_comm_last_status(scann_hip_comm *comm);

/* ---- index files ---------------------------------------------------------
 * The reference keeps indexes in memory only (no save/load: SURVEY section 5); its arrays are the
 * DenseDataset buffer (data_format/dataset.rs:46-61), TreePartitioner.centers and the partition
 * lists (partitioning/partitioner.rs:132-142, tree_x_hybrid/mod.rs:81-90), the Codebook and the
 * per-point codes.  One little-endian container holds exactly the fields of scann_hip_txh_desc /
 * the arguments of scann_hip_bf_create, so the GPU library, the CPU oracle (numpy reader:
 * scann_rust_amd/index_file.py) and the golden fixtures share it:
 *
 *   [0, 256)   header   "SCANNIDX", version 1, kind (0 brute force, 1 tree / hasher index), the
 *                        scalar descriptor fields, section count, file size
 *   [256, ...) table    64 bytes per section: name[24], dtype (0 f32, 1 u32, 2 u8), offset, bytes
 *   sections   "data" "centers" "leaf_offsets" "leaf_ids" "leaf_sizes_global" "codebook" "codes",
 *              each starting on a 4096-byte boundary (absent arrays have no section)
 *
 * write: host arrays -> file.  load: the file is mmap'ed (never read into a second host copy), the
 * mapping pinned for DMA when the driver allows it (SCANN_HIP_LOAD_PIN=0 skips that), and the
 * arrays uploaded by the same code as scann_hip_*_create.  Errors: missing file -> NotFound; bad
 * magic / version -> InvalidArgument; truncated or inconsistent file -> DataLoss. */
typedef struct {
    uint32_t version;
    uint32_t kind;                 /* 0 = brute force, 1 = tree / hasher index */
    uint64_t n_rows, n_local, file_bytes;
    uint32_t dim, stride, num_partitions, num_subspaces, num_codes, dims_per_subspace;
    int32_t distance_measure, data_is_csr_order, codes_packed4, use_residuals;
    uint32_t partitions_to_search;
    float pre_reorder_multiplier;
    int32_t has_data;              /* exact re-ordering possible */
} scann_hip_file_info;
int scann_hip_txh_write_file(const char *path, const scann_hip_txh_desc *desc);
int scann_hip_bf_write_file(const char *path, const float *data, uint64_t n, uint32_t dim,
                            uint32_t stride, int measure);
int scann_hip_index_file_info(const char *path, scann_hip_file_info *out_info);
int scann_hip_index_load_file(scann_hip_ctx *ctx, const char *path, scann_hip_index **out_index);
/* Writes a HANDLE to the container: its arrays are read back from the device and stored in the sections of
 * scann_hip_txh_write_file / scann_hip_bf_write_file (codes in the PackedCodes4Bit byte layout with codes_packed4 = 1
 * when num_codes <= 16, one byte per subspace otherwise; a handle created without rows has no "data" section, and as
 * it keeps no row count, n_rows is written as the smallest count that holds every datapoint index).  This is
 * how an index made by scann_hip_fold_mutable is persisted; scann_hip_index_load_file on the file gives a handle that
 * searches identically.  Any unsharded f32 brute-force, tree, hasher or Partitioned handle, and tree / hasher handles
 * over quantized rows (scann_hip_txh_create_quantized: "rows_q" / "rows_q_meta" instead of "data"); quantized
 * brute-force rows and shards (leaf_sizes_global) -> Unimplemented.  Transient host memory: one copy of the index. */
int scann_hip_index_write_file(const scann_hip_index *index, const char *path);

/* ---- building blocks exposed for parity tests / callers ---------------------- */
/* TreePartitioner::partition for a batch (tree_partitioner.rs:196-229). */
int scann_hip_txh_partition(scann_hip_index *index, const float *queries, uint32_t nq,
                            uint32_t q_stride, uint32_t q_dim, uint32_t num_partitions,
                            uint32_t *out_tokens, float *out_dists, uint32_t *out_count);
/* LookupTable::from_query (hashes/lut.rs:47-70) for nq queries; leaf_for_query NULL =
 * no residual, else residual against centers[leaf_for_query[i]] (mod.rs:309-316).
 * out_lut: [nq][S][K]. */
int scann_hip_lut_from_query(scann_hip_index *index, const float *queries, uint32_t nq,
                             uint32_t q_stride, const uint32_t *leaf_for_query,
                             float *out_lut);
/* LookupTable::compute_distance over every local point (hashes/lut.rs:74-82,
 * hasher.rs:179-182) for nq explicit f32 LUTs [nq][S][K]: out [nq][n_local] in CSR
 * row order. */
int scann_hip_adc_distances(scann_hip_index *index, const float *luts, uint32_t nq,
                            float *out_dist);
/* Lut16SimdTables::compute_distances_batch (hashes/lut16_simd.rs:119-141 ->
 * simd/dispatch.rs:259-295): u8 tables [S][16], packed codes [n][ceil(S/2)];
 * out[i] = sum_u32 * multiplier + bias * S. */
int scann_hip_lut16_distances_batch(scann_hip_ctx *ctx, const uint8_t *packed_codes,
                                    const uint8_t *lut8, uint32_t num_subspaces, uint64_t n,
                                    float bias, float multiplier, float *out);
/* Lut16SimdTables::from_float_tables (hashes/lut16_simd.rs:39-90): global min / max over the
 * S x 16 f32 tables, scale = 255 / range, lut8 = round((v - min) * scale) as u8 (round half away
 * from zero, saturating), bias = min, multiplier = 1 / scale; range < 1e-10 -> scale = multiplier
 * = 1.  S == 0 -> bias 0, multiplier 1, nothing written.  Runs on the device (one workgroup). */
int scann_hip_lut16_quantize(scann_hip_ctx *ctx, const float *tables, uint32_t num_subspaces,
                             uint8_t *out_lut8, float *out_bias, float *out_multiplier);
/* The reference's FP8 codec and quantizer (quantization/fp8.rs:80-268) -- its own bit-level conversion,
 * not a hardware format table: exponent bias 7 (E4M3) / 15 (E5M2); a mantissa carry wraps without bumping
 * the exponent; the top exponent field only encodes the maximum (0x7E / 0x7C: overflow, infinity, NaN);
 * values under the smallest normal flush to signed zero.
 *   quantize:   out[i] = from_f32(values[i] * scale)      (Quantizer::quantize over Fp8Quantizer, :247-255)
 *   dequantize: out[i] = to_f32(bits[i]) / scale          (:257-264)
 * (calibrate_scale, :238-244, is fp8_max / max(max_abs, 1e-10) with fp8_max 448 / 57344: a host one-liner.) */
#define SCANN_HIP_FP8_E4M3 0
#define SCANN_HIP_FP8_E5M2 1
int scann_hip_fp8_quantize(scann_hip_ctx *ctx, const float *values, uint64_t n, float scale, int format,
                           uint8_t *out_bits);
int scann_hip_fp8_dequantize(scann_hip_ctx *ctx, const uint8_t *bits, uint64_t n, float scale, int format,
                             float *out_values);
/* one_to_many_fp8_float_squared_l2 / one_to_many_fp8_float_dot_product
 * (distance_measures/one_to_many_asymmetric.rs:327-377): f32 query against E4M3 rows [num_points][stride],
 * one sequential f32 sum per row; measure SCANN_HIP_SQUARED_L2 or SCANN_HIP_DOT_PRODUCT (negated), others
 * Unimplemented.  Bit-identical to the reference's loops.  The same codec, with a per-row calibrate_scale,
 * is the optional FP8 row store of the re-rank filter (SCANN_HIP_RERANK_STORE=fp8 at index creation). */
int scann_hip_fp8_distances(scann_hip_ctx *ctx, const float *query, uint32_t dim, const uint8_t *database,
                            uint64_t stride, uint64_t num_points, int measure, float *out_distances);
/* Codebook::encode over rows (hashes/codebook.rs:82-95, 205-215); optional residual
 * against centers[leaf_of_row[i]] (tree_x_hybrid/mod.rs:177-189).  out_codes [n][S]. */
int scann_hip_encode(scann_hip_ctx *ctx, const float *codebook, uint32_t num_subspaces,
                     uint32_t num_codes, uint32_t dims_per_subspace, const float *rows,
                     uint64_t n, uint32_t stride, const float *centers,
                     const uint32_t *leaf_of_row, uint8_t *out_codes);
/* one_to_many_{squared_l2,dot_product}_strided for a batch = the dense Q x N matrix of
 * batch_squared_l2_simd / batch_dot_product_simd (distance_measures/one_to_many.rs:228-373,
 * many_to_many.rs:301-373).  out [nq][n]. */
int scann_hip_bf_distances(scann_hip_index *index, const float *queries, uint32_t nq,
                           uint32_t q_stride, float *out);

/* ---- index build on the GPU ------------------------------------------
 * K-means over the rows of a brute-force index, or over the column window [col_offset,
 * col_offset + sub_dim) of them (per-subspace codebook training, src/hashes/codebook.rs:177-199).
 *
 * simd_threshold = KMeansConfig.simd_threshold (src/trees/kmeans.rs:43-46, default 128): distances
 *   over sub_dim >= simd_threshold values use the AVX2 summation order of squared_l2_f32 (8 FMA lane
 *   chains + fixed horizontal-sum tree + unfused scalar tail, simd/x86.rs:139-165), shorter ones the
 *   sequential scalar sum (:419-431).  0 = always the AVX2 order, UINT32_MAX = always sequential.
 * scann_hip_kmeans_init_pp: KMeans::kmeans_plusplus_init (src/trees/kmeans.rs:295-349); centers_out
 *   [k][sub_dim].  DEVIATION (seeding parity is unpinned by construction): the reference draws from
 *   rand::StdRng, which is not reproducible here -- a documented splitmix64 stream is
 *   used instead -- and its D^2 sampling sums min_d sequentially in f32 (:318-331), an n-long
 *   dependent chain per seed; here the total and the cumulative search run in f64 with a fixed
 *   reduction tree.  The minimum distances themselves follow the reference's arithmetic.
 *   The rule, as tests/build_model.py restates it: splitmix64(seed) output 0 mod n is the first seed; every
 *   later seed consumes two outputs in order, u = (z >> 11) 2^-53 and fallback = z mod n; min_d[i] is the
 *   smallest squared distance of row i to a chosen seed (strict '<': a NaN minimum stays); the seed is the
 *   first row whose cumulative min_d reaches u * total.  total == 0 (every row already coincides with a
 *   seed, e.g. k > number of distinct rows): rows[fallback].  total == +inf: the first row whose min_d is
 *   +inf (the rule read in the extended reals).  total NaN (a row with a NaN element makes its min_d NaN):
 *   rows[fallback] as well -- a second DEVIATION: no comparison of the reference's loop holds against a NaN
 *   threshold, so it would select row 0 every time.
 *   Because the sums are rounded f64 sums in tree order, a seed may differ from the exactly evaluated rule
 *   only where the cumulative sum lies within (n + 1) 2^-52, relatively, of u * total.
 * scann_hip_kmeans_lloyd: the Lloyd loop of KMeans::fit_single (:210-263) from the caller's initial
 *   centres (updated in place): assign_clusters (strict '<', lowest index on ties), inertia = the f64
 *   sum of the minimum distances in datapoint order (:376; computed by a reduction tree when every
 *   partial sum is exactly representable -- then all orders agree -- and by the sequential chain
 *   otherwise), stop when |prev - inertia| / (prev + 1e-10) < convergence_threshold, update_centers
 *   (f64 sums in ascending datapoint order, mean cast to f32, empty cluster c takes row c % n), then
 *   the final assignment.  Bit-identical to the reference's loop from the same initial centres.
 *   Outputs may be NULL.  A row whose every distance is NaN (a NaN element in the row, or in every centre)
 *   joins cluster 0 and adds +inf to the inertia, as assign_clusters' min_dist does.
 * LIMIT: the assignment stages whole centres in LDS (160 KB per workgroup), each padded to a multiple of 4
 *   values: 16 centres in the sequential order (8 where 16 do not fit, sub_dim > 2560), 8 in the AVX2 order.
 *   sub_dim > 5120 makes scann_hip_kmeans_lloyd return ResourceExhausted in either order (the seeding stages
 *   no centres and has no such limit). */
int scann_hip_kmeans_init_pp(scann_hip_index *bf_index, uint32_t col_offset, uint32_t sub_dim, uint32_t k,
                             uint64_t seed, uint32_t simd_threshold, float *centers_out);
int scann_hip_kmeans_lloyd(scann_hip_index *bf_index, uint32_t col_offset, uint32_t sub_dim, float *centers,
                           uint32_t k, uint32_t max_iterations, double convergence_threshold,
                           uint32_t simd_threshold, uint32_t *out_assign, uint32_t *out_sizes,
                           double *out_inertia, uint32_t *out_iterations, int *out_converged);

/* BruteForceSearcher::search_radius (src/brute_force/searcher.rs:142-167) for one query: every
 * datapoint with distance <= radius, stable-sorted by distance.  Writes at most `capacity` rows;
 * *out_count receives the number found (call again with a larger capacity if it exceeds it).
 * Empty dataset -> OK with 0 rows; wrong q_dim -> InvalidArgument.
 * scann_hip_bf_search_radius_opts: the same with opts->allow_bitmap (host pointer) applied -- every ALLOWED
 * datapoint with distance <= radius, i.e. the radius search of a handle built from the allowed rows alone,
 * indices mapped back.  opts == NULL or a NULL bitmap is scann_hip_bf_search_radius; other fields are not read. */
int scann_hip_bf_search_radius_opts(scann_hip_index *index, const float *query, uint32_t q_dim, float radius,
                                    const scann_hip_search_opts *opts, uint32_t *out_idx, float *out_dist,
                                    uint64_t capacity, uint64_t *out_count);
/* Rows of an n-row index that an allow-bitmap (host pointer) of capacity allow_bitmap_bits allows: the set bits
 * below min(allow_bitmap_bits, n).  This is the count the host entry points plan a filtered brute-force search
 * with (k = min(k, count), the choice between the compacted id list and the bit test); needs no device. */
uint64_t scann_hip_allow_bitmap_count(const uint64_t *allow_bitmap, uint64_t allow_bitmap_bits, uint64_t n);

/* RestrictAllowlist::from_indices (restricts/allowlist.rs:27-40) for a whole batch: the strided bitmap block of
 * scann_hip_search_opts.allow_bitmap_stride from per-query id lists.  Query i's ids are ids[offsets[i] ..
 * offsets[i + 1]) (offsets: nq + 1 ascending values); bit id of its bitmap -- words [i * stride_words, i *
 * stride_words + ceil(bits / 64)) of out_words -- is set for every id < bits.  All nq * stride_words words are
 * written, the gap words as zero; an id at or past `bits` is ignored; duplicates and unsorted lists are fine.
 * stride_words < ceil(bits / 64) -> InvalidArgument.  Host form: host pointers, no context, no GPU.  Device form:
 * device pointers, a clear and one scatter kernel (64-bit atomic OR) enqueued on hip_stream, no synchronisation;
 * its output is bitwise the host form's. */
int scann_hip_allow_bitmaps_from_ids(const uint32_t *ids, const uint64_t *offsets, uint32_t nq, uint64_t bits,
                                     uint64_t stride_words, uint64_t *out_words);
int scann_hip_allow_bitmaps_from_ids_device(scann_hip_ctx *ctx, const uint32_t *d_ids, const uint64_t *d_offsets,
                                            uint32_t nq, uint64_t bits, uint64_t stride_words, uint64_t *d_out_words,
                                            void *hip_stream);

/* ---- tag filters: a device-resident token map that writes per-query bitmaps (restricts/allowlist.rs:184-244) ----
 * RestrictTokenMap: each datapoint carries any number of u64 tokens; create_allowlist(tokens) allows a datapoint that
 * has at least one of the tokens.  The handle holds the map on the device -- the distinct tokens ascending, a CSR of
 * offsets, the concatenated ascending postings -- uploaded once and shared by every query of every batch; a batch
 * sends a few tokens per query and one kernel writes the strided bitmap block of
 * scann_hip_search_opts.allow_bitmap_stride.
 *   create   pair i is add_token(indices[i], tokens[i]) (:206-211).  The bitmap of a token set is a set union and
 *            RestrictAllowlist::add ignores an index at or past the capacity (:59-65), so the pairs are sorted by
 *            (token, index) on the host, duplicates and indices >= num_datapoints dropped.  n_pairs = 0 gives a valid
 *            empty map.  num_datapoints >= 2^32 - 1 -> OutOfRange; null arrays with n_pairs > 0 -> InvalidArgument.
 *            A created map does not change (add_token after create: build a new map).
 *   num_tokens        distinct tokens as given (HashMap::len, :241-243): a token whose every index was out of range
 *                     still counts.
 *   get_indices       the STORED posting: ascending, deduplicated, below num_datapoints.  DEPARTURE from the reference,
 *                     whose get_indices (:221-223) returns insertion order with duplicates and out-of-range indices
 *                     (scann.hpp's host RestrictTokenMap keeps that order).  *out_n receives the count; an unknown
 *                     token gives 0 and Ok (the reference's None); capacity < count -> ResourceExhausted with *out_n
 *                     set and nothing written.
 * Bitmaps of a batch (create_allowlist per query, :226-238): query i names q tokens[offsets[i] .. offsets[i + 1])
 * (offsets: nq + 1 ascending values); bit j of its bitmap -- words [i * stride_words, i * stride_words +
 * ceil(num_datapoints / 64)) -- is set iff some named token has j in its posting.  The capacity is the map's
 * num_datapoints (pass it as allow_bitmap_bits).  The contract is that of scann_hip_allow_bitmaps_from_ids: all nq *
 * stride_words words are written, gap words as zero; stride_words < ceil(bits / 64) or >= 2^32 -> InvalidArgument.
 * Unknown tokens, repeated tokens and empty lists are fine (an empty list gives an all-zero bitmap).
 *   _device           device pointers; ONE kernel enqueued on hip_stream: no clear, no global atomic, no
 *                     synchronisation, no count visits the host.  A search enqueued on the same stream right after it
 *                     reads the block in place.  Workgroup (t, y) assembles tile t (SCANN_HIP_TOKEN_TILE_BITS bits) of
 *                     the bitmaps of queries y, y + gridDim.y, ... in LDS and stores it once, 16 bytes a lane.
 *   (no suffix)       host pointers, synchronous: lists up, the same kernel, the block back.  One call at a time per
 *                     map (serialised inside).
 *   scann_hip_allow_bitmaps_from_tokens   stateless, on the host, no context, no GPU: the model and the form for
 *                     machines without a device.  The two handle forms give its output bitwise. */
typedef struct scann_hip_token_map scann_hip_token_map;
#define SCANN_HIP_TOKEN_TILE_BITS 65536
int scann_hip_token_map_create(scann_hip_ctx *ctx, uint64_t num_datapoints, const uint32_t *indices,
                               const uint64_t *tokens, uint64_t n_pairs, scann_hip_token_map **out);
void scann_hip_token_map_destroy(scann_hip_token_map *m);
uint64_t scann_hip_token_map_num_tokens(const scann_hip_token_map *m);
uint64_t scann_hip_token_map_num_datapoints(const scann_hip_token_map *m);
int scann_hip_token_map_get_indices(const scann_hip_token_map *m, uint64_t token, uint32_t *out, uint64_t capacity,
                                    uint64_t *out_n);
int scann_hip_token_map_allow_bitmaps_device(const scann_hip_token_map *m, const uint64_t *d_tokens,
                                             const uint64_t *d_offsets, uint32_t nq, uint64_t stride_words,
                                             uint64_t *d_out_words, void *hip_stream);
int scann_hip_token_map_allow_bitmaps(scann_hip_token_map *m, const uint64_t *tokens, const uint64_t *offsets,
                                      uint32_t nq, uint64_t stride_words, uint64_t *out_words);
int scann_hip_allow_bitmaps_from_tokens(const uint32_t *indices, const uint64_t *tokens, uint64_t n_pairs,
                                        uint64_t num_datapoints, const uint64_t *q_tokens, const uint64_t *q_offsets,
                                        uint32_t nq, uint64_t stride_words, uint64_t *out_words);
/* search_with_filter(create_allowlist(tokens of query i)) for a batch on a tree or flat-hasher handle, host pointers,
 * synchronous: queries and token lists go up, the block is built on the device by the map's kernel and
 * scann_hip_search_batched_device reads it on the same stream with nothing between the two enqueues; the rows come
 * back.  opts as for scann_hip_search_batched, with allow_bitmap NULL (set -> InvalidArgument: the lists are the
 * filter); index and map live on the same device.  Where the enqueue-only search reports Aborted or ResourceExhausted
 * (scann_hip_index_last_device_status), the batch is answered by scann_hip_search_batched under the same block.
 * Brute-force handles refuse per-query bitmaps as before (Unimplemented).  k = 0 -> InvalidArgument. */
int scann_hip_search_batched_tokens(scann_hip_index *index, scann_hip_token_map *m, const float *queries, uint32_t nq,
                                    uint32_t q_stride, uint32_t q_dim, uint32_t k, const scann_hip_search_opts *opts,
                                    const uint64_t *q_tokens, const uint64_t *q_offsets, uint32_t *out_idx,
                                    float *out_dist, uint32_t *out_count);

/* AndFilter / OrFilter / NotFilter (restricts/mod.rs:98-170) over strided bitmap blocks: the token map gives OR within
 * one attribute; "tenant X AND category in {..}" is an AND across two blocks.  Words [0, ceil(bits / 64)) of row i of
 * out = op(row i of a, row i of b); the last word is masked to `bits`, so NOT never sets a bit at or past the
 * capacity; gap words of out are not touched.  stride_a / stride_b = 0: one bitmap shared by all queries.  out may be
 * exactly a or b (same pointer, same stride).  SCANN_HIP_ALLOW_NOT does not read b (NULL is fine).  Unknown op, a
 * non-zero operand stride or an output stride below ceil(bits / 64) -> InvalidArgument.  Device form: device
 * pointers, one streaming kernel enqueued on hip_stream (16 bytes a lane where every row is 16-byte aligned), no
 * synchronisation.  Host form: host pointers, no context, no GPU; the model.  RangeFilter is the attribute table's
 * row-index column, below: a range ANDs into a block in place, with no second block and no combine pass. */
#define SCANN_HIP_ALLOW_AND 1
#define SCANN_HIP_ALLOW_OR 2
#define SCANN_HIP_ALLOW_ANDNOT 3 /* a & ~b */
#define SCANN_HIP_ALLOW_NOT 4    /* ~a */
int scann_hip_allow_bitmaps_combine(int op, const uint64_t *a, uint64_t stride_a, const uint64_t *b, uint64_t stride_b,
                                    uint32_t nq, uint64_t bits, uint64_t *out, uint64_t stride_out);
int scann_hip_allow_bitmaps_combine_device(scann_hip_ctx *ctx, int op, const uint64_t *d_a, uint64_t stride_a,
                                           const uint64_t *d_b, uint64_t stride_b, uint32_t nq, uint64_t bits,
                                           uint64_t *d_out, uint64_t stride_out, void *hip_stream);
/* ---- range filters: typed attribute columns resident on the device that write per-query bitmaps ------------------
 * RangeFilter (restricts/mod.rs:73-95) allows start <= index < end on the datapoint index.  The handle holds n_columns
 * typed columns of num_datapoints values each -- SCANN_HIP_ATTR_I64 (int64_t: timestamps, counters, ids) or
 * SCANN_HIP_ATTR_F32 (float: prices, scores) -- uploaded once and shared by every query of every batch.  The
 * pseudo-column SCANN_HIP_ATTR_ROW_INDEX needs no storage: its value at row j is j as an i64, which is the reference's
 * RangeFilter: RangeFilter::new(start, end) is lo = start, hi = (int64_t)end - 1 (end = 0 and start > end give an
 * empty bitmap; the reference's num_allowed underflows there and is not mirrored).
 *   create   n_columns = 0 is valid (only the row index), num_datapoints = 0 too (nothing but gap words is written).
 *            num_datapoints >= 2^32 - 1 -> OutOfRange; an unknown type or a null column pointer with num_datapoints >
 *            0 -> InvalidArgument.  A created table does not change (to change a value: build a new table).
 *   column_type   SCANN_HIP_ATTR_I64 / _F32, 0 for an unknown column.
 * Bitmaps of a batch: the call names n_cols <= SCANN_HIP_ATTR_MAX_CLAUSES clauses, cols[c] (a small HOST array, the
 * same for every query; a column index or SCANN_HIP_ATTR_ROW_INDEX; a column may repeat: two clauses on one column
 * intersect), and gives one inclusive range per (query, clause): bounds[(q * n_cols + c) * 2 + {0, 1}] = lo, hi (8
 * bytes each, an f32 in the low four).  Bit j of query q's bitmap -- words [q * stride_words, q * stride_words +
 * ceil(num_datapoints / 64)) -- is the AND over the clauses of lo <= value(cols[c], j) && value(cols[c], j) <= hi.
 * i64 columns compare as signed 64-bit integers, with no detour through a float type.  f32 columns compare by IEEE on
 * the stored value: -0.0 matches [0, 0], denormals are compared as stored (no flush), a NaN value matches no range (a
 * NaN attribute is "missing"), a NaN bound matches nothing, [-inf, +inf] matches every non-NaN row.  So a query that
 * does not care about a column STILL EXCLUDES that column's NaN rows if the column is among the call's clauses: leave
 * the column out of cols, or give such batches a call of their own.  lo > hi gives an empty bitmap; n_cols = 0 is the
 * empty conjunction (every bit below num_datapoints).  No bit at or past num_datapoints is ever set, under any op.
 *   op 0                     write: all nq * stride_words words are written, gap words as zero (the contract of
 *                            scann_hip_allow_bitmaps_from_ids)
 *   SCANN_HIP_ALLOW_AND      out = out & range: only words [0, ceil(bits / 64)) of each row are read and written, gap
 *   SCANN_HIP_ALLOW_OR       out = out | range     words are untouched (as scann_hip_allow_bitmaps_combine leaves
 *   SCANN_HIP_ALLOW_ANDNOT   out = out & ~range    them): a token block AND a range is one read-modify-write
 *   anything else (SCANN_HIP_ALLOW_NOT included) -> InvalidArgument.
 * Refusals come before anything is enqueued, and a refused call writes nothing: n_cols > SCANN_HIP_ATTR_MAX_CLAUSES ->
 * Unimplemented; a clause column that is neither < n_columns nor the row index, null cols / bounds / output where
 * they would be read, stride_words < ceil(bits / 64) or >= 2^32 -> InvalidArgument.
 *   _device           device pointers for bounds and output, cols on the host (read at the call); ONE kernel enqueued
 *                     on hip_stream: no clear, no global atomic, no synchronisation, nothing visits the host.
 *                     Workgroup (t, y) holds tile t (SCANN_HIP_RANGE_TILE_BITS rows) of every clause's column in
 *                     registers and writes that tile of the bitmaps of queries y, y + gridDim.y, ...
 *   (no suffix)       host pointers, synchronous: bounds up (for op != 0 the block too), the same kernel, the block
 *                     back.  One call at a time per table (serialised inside).
 *   scann_hip_allow_bitmaps_from_ranges   stateless, on the host, no context, no GPU: the model and the form for
 *                     machines without a device.  The two handle forms give its output bitwise. */
typedef struct scann_hip_attr_table scann_hip_attr_table;
typedef union { int64_t i64; float f32; uint64_t bits; } scann_hip_range_bound; /* 8 bytes; f32 in the low 4 */
#define SCANN_HIP_ATTR_I64 1
#define SCANN_HIP_ATTR_F32 2
#define SCANN_HIP_ATTR_ROW_INDEX 0xFFFFFFFFu
#define SCANN_HIP_ATTR_MAX_CLAUSES 8
#define SCANN_HIP_RANGE_TILE_BITS 1024
int scann_hip_attr_table_create(scann_hip_ctx *ctx, uint64_t num_datapoints, uint32_t n_columns, const int32_t *types,
                                const void *const *columns, scann_hip_attr_table **out);
void scann_hip_attr_table_destroy(scann_hip_attr_table *t);
uint64_t scann_hip_attr_table_num_datapoints(const scann_hip_attr_table *t);
uint32_t scann_hip_attr_table_num_columns(const scann_hip_attr_table *t);
int scann_hip_attr_table_column_type(const scann_hip_attr_table *t, uint32_t column);
int scann_hip_attr_table_allow_bitmaps_device(const scann_hip_attr_table *t, const uint32_t *cols, uint32_t n_cols,
                                              const scann_hip_range_bound *d_bounds, uint32_t nq, int op,
                                              uint64_t stride_words, uint64_t *d_out_words, void *hip_stream);
int scann_hip_attr_table_allow_bitmaps(scann_hip_attr_table *t, const uint32_t *cols, uint32_t n_cols,
                                       const scann_hip_range_bound *bounds, uint32_t nq, int op, uint64_t stride_words,
                                       uint64_t *out_words);
int scann_hip_allow_bitmaps_from_ranges(uint64_t num_datapoints, uint32_t n_columns, const int32_t *types,
                                        const void *const *columns, const uint32_t *cols, uint32_t n_cols,
                                        const scann_hip_range_bound *bounds, uint32_t nq, int op, uint64_t stride_words,
                                        uint64_t *out_words);
/* The twin of scann_hip_search_batched_tokens: host pointers, synchronous: queries and bounds go up, the block is built
 * on the device by the table's kernel (op 0) and scann_hip_search_batched_device reads it on the same stream with
 * nothing between the two enqueues; the rows come back.  opts as for scann_hip_search_batched, with allow_bitmap NULL
 * (set -> InvalidArgument: the ranges are the filter); index and table live on the same device, and the table's
 * num_datapoints equals the index's row count (else InvalidArgument).  Where the enqueue-only search reports Aborted
 * or ResourceExhausted, the batch is answered by scann_hip_search_batched under the same block.  Brute-force handles
 * refuse per-query bitmaps as before (Unimplemented).  k = 0 -> InvalidArgument. */
int scann_hip_search_batched_ranges(scann_hip_index *index, scann_hip_attr_table *t, const float *queries, uint32_t nq,
                                    uint32_t q_stride, uint32_t q_dim, uint32_t k, const scann_hip_search_opts *opts,
                                    const uint32_t *cols, uint32_t n_cols, const scann_hip_range_bound *bounds,
                                    uint32_t *out_idx, float *out_dist, uint32_t *out_count);
int scann_hip_bf_search_radius(scann_hip_index *index, const float *query, uint32_t q_dim, float radius,
                               uint32_t *out_idx, float *out_dist, uint64_t capacity,
                               uint64_t *out_count);

/* Index build helper: for every row of a brute-force index, the nearest of
 * `num_centers` centres [num_centers][dim] under the partitioner's arithmetic --
 * TreePartitioner::partition(x, 1) as used by TreeXHybridSearcher::compute_residuals
 * (tree_x_hybrid/mod.rs:212-237) and KMeans::assign_clusters (trees/kmeans.rs:352-379):
 * sequential scalar SquaredL2, lowest centre index on ties.  out_dist may be NULL.
 * NaN distances order last (the partitioner's ordered sort; assign_clusters' strict '<' never selects one).
 * A row whose EVERY distance is NaN gets centre 0 and out_dist = +inf: the two references agree on the centre
 * and disagree on the value (partition(x, 1) reports the NaN, assign_clusters keeps its initial +inf); the
 * library's value is assign_clusters'.
 * LIMIT: 16 centres are staged in LDS, each padded to a multiple of 4 values: 64 * ceil(dim / 4) * 4 bytes of
 * the workgroup's 160 KB; 8 centres where 16 do not fit (dim > 2560; the result does not depend on the tile).
 * dim > 5120 returns ResourceExhausted. */
int scann_hip_bf_assign_nearest(scann_hip_index *index, const float *centers, uint32_t num_centers,
                                uint32_t *out_assign, float *out_dist);

/* ---- mutable indexes: add, remove and update rows on a live device index (mutator/mod.rs) --------------
 * MutableDataset (mod.rs:286-490) and the rebuild counter of IncrementalUpdater (mod.rs:527-545) over a device index,
 * LSM style: an immutable BASE handle the caller created (and keeps alive: the mutable handle borrows it and must be
 * destroyed first), a live bitmap over the base rows resident on the device (one bit per base datapoint; mutations
 * flip bits with a small kernel over the batch's ids, the bitmap is never re-uploaded), and a dense, all-live DELTA
 * segment of up to `capacity` f32 rows (stride scann_hip_compute_stride(dim)) holding added and changed rows, each with
 * its external id.  Removing a delta row moves the last row into the hole (a device-to-device copy), so delta rows sit
 * in arbitrary order and nothing depends on their slots.  Wrapping a base does not modify it: searching the base
 * directly gives what it gives today.
 * Ids: u32, stable.  Base row j has id j; add returns next_index++ starting at the base size, never reused
 * (mod.rs:291); after a rebase base row j has id base_ids[j].  0xFFFFFFFF stays the empty-slot marker: when the next
 * id would be 0xFFFFFFFF, add returns OutOfRange.
 * Supported bases: f32 brute-force handles (every measure); unsharded Tree-X-Hybrid / AsymmetricHasher handles created
 * with `data` in datapoint order (data != NULL, data_is_csr_order == 0), searched with exact_reorder = 1; the live
 * bitmap covers datapoint indices below scann_hip_index_size(base), so a datapoint index at or past it counts as removed
 * once any row is removed or filtered.  Unimplemented: quantized brute-force rows, SearchMode::Partitioned, shards (leaf_sizes_global),
 * handles without rows or with rows in CSR order (at create / rebase), exact_reorder = 0 (at search: approximate and
 * exact distances cannot be merged).  capacity 0 or above SCANN_HIP_MUTABLE_MAX_CAPACITY -> InvalidArgument.
 *
 * Mutations (the reference's semantics, quirks included).  Every call takes a batch of n rows / ids -- one upload and
 * one kernel per batch; a single mutation is a batch of one.  A batch is applied in order, all or nothing: it is
 * validated on the host first, and if any element would fail the call returns that error with nothing changed (no id
 * consumed, no counter bump); the batch's staging buffers are allocated before anything changes, so ResourceExhausted
 * from the device allocator leaves the handle as it was too.  A HIP error while the batch is being copied or its kernels
 * launched (Internal) leaves the host map ahead of the device: destroy the handle.  rows: n rows of `dim` floats, row i at
 * rows + i * row_stride.
 *   add     dim != index dim -> InvalidArgument; more rows than the delta has free slots -> ResourceExhausted.
 *           Appends to the delta, out_ids[i] = the new id, counter += n.
 *   remove  an id never issued, or dropped by a rebase -> NotFound.  Removing an already removed id succeeds
 *           (mod.rs:320-329: the set absorbs it) and still counts as a mutation.  A base row has its live bit cleared,
 *           a delta row is swap-removed.
 *   update  unknown id -> NotFound, dim mismatch -> InvalidArgument.  REVIVES a removed id (mod.rs:359-360).  A live
 *           delta row is overwritten in place; a base row (live or removed) has its live bit cleared and the new row
 *           goes to the delta under the same id; a removed former delta row goes to the delta again.  A batch that
 *           needs more new delta slots than are free -> ResourceExhausted.
 *   get     copies the live row (dim floats) from wherever it lives; not live -> NotFound.  exists: 1 / 0.
 *           size: live rows.  pending: mutations since create or the last rebase; needs_rebuild(t): pending >= t.
 *
 * Search (host entry point; output conventions of scann_hip_search_batched: rows ascending, slots past out_count[i]
 * hold 0xFFFFFFFF / +inf).  out_idx holds EXTERNAL ids; opts->allow_bitmap is a host bitmap over EXTERNAL ids with the
 * capacity rule of scann_hip_search_opts (ids at or past allow_bitmap_bits are not allowed, delta ids included).
 * One stream, three stages, one synchronisation:
 *   1. base pass: the base's enqueue-only search (scann_hip_search_batched_device) under a device bitmap -- none when
 *      every base row is live and there is no user filter (today's unfiltered path, shortlist included), the resident
 *      live bitmap when rows are removed and there is no user filter, otherwise live[j] & user[id of j] from one kernel
 *      (a word-wise AND before a rebase, a gather through base_ids after).  If, after the synchronisation, the base
 *      reports Aborted or ResourceExhausted (scann_hip_index_last_device_status), the base pass is repeated through
 *      scann_hip_search_batched with the same bitmap and stages 2 and 3 run again: never partial rows.
 *   2. delta pass (delta_scan_kernel): every (query, delta row) distance by the reference's per-pair arithmetic under
 *      the measure of the base's final distances (brute force: the handle's; tree / AH: the re-rank's), queries tiled
 *      through LDS, the user bitmap tested on the external id; each workgroup sorts a tile of
 *      SCANN_HIP_MUTABLE_DELTA_TILE delta rows in LDS by (distance, EXTERNAL id) and emits its first min(k, tile).
 *   3. merge (mutable_merge_kernel): base indices mapped to external ids, the k best of base list + delta lists by
 *      (distance, external id), out_count = min(k, found).
 * With no mutation at all (empty delta, every row live, identity ids) the call IS scann_hip_search_batched on the base,
 * writing straight into the caller's arrays.
 * Contract:
 *   - brute-force base: the answer is exactly that of scann_hip_bf_create over the live rows taken in ascending
 *     external-id order, indices mapped back; distances bitwise identical; ties broken by (distance, external id);
 *     k = min(k, live allowed rows) -- whatever the mix of base and delta rows: an updated row with a low id sitting in
 *     a late delta slot still wins its ties.
 *   - tree / AH base: the base's filtered answer under the live bitmap (the one scann_hip_search_opts documents),
 *     merged with the exact distances of ALL live delta rows; delta rows are never subject to quantisation loss;
 *     pre_reorder_k applies to the base only.
 *   - a search observes every mutation whose call returned before the search was called.
 *   - mutations and searches may come from any thread; they serialise on the handle's mutex (parallel search slots are
 *     a documented limit).  create / destroy / rebase need external synchronisation against the BASE's other users
 *     only in that the base must outlive the handle.
 *   - known cost: one removed base row sends a brute-force base onto the filtered path, which never takes the
 *     bf16 shortlist (see allow_bitmap above).
 * Scratch: the partial lists take nq * ceil(delta rows / tile) * min(k, tile) * 8 bytes and stay with the handle: 1.3 MB at
 * nq = 1024, k = 10 and a 16 384-row delta, but 512 MB at nq = 1024, k >= 1024 and a full 65 536-row delta (then as large
 * as an [nq][delta] matrix of keys): split such batches.
 * Errors: q_dim != dim, k > SCANN_HIP_MUTABLE_MAX_K -> InvalidArgument; exact_reorder = 0 or per-stage outputs on a
 * tree / AH base -> Unimplemented.  k = 0 -> empty rows.
 *
 * export_live / rebase (MutableDataset::compact, mod.rs:440-471, as two calls).  export_live writes every live row
 * (rows of scann_hip_compute_stride(dim) floats, padding zero) and its id in ascending id order to host memory; base
 * rows are gathered on the device (prefix sum over the live bitmap + a gather kernel reading the base's f32 rows),
 * delta rows are placed among them by id.  *out_n = live rows; capacity_rows < live rows -> ResourceExhausted with
 * *out_n set and nothing written.  rebase swaps in a new base handle whose row j has external id base_ids[j] (strictly
 * ascending, no 0xFFFFFFFF, else InvalidArgument; NULL = identity); n must equal scann_hip_index_size(new_base), same dim
 * and kind constraints as create.  It empties the delta, sets every bit live, resets the counter and forgets every id
 * not in base_ids (NotFound afterwards); next_index is kept (raised past the largest id if need be).  The caller builds
 * new_base from the exported rows however it likes and destroys the old base afterwards.
 * scann_hip_mutable_enable_timing / _last_stage_ms: HIP-event times (ms) of { base pass, delta scan, merge } of the
 * last search on the three-stage route (0 for a stage that did not run).
 *
 * fold (MutableDataset::compact, mod.rs:440-471, in ONE call and without the rows visiting the host): builds a new
 * immutable base from the live rows ON THE DEVICE, keeping the trained model, and rebases the handle onto it.  Let the
 * live ids in ascending order be i_0 < ... < i_{n'-1}, base and delta rows alike: new datapoint j is the live row of id
 * i_j (export_live's order), out_base_ids[j] = i_j, rows are bit-copies with stride scann_hip_compute_stride(dim) and
 * zero padding, gathered on the device.
 *   - brute-force base: *out_new_base equals scann_hip_bf_create over those rows under the same measure in every
 *     observable way, shortlist copies included.
 *   - tree base: centres, codebook, use_residuals, partitions_to_search, multiplier and measure are unchanged.  A live
 *     base row keeps its leaf and its code words bit for bit (never re-assigned, never re-encoded).  A delta row gets
 *     token = TreePartitioner::partition(x, 1) with the arithmetic and tie / NaN rules of scann_hip_bf_assign_nearest
 *     (lowest centre on ties, centre 0 when no distance compares below +inf) and the code Codebook::encode(x -
 *     centre[token]) (encode(x) when use_residuals = 0; strict '<': lowest code on ties).  Leaf l holds
 *     { j : token(j) = l } in ASCENDING j: array for array what TreeXHybridSearcher::build (mod.rs:162-204) gives over
 *     the live rows with the model frozen.
 *   - flat hasher base: codes'[j] = the old code of a base row, encode(x) of a delta row.
 *   The derived structures (transposed centres, sparse-MFMA operand planes, 8-bit re-rank rows and their uniform-scale
 *   decision, the sorted leaf sizes the planner reads) are built by the code the create functions run after their
 *   upload.  Not re-trained, not re-balanced: after many folds of drifting data the caller still rebuilds.
 * Handle state: rebased onto *out_new_base inside the call (the effects of scann_hip_mutable_rebase with out_base_ids):
 * empty delta, every bit live, counter reset, next_index kept, every id keeps meaning the same row.  The caller owns
 * *out_new_base and destroys the OLD base afterwards.  out_base_ids may be NULL; with out_base_ids != NULL,
 * capacity_rows < n' -> ResourceExhausted with *out_n = n' and nothing changed.  *out_n = n' on success.
 * Preconditions of a tree base, each FailedPrecondition with the handle untouched: n_local == n_rows; every old leaf
 * strictly ascending in datapoint index (what the reference's build and trainer.py produce; checked on the device);
 * the live rows reached through the leaves number what the live bitmap counts (no datapoint in two leaves or in none).
 * No live row -> InvalidArgument ("Cannot build from empty dataset").  Any failure before the swap leaves the handle
 * exactly as it was and frees what the call allocated.  The call holds the handle's mutex: searches and mutations
 * wait.  Old and new index are resident at once: a transient 2x of the index's device memory until the caller
 * destroys the old base.
 * Device work: per SCANN_HIP_FOLD_CHUNK CSR positions one workgroup counts the surviving entries (one ballot per wave,
 * kept as a bitmap over CSR positions) and checks the ascending rule; a scan over the chunk counts and one over the
 * delta's per-leaf histogram give the new offsets; survivors and delta entries are scattered to
 * new_off[leaf] + (survivors of the leaf before) + (delta entries of the leaf before) -- the cross counts by binary
 * search, a leaf of any length being shared by as many workgroups as it has chunks; rows are gathered by export_live's
 * kernels into device memory.  Device-to-host traffic: the L + 1 new offsets with one flag word, and what the create
 * functions' second half reads.  out_base_ids comes from the host's own id tables.
 * scann_hip_fold_mutable_stage_ms: times (ms) of the last successful fold's { row gather, assign + encode of the delta
 * rows, count + scans, code / id scatter, finish half with the swap }.  The first four are HIP-event spans that hold the
 * stage's kernels and nothing else: the call allocates and uploads everything before the first event, and the
 * read-back of the offsets with its synchronisation lies between the third and the fourth span, inside none.  A span
 * still counts the launch gaps between its kernels.  The fifth is taken by the host clock.  Zeros before the first
 * fold; the three middle stages are exactly 0 for a brute-force base, which has no such kernels.
 * The two fold functions are named scann_hip_fold_mutable*, not scann_hip_mutable_fold*: they belong to this block and
 * are declared with it below. */
typedef struct scann_hip_mutable scann_hip_mutable;
#define SCANN_HIP_MUTABLE_MAX_CAPACITY 65536
#define SCANN_HIP_MUTABLE_MAX_K 2048
#define SCANN_HIP_MUTABLE_DELTA_TILE 1024
#define SCANN_HIP_FOLD_CHUNK 1024
int scann_hip_mutable_create(scann_hip_ctx *ctx, scann_hip_index *base, uint32_t capacity, scann_hip_mutable **out);
void scann_hip_mutable_destroy(scann_hip_mutable *m);
int scann_hip_mutable_add(scann_hip_mutable *m, const float *rows, uint32_t n, uint32_t row_stride, uint32_t dim,
                          uint32_t *out_ids);
int scann_hip_mutable_remove(scann_hip_mutable *m, const uint32_t *ids, uint32_t n);
int scann_hip_mutable_update(scann_hip_mutable *m, const uint32_t *ids, const float *rows, uint32_t n,
                             uint32_t row_stride, uint32_t dim);
int scann_hip_mutable_get(scann_hip_mutable *m, uint32_t id, float *out_row);
int scann_hip_mutable_exists(scann_hip_mutable *m, uint32_t id);
uint64_t scann_hip_mutable_size(scann_hip_mutable *m);
uint64_t scann_hip_mutable_pending(scann_hip_mutable *m);
int scann_hip_mutable_needs_rebuild(scann_hip_mutable *m, uint64_t threshold);
int scann_hip_mutable_search(scann_hip_mutable *m, const float *queries, uint32_t nq, uint32_t q_stride, uint32_t q_dim,
                             uint32_t k, const scann_hip_search_opts *opts, uint32_t *out_idx, float *out_dist,
                             uint32_t *out_count);
int scann_hip_mutable_export_live(scann_hip_mutable *m, float *out_rows, uint32_t *out_ids, uint64_t capacity_rows,
                                  uint64_t *out_n);
int scann_hip_mutable_rebase(scann_hip_mutable *m, scann_hip_index *new_base, const uint32_t *base_ids, uint64_t n);
void scann_hip_mutable_enable_timing(scann_hip_mutable *m, int enable);
int scann_hip_mutable_last_stage_ms(scann_hip_mutable *m, float *out_ms3);
/* fold (above): the compaction of a scann_hip_mutable handle */
int scann_hip_fold_mutable(scann_hip_mutable *m, scann_hip_index **out_new_base, uint32_t *out_base_ids,
                           uint64_t capacity_rows, uint64_t *out_n);
int scann_hip_fold_mutable_stage_ms(scann_hip_mutable *m, float *out_ms5);

/* ---- device build ----------------------------------------------------------------
 * scann_hip_txh_build: TreeXHybridSearcher::build (tree_x_hybrid/mod.rs:131-237) or, with num_partitions == 0,
 * AsymmetricHasher::build / build_no_store (hashes/hasher.rs:109-159) in one call, from the resident rows of an f32
 * brute-force handle.  No row, code, id list or assignment crosses to the host: the host reads back convergence
 * words, the leaf offsets (the planner's, as in the fold) and nothing else.  `rows` is left untouched and stays the
 * caller's; the new handle owns all its arrays (the rows are copied device to device when store_rows is set; without
 * them exact reordering returns FailedPrecondition, as after scann_hip_txh_create with data == NULL).
 *
 * THE RULE, as a function of the seeds -- every array of the new handle (centres, leaf offsets, leaf ids, codebook,
 * packed codes, rows) is bit-identical to these steps run through the public primitives:
 *   1 partitioner   k = min(num_partitions, n); scann_hip_kmeans_init_pp(k, kmeans_seed), then scann_hip_kmeans_lloyd
 *                   (kmeans_iterations, kmeans_convergence): centres and the assignment `leaf`.  The CSR lists hold
 *                   ascending datapoint index inside each leaf.  The new handle has k leaves.
 *   2 training rows in DATAPOINT order: x - centres[token(x)], token = scann_hip_bf_assign_nearest (partition(x, 1):
 *                   sequential scalar order, lowest index on ties -- not the k-means assignment, which takes the AVX2
 *                   order from simd_threshold dims on); the rows themselves when use_residuals == 0 or flat.
 *                   (scann.hpp's host build() trains on the residuals in CSR order against the k-means assignment,
 *                   another training order: its codebooks differ.)
 *   3 codebook      per subspace s: kc = min(num_codes, n) centres from scann_hip_kmeans_init_pp(seed + s) over the
 *                   column window, then scann_hip_kmeans_lloyd(training_iterations, convergence_threshold); codes
 *                   kc .. num_codes - 1 repeat centre kc - 1.
 *   4 codes         scann_hip_encode of x - centres[leaf(x)] (x itself when use_residuals == 0 or flat), stored in
 *                   CSR row order, packed 4-bit for num_codes <= 16, bytes above.
 *   5 finish        the second half of scann_hip_txh_create on the device arrays.
 * batched_codebook: 1 trains all subspaces in lockstep (one pass over the training rows per seeding round and per
 *   Lloyd iteration; a subspace that converged or reached training_iterations is frozen and skipped); 0 runs one
 *   seeding and one Lloyd loop per subspace, as the primitives do.  Both give the same bits.  The batched kernels
 *   take the sequential scalar order only: with dims_per_subspace >= simd_threshold (the AVX2 order), or
 *   n * num_subspaces >= 2^31, the per-subspace route is taken whatever the flag says.
 * REFUSED before any training launch: `rows` not an f32 brute-force handle (quantized rows: InvalidArgument), n == 0
 *   or dim % num_subspaces != 0 (InvalidArgument), the (num_subspaces, num_codes) shapes, the leaf ceiling and the
 *   measures scann_hip_txh_create refuses (same status), dimensions past the k-means LDS limit (dim > 5120 for a tree,
 *   dims_per_subspace > 5120 flat: ResourceExhausted), n >= 2^31 (OutOfRange).
 * out_report (may be NULL): the partitioner's and every subspace's iteration count and converged flag as
 *   scann_hip_kmeans_lloyd reports them, and stage_ms, host-clock milliseconds of: partition seeding, partition Lloyd,
 *   CSR + residuals, codebook seeding, codebook Lloyd, encode + pack, finish half. */
typedef struct scann_hip_build_config {
    uint32_t num_partitions;          /* 0 = AsymmetricHasher::build (flat), else TreeXHybridSearcher::build */
    uint32_t kmeans_iterations;       /* 100  (tree_partitioner.rs:72) */
    double   kmeans_convergence;      /* 1e-5 */
    uint64_t kmeans_seed;             /* 42 */
    uint32_t num_subspaces, num_codes;
    uint32_t training_iterations;     /* 25   (CodebookConfig.max_iterations) */
    double   convergence_threshold;   /* 1e-5 */
    uint64_t seed;                    /* 42; subspace s trains with seed + s (codebook.rs:177-199) */
    uint32_t simd_threshold;          /* 128  (KMeansConfig.simd_threshold) */
    int32_t  use_residuals;           /* 1 */
    int32_t  store_rows;              /* 1; 0 = build_no_store (hasher.rs:137-159) */
    int32_t  batched_codebook;        /* 1; 0 = one Lloyd loop per subspace, as the primitives run it */
    uint32_t partitions_to_search; float pre_reorder_multiplier; int32_t distance_measure;
} scann_hip_build_config;

typedef struct scann_hip_build_report {
    uint32_t partition_iterations; int32_t partition_converged; double partition_inertia;
    uint32_t subspace_iterations[64]; int32_t subspace_converged[64];
    float stage_ms[7];
} scann_hip_build_report;

/* the defaults noted above, partitions_to_search 10, pre_reorder_multiplier 3 (TreeXHybridConfig), SquaredL2;
 * num_partitions, num_subspaces and num_codes are left 0: the caller sets them */
void scann_hip_build_config_default(scann_hip_build_config *cfg);
int scann_hip_txh_build(scann_hip_index *rows, const scann_hip_build_config *cfg, scann_hip_index **out_index,
                        scann_hip_build_report *out_report);

/* ---- hierarchical device build ------------------------------------------------------
 * scann_hip_txh_build_hierarchical: scann_hip_txh_build with the partitioner of TreePartitioner::build_hierarchical
 * (partitioning/tree_partitioner.rs:101-140) -- a KMeansTree (trees/kmeans_tree.rs:183-284) built on the device and
 * flattened to its leaves.  The result is an ordinary tree handle whose partitions are the tree's leaves and whose
 * centres are the leaves' means: search, filters, fold and index files treat it like any other; the tree itself is not
 * kept.  A tree of depth 2 with c children per node scores every row against 2 c centres per iteration for up to c^2
 * leaves, where the flat partitioner scores it against all c^2.
 * COMPOSITION: the reference has build_hierarchical but no searcher of it calls it; feeding the flattened
 * leaves to steps 2-5 of scann_hip_txh_build is this project's own composition.
 * Of `cfg`, num_partitions, kmeans_iterations, kmeans_convergence and kmeans_seed are IGNORED: `tree` replaces them.
 * Every other field means what it means to scann_hip_txh_build (simd_threshold also governs the tree's k-means).
 *
 * THE RULE, as a function of the seeds -- every array of the new handle is bit-identical to these steps run through
 * the public primitives:
 *   1 tree          build_node (kmeans_tree.rs:212-267) over nodes whose members are ascending datapoint indices; the
 *                   root holds every row at depth 0.  A node at depth d with n_node members is a LEAF when
 *                   d >= max_depth, n_node <= min_leaf_size or n_node <= num_children.  Any other node trains
 *                   k = min(num_children, n_node) = num_children centres exactly as the two primitives run, in this
 *                   order, on a brute-force handle that holds the node's rows alone (member t = row t):
 *                   scann_hip_kmeans_init_pp(k, seed + d, cfg->simd_threshold), then scann_hip_kmeans_lloyd
 *                   (kmeans_iterations, kmeans_convergence, cfg->simd_threshold) -- so an empty cluster c takes the
 *                   node's member c % n_node, and every node of a level draws from the same stream.  Its children are
 *                   the NON-EMPTY clusters of the final assignment, in cluster order, each with its members ascending;
 *                   a node with exactly one non-empty cluster is a leaf.  Leaves are numbered depth first, children in
 *                   order (collect_leaves).  The centre of a leaf is compute_center (:270-284): per dimension the f64
 *                   sum of its members in ascending order, divided by the count, cast to f32 -- the arithmetic of the
 *                   Lloyd loop's centre update applied to the FINAL assignment, not the loop's last centres.  The CSR
 *                   lists hold ascending datapoint index inside each leaf.
 *   2-5             steps 2-5 of scann_hip_txh_build on those centres and that leaf assignment: training rows in
 *                   datapoint order against scann_hip_bf_assign_nearest of the flattened centres, codebook, codes in
 *                   CSR order, finish.
 * All nodes of one level train in lockstep: the number of kernel launches per seeding round and per Lloyd iteration does
 * not depend on the number of nodes.  A node that converged is frozen and skipped.  Rows are gathered through the
 * level's permutation, never copied into level order.  The host keeps the level's node table: it reads the per-node
 * stop records once per iteration and the cluster offsets once per level; no row, distance or assignment visits it.
 * Extra device memory during the tree stage, released before step 2: n * dim * 4 bytes (member-ordered rows of the
 * centre update, as scann_hip_kmeans_lloyd holds) and 9 arrays of n * 4 bytes, plus num_children * dim * 4 bytes per
 * training node of a level.
 * REFUSED before any training launch (`rows` keeps searching): everything scann_hip_txh_build refuses, with the same
 *   status (the leaf ceiling aside); num_children == 0 -> InvalidArgument; max_depth > 4 -> Unimplemented.
 *   max_depth == 0, or n <= num_children or n <= min_leaf_size at the root: a single leaf holding every row.
 *   More than 16384 leaves (the search's num_partitions ceiling) is known only during the tree stage: Unimplemented
 *   with the node count in the message, as soon as a level has more than 16384 nodes; no handle is returned.
 * out_report (may be NULL): as scann_hip_txh_build's; the partition_* slots hold the ROOT's k-means (zeros when the root
 *   is a leaf), stage_ms[0] and [1] the seeding and the Lloyd time of the whole tree stage.
 * out_tree_report (may be NULL): per level d = 0..4, level_nodes = the nodes that ran k-means at depth d,
 *   level_iterations = the sum of their iteration counts, level_converged = how many converged, level_leaves = the leaves
 *   of depth d; stage_ms[2 d] and [2 d + 1] = host-clock milliseconds of level d's seeding and of its Lloyd loop with
 *   the children's layout. */
typedef struct scann_hip_tree_config {   /* KMeansTreeConfig, kmeans_tree.rs:20-55 */
    uint32_t num_children;        /* 100 */
    uint32_t max_depth;           /* 1 = flat */
    uint32_t min_leaf_size;       /* 1 */
    uint32_t kmeans_iterations;   /* 100 */
    double   kmeans_convergence;  /* 1e-5 */
    uint64_t seed;                /* 42; a node at depth d trains with seed + d (kmeans_tree.rs:235) */
} scann_hip_tree_config;

typedef struct scann_hip_tree_report {
    uint32_t num_leaves, depth_reached;
    uint32_t level_nodes[5], level_iterations[5], level_converged[5], level_leaves[5];
    float stage_ms[10];
} scann_hip_tree_report;

void scann_hip_tree_config_default(scann_hip_tree_config *tree);
int scann_hip_txh_build_hierarchical(scann_hip_index *rows, const scann_hip_tree_config *tree,
                                     const scann_hip_build_config *cfg, scann_hip_index **out_index,
                                     scann_hip_build_report *out_report, scann_hip_tree_report *out_tree_report);

/* ---- PCA training on the device (PcaProjection::train, projection/pca.rs:71-129, utils/linear_algebra.rs:89-120) ----
 * Trains a SCANN_HIP_PROJ_PCA projection from the resident rows of an f32 brute-force handle (in_dim = its dim); no row
 * crosses to the host.  The object is indistinguishable from one scann_hip_projection_create makes from the same
 * arrays.  THE RULE is the project's own (the reference's shuffle and nalgebra SVD are not reproducible: SURVEY F2, F4,
 * F10), the one trainer.pca_projection states:
 *   1 sample      max_samples == 0 or >= n: every row, in order.  Otherwise ns = max_samples rows, row t =
 *                 splitmix64(seed ^ 0x9CA, 0, ns)[t] % n: with replacement, counter based, computed on the device.
 *   2 mean        per column in f64, in a fixed order that depends on ns alone (at most 1024 runs of consecutive sample
 *                 positions, each summed ascending, the runs added ascending); no floating-point atomics.  The
 *                 projection's mean is its rounding to f32.
 *   3 covariance  C = sum (x - mean64)(x - mean64)^T / max(1, ns - 1): rows widened to f64 and centred with the
 *                 UNROUNDED f64 mean before the product; two passes, never E[xx^T] - mu mu^T.  Elements between dim and
 *                 stride are never read.  Computed on v_mfma_f64_16x16x4_f64, upper-triangle tiles only and mirrored,
 *                 split over row runs into a workspace of at most 128 MiB and reduced in ascending run order.
 *   4 eigen-solve cyclic Jacobi on C, in f64, on the device: a fixed round-robin pairing (d - 1 rounds of floor(d / 2)
 *                 disjoint rotations, a bye for odd d), one kernel per round, so the result is a function of C alone.
 *                 Converged when the Frobenius norm of the strict off-diagonal, summed from the off-diagonal entries
 *                 themselves, is <= 2^-46 ||C||_F.  At most 30 sweeps; out_sweeps and out_converged report the count
 *                 and the outcome; an unconverged solve still returns its result, with *out_converged = 0.
 *   5 components  eigenvalues descending (ties: lower original column first); each component's sign makes its
 *                 largest-magnitude entry positive (ties: lowest index); cast to f32; matrix [out_dim][in_dim].
 * Only the matrix, the mean and the optional outputs are read back: out_eigenvalues [in_dim] (all of them, sorted),
 * out_covariance [in_dim][in_dim] (before the solve), each may be NULL, as may out_sweeps and out_converged.
 * Device memory while training, released on return (d = in_dim, m = d rounded up to even): ns * 4 bytes of sample
 * indices when sampling, 1024 * d * 8 of mean runs, at most 128 MiB of covariance runs, 3 * m * m * 8 for the solve.
 * REFUSED before any launch (`rows` keeps searching): not an f32 brute-force handle (a quantized, tree or hasher
 * handle), n == 0, out_dim == 0 or > in_dim -> InvalidArgument; in_dim > 2048 -> ResourceExhausted, the message naming
 * the limit (the solve is O(d^3) per sweep). */
int scann_hip_pca_train(scann_hip_index *rows, uint32_t out_dim, uint64_t max_samples, uint64_t seed,
                        scann_hip_projection **out_projection, double *out_eigenvalues, double *out_covariance,
                        uint32_t *out_sweeps, int *out_converged);
/* The arrays of a projection object, any kind: out_matrix [out_dim][in_dim] (not written for TRUNCATE), out_mean
 * [in_dim] (written for PCA only); each may be NULL. */
int scann_hip_projection_arrays(const scann_hip_projection *projection, float *out_matrix, float *out_mean);
/* Host-clock milliseconds of the calling thread's last scann_hip_pca_train: sample + mean, covariance, eigen-solve,
 * components + read-back. */
void scann_hip_pca_last_stage_ms(float *out_ms4);

/* ---- projected device build ---------------------------------------------------------
 * scann_hip_txh_build for a PROJECTED index, in one call: `rows` is an f32 brute-force handle of projection.in_dim
 * floats per row, `projection` any kind (PCA from scann_hip_pca_train, a caller's MATRIX or TRUNCATE).  THE RULE: every
 * array of the new handle is bit-identical to, and its searches are those of, this chain through the public entry points:
 *   1 scann_hip_project_device of the rows into [n][out_dim];
 *   2 scann_hip_bf_create of those rows at stride out_dim;
 *   3 scann_hip_txh_build(cfg with store_rows = 0);
 *   4 scann_hip_txh_create_projected from the built arrays, with the original rows, or none when cfg->store_rows == 0.
 * No code, id list, assignment or row visits the host; the projection is copied into the handle (the caller may destroy
 * it) and the original rows are copied device to device.  Extra device memory during the call, beyond
 * scann_hip_txh_build's: n * out_dim * 4 bytes for the projected rows, released before the handle is assembled.
 * out_report: as scann_hip_txh_build's, all seven stage_ms slots; the projection pass is added to stage_ms[0].
 * The handle writes and reloads through the proj_* file sections like any projected handle.
 * REFUSED before any launch: everything scann_hip_txh_build refuses, judged on out_dim (dim % num_subspaces, the k-means
 * LDS limit, ...); a NULL projection and rows whose dim is not projection.in_dim -> InvalidArgument. */
int scann_hip_txh_build_projected(scann_hip_index *rows, const scann_hip_projection *projection,
                                  const scann_hip_build_config *cfg, scann_hip_index **out_index,
                                  scann_hip_build_report *out_report);

/* ---- introspection ------------------------------------------------------------- */
uint64_t scann_hip_index_size(const scann_hip_index *index);          /* Searcher::dataset_size */
uint32_t scann_hip_index_dimensionality(const scann_hip_index *index);/* Searcher::dimensionality */
/* Bytes of the handle's persistent device allocations, any handle kind: rows (f32 or quantized), the 8-bit and bf16
 * shadow stores and their per-row data, codes, sparse operand planes, ids, leaf tables, centres, codebook, attached
 * crowding attributes.  Search workspaces are not counted.  NULL -> 0. */
uint64_t scann_hip_index_device_bytes(const scann_hip_index *index);
void scann_hip_index_destroy(scann_hip_index *index);

/* Kernel timing hook for bench.py: mean HIP-event time (ms) of the dominant kernel over
 * the search launches issued on `index` since timing was enabled (ring of 64 event pairs
 * recorded on the stream each kernel was launched on; 0 if timing is off).  Enabling
 * resets the ring; reading synchronises on the recorded events. */
void scann_hip_index_enable_timing(scann_hip_index *index, int enable);
float scann_hip_index_last_kernel_ms(scann_hip_index *index, const char **out_kernel_name);

#ifdef __cplusplus
}
#endif
#endif

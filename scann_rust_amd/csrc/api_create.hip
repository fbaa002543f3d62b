// api_create.hip -- C ABI, creation of index handles: brute-force and tree / hasher handles from host arrays, quantized
// and projected ones, the handles a fold or a device build ends in, PCA training.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "build.h"
#include "handle.h"
#include "index_arrays.h"
#include "ktree.h"
#include "launch.h"
#include "mutable.h"
#include "pca.h"
#include "scalarq.h"

using namespace scann;

static int index_common_init(scann_hip_index *ix);
static int bf_finish(scann_hip_index *ix, uint64_t n, uint32_t dim, uint32_t stride, int measure);
static int bf_finish_quantized(scann_hip_index *ix, uint64_t n, uint32_t dim, uint32_t stride, int row_format,
                               float inv_multiplier, int measure);
static int txh_finish(scann_hip_index *ix, const scann_hip_txh_desc *d, const std::vector<uint32_t> &off);

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

static int index_common_init(scann_hip_index *ix) {
    SCANN_HIP_CHECK(hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking));
    for (int i = 0; i < scann_hip_index::kEvRing; ++i) {
        SCANN_HIP_CHECK(hipEventCreate(&ix->evs[i][0]));
        SCANN_HIP_CHECK(hipEventCreate(&ix->evs[i][1]));
    }
    return SCANN_HIP_OK;
}

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

// =====================================================================================
// Tree-X-Hybrid / AsymmetricHasher index
// =====================================================================================

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

// ---- projected handles (project.h) ------------------------------------------------------------------

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

int scann_hip_txh_create(scann_hip_ctx *ctx, const scann_hip_txh_desc *d, scann_hip_index **out) {
    return scann::txh_create_checked(ctx, d, out, SCANN_HIP_INVALID_ARGUMENT);
}

int scann_hip_txh_create_quantized(scann_hip_ctx *ctx, const scann_hip_txh_desc *d, const void *rows, int row_format,
                                   float inv_multiplier, scann_hip_index **out) {
    if (!ctx || !d || !out) return fail(SCANN_HIP_INVALID_ARGUMENT, "null ctx/desc/out_index");
    SCANN_TRY(scann::txh_quantized_args(d, rows, row_format, inv_multiplier));
    return scann::txh_create_checked(ctx, d, out, SCANN_HIP_INVALID_ARGUMENT, rows, row_format, inv_multiplier);
}

int scann_hip_txh_create_projected(scann_hip_ctx *ctx, const scann_hip_txh_desc *d, const scann_hip_projection *proj,
                                   const float *rows, uint64_t n_rows, uint32_t row_dim, uint32_t row_stride,
                                   scann_hip_index **out) {
    return scann::txh_create_projected_checked(ctx, d, proj, rows, n_rows, row_dim, row_stride, out, SCANN_HIP_INVALID_ARGUMENT);
}

int scann_hip_index_projection_info(const scann_hip_index *ix, uint32_t *out4) {
    if (!ix || !out4) return fail(SCANN_HIP_INVALID_ARGUMENT, "null index/output");
    out4[0] = (uint32_t)ix->proj.kind;
    out4[1] = ix->proj.in_dim;
    out4[2] = ix->proj.out_dim;
    out4[3] = ix->proj.start;
    return SCANN_HIP_OK;
}

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

void scann_hip_tree_config_default(scann_hip_tree_config *c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->num_children = 100;            // KMeansTreeConfig::default (kmeans_tree.rs:42-55)
    c->max_depth = 1;
    c->min_leaf_size = 1;
    c->kmeans_iterations = 100;
    c->kmeans_convergence = 1e-5;
    c->seed = 42;
}

int scann_hip_txh_build_hierarchical(scann_hip_index *rows, const scann_hip_tree_config *tree,
                                     const scann_hip_build_config *cfg, scann_hip_index **out_index,
                                     scann_hip_build_report *out_report, scann_hip_tree_report *out_tree_report) {
    if (!rows || !tree || !cfg || !out_index) return fail(SCANN_HIP_INVALID_ARGUMENT, "null rows/tree/config/out_index");
    *out_index = nullptr;
    if (out_report) std::memset(out_report, 0, sizeof(*out_report));
    if (out_tree_report) std::memset(out_tree_report, 0, sizeof(*out_tree_report));
    if (rows->kind != KIND_BF) return fail(SCANN_HIP_INVALID_ARGUMENT, "not a brute-force index");
    std::lock_guard<std::mutex> lock(rows->mu);
    SCANN_TRY(set_device(rows->ctx));
    scann_hip_build_config c = *cfg;   // the tree configuration replaces the flat partitioner's four fields
    c.num_partitions = 1;              // "a tree"; the number of leaves is known after the tree stage
    c.kmeans_iterations = tree->kmeans_iterations;
    c.kmeans_convergence = tree->kmeans_convergence;
    c.kmeans_seed = tree->seed;
    SCANN_TRY(build_check(rows->bf, c));   // every refusal of scann_hip_txh_build, before the first training launch
    SCANN_TRY(ktree_check(*tree));
    BuildParts parts;
    SCANN_TRY(build_txh_hierarchical_device(rows->bf, *tree, c, rows->stream, &parts, out_report, out_tree_report));
    c.num_partitions = parts.L;
    return index_build_txh(rows, c, parts, out_index, out_report);
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

}  // extern "C"

// index_file.hip -- the on-disk index container (include/scann_hip.h "index files"): writer,
// header inspection, and the mmap -> (pinned) -> device loader.  Host code only.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "index_arrays.h"
#include "knobs.h"
#include "launch.h"

namespace {

using scann::fail;

constexpr char kMagic[8] = {'S', 'C', 'A', 'N', 'N', 'I', 'D', 'X'};
constexpr uint32_t kVersion = 1;
constexpr uint64_t kAlign = 4096;
enum { DT_F32 = 0, DT_U32 = 1, DT_U8 = 2 };

struct FileHeader {   // 256 bytes, little-endian, no implicit padding
    char magic[8];
    uint32_t version, kind;
    uint64_t n_rows, n_local, file_bytes;
    uint32_t dim, stride, num_partitions, num_subspaces, num_codes, dims_per_subspace;
    int32_t distance_measure, data_is_csr_order, codes_packed4, use_residuals;
    uint32_t partitions_to_search;
    float pre_reorder_multiplier;
    uint32_t n_sections;
    uint32_t reserved[41];
};
static_assert(sizeof(FileHeader) == 256, "header layout");

struct FileSection {  // 64 bytes
    char name[24];
    uint32_t dtype, reserved0;
    uint64_t offset, nbytes;
    uint64_t reserved1[2];
};
static_assert(sizeof(FileSection) == 64, "section layout");

struct PendingSection {
    const char *name;
    uint32_t dtype;
    const void *ptr;
    uint64_t nbytes;
};

int write_container(const char *path, FileHeader h, const std::vector<PendingSection> &secs) {
    std::vector<FileSection> table(secs.size());
    uint64_t off = sizeof(FileHeader) + sizeof(FileSection) * secs.size();
    for (size_t i = 0; i < secs.size(); ++i) {
        off = (off + kAlign - 1) / kAlign * kAlign;
        std::memset(&table[i], 0, sizeof(FileSection));
        std::strncpy(table[i].name, secs[i].name, sizeof(table[i].name) - 1);
        table[i].dtype = secs[i].dtype;
        table[i].offset = off;
        table[i].nbytes = secs[i].nbytes;
        off += secs[i].nbytes;
    }
    h.n_sections = (uint32_t)secs.size();
    h.file_bytes = off;
    FILE *f = std::fopen(path, "wb");
    if (!f) return fail(errno == EACCES ? SCANN_HIP_PERMISSION_DENIED : SCANN_HIP_NOT_FOUND,
                        std::string("cannot create ") + path + ": " + std::strerror(errno));
    bool ok = std::fwrite(&h, sizeof(h), 1, f) == 1;
    if (ok && !table.empty()) ok = std::fwrite(table.data(), sizeof(FileSection), table.size(), f) == table.size();
    uint64_t pos = sizeof(FileHeader) + sizeof(FileSection) * secs.size();
    static const char zeros[4096] = {0};
    for (size_t i = 0; ok && i < secs.size(); ++i) {
        while (ok && pos < table[i].offset) {
            const size_t pad = (size_t)std::min<uint64_t>(sizeof(zeros), table[i].offset - pos);
            ok = std::fwrite(zeros, 1, pad, f) == pad;
            pos += pad;
        }
        if (ok && secs[i].nbytes) ok = std::fwrite(secs[i].ptr, 1, secs[i].nbytes, f) == secs[i].nbytes;
        pos += secs[i].nbytes;
    }
    if (std::fclose(f) != 0) ok = false;
    if (!ok) {
        std::remove(path);
        return fail(SCANN_HIP_DATA_LOSS, std::string("short write to ") + path);
    }
    return SCANN_HIP_OK;
}

FileHeader blank_header(uint32_t kind) {
    FileHeader h;
    std::memset(&h, 0, sizeof(h));
    std::memcpy(h.magic, kMagic, 8);
    h.version = kVersion;
    h.kind = kind;
    return h;
}

// a read-only mapping of a validated file
struct Mapping {
    void *base = MAP_FAILED;
    size_t bytes = 0;
    bool pinned = false;
    ~Mapping() {
        if (pinned) (void)hipHostUnregister(base);
        if (base != MAP_FAILED) munmap(base, bytes);
    }
    const FileHeader &header() const { return *static_cast<const FileHeader *>(base); }
    const FileSection *find(const char *name) const {
        const FileSection *t = reinterpret_cast<const FileSection *>(static_cast<const char *>(base) + sizeof(FileHeader));
        for (uint32_t i = 0; i < header().n_sections; ++i)
            if (std::strncmp(t[i].name, name, sizeof(t[i].name)) == 0) return &t[i];
        return nullptr;
    }
    const void *data(const FileSection *s) const { return s ? static_cast<const char *>(base) + s->offset : nullptr; }
};

int open_mapping(const char *path, Mapping *m) {
    if (!path) return fail(SCANN_HIP_INVALID_ARGUMENT, "path is null");
    const int fd = open(path, O_RDONLY);
    if (fd < 0)
        return fail(errno == EACCES ? SCANN_HIP_PERMISSION_DENIED : SCANN_HIP_NOT_FOUND,
                    std::string("cannot open ") + path + ": " + std::strerror(errno));
    struct stat st;
    if (fstat(fd, &st) != 0) {
        close(fd);
        return fail(SCANN_HIP_INTERNAL, std::string("fstat failed on ") + path);
    }
    if ((uint64_t)st.st_size < sizeof(FileHeader)) {
        close(fd);
        return fail(SCANN_HIP_DATA_LOSS, std::string(path) + ": shorter than an index header");
    }
    m->bytes = (size_t)st.st_size;
    m->base = mmap(nullptr, m->bytes, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (m->base == MAP_FAILED) return fail(SCANN_HIP_RESOURCE_EXHAUSTED, std::string("mmap failed on ") + path);
    const FileHeader &h = m->header();
    if (std::memcmp(h.magic, kMagic, 8) != 0)
        return fail(SCANN_HIP_INVALID_ARGUMENT, std::string(path) + ": not a SCANNIDX file");
    if (h.version != kVersion)
        return fail(SCANN_HIP_INVALID_ARGUMENT,
                    std::string(path) + ": unsupported index file version " + std::to_string(h.version));
    if (h.file_bytes != (uint64_t)st.st_size)
        return fail(SCANN_HIP_DATA_LOSS, std::string(path) + ": file is " + std::to_string(st.st_size) +
                                             " bytes, header says " + std::to_string(h.file_bytes));
    if (h.kind > 1 || h.n_sections > 64 ||
        sizeof(FileHeader) + (uint64_t)h.n_sections * sizeof(FileSection) > (uint64_t)st.st_size)
        return fail(SCANN_HIP_DATA_LOSS, std::string(path) + ": corrupt header");
    const FileSection *t = reinterpret_cast<const FileSection *>(static_cast<const char *>(m->base) + sizeof(FileHeader));
    for (uint32_t i = 0; i < h.n_sections; ++i)
        if (t[i].offset % kAlign != 0 || t[i].offset > h.file_bytes || t[i].nbytes > h.file_bytes - t[i].offset)
            return fail(SCANN_HIP_DATA_LOSS, std::string(path) + ": section table out of bounds");
    return SCANN_HIP_OK;
}

// a * b * c, or UINT64_MAX (which no section of a validated file can have) on overflow
uint64_t bytes3(uint64_t a, uint64_t b, uint64_t c) {
    uint64_t ab, abc;
    if (__builtin_mul_overflow(a, b, &ab) || __builtin_mul_overflow(ab, c, &abc)) return ~0ull;
    return abc;
}

// section `name` must exist with exactly `want` bytes (or be absent when !required)
int section(const Mapping &m, const char *path, const char *name, uint64_t want, bool required,
            const void **out) {
    const FileSection *s = m.find(name);
    *out = nullptr;
    if (!s) {
        if (required) return fail(SCANN_HIP_DATA_LOSS, std::string(path) + ": section '" + name + "' is missing");
        return SCANN_HIP_OK;
    }
    if (s->nbytes != want)
        return fail(SCANN_HIP_DATA_LOSS, std::string(path) + ": section '" + name + "' has " +
                                             std::to_string(s->nbytes) + " bytes, expected " + std::to_string(want));
    *out = m.data(s);
    return SCANN_HIP_OK;
}

// The projection of a projected handle and its rows, as write_txh stores them: `proj_meta` (u32: kind, in_dim, out_dim,
// start, row_stride), `proj_matrix` (f32 [out_dim][in_dim]; MATRIX, PCA), `proj_mean` (f32 [in_dim]; PCA), and `data` =
// the original rows, row_stride floats apart (the header's dim / stride keep describing the index space).
struct ProjSections {
    const uint32_t *meta = nullptr;   // [5]
    const float *matrix = nullptr, *mean = nullptr, *rows = nullptr;
};

// scann_hip_txh_write_file, and with rows_q != nullptr the file of a handle over quantized rows: no `data` section,
// the rows' bytes in `rows_q`, {format, inv_multiplier bits} in `rows_q_meta`; with pj != nullptr a projected handle's
int write_txh(const char *path, const scann_hip_txh_desc *d, const void *rows_q, uint64_t rows_q_bytes, int rows_q_fmt,
              float rows_q_inv, const ProjSections *pj = nullptr) {
    if (!path || !d) return fail(SCANN_HIP_INVALID_ARGUMENT, "path/desc is null");
    const bool ah = d->num_partitions == 0;
    const bool exact = !d->codebook && !d->codes && d->num_subspaces == 0;
    if (d->n_local == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "Cannot build from empty dataset");
    if (!exact && (!d->codebook || !d->codes)) return fail(SCANN_HIP_INVALID_ARGUMENT, "codebook/codes null");
    if (!ah && (!d->centers || !d->leaf_offsets || !d->leaf_ids))
        return fail(SCANN_HIP_INVALID_ARGUMENT, "centers/leaf_offsets/leaf_ids null");
    FileHeader h = blank_header(1);
    h.n_rows = d->n_rows;
    h.n_local = d->n_local;
    h.dim = d->dim;
    h.stride = d->stride;
    h.num_partitions = d->num_partitions;
    h.num_subspaces = d->num_subspaces;
    h.num_codes = d->num_codes;
    h.dims_per_subspace = d->dims_per_subspace;
    h.distance_measure = d->distance_measure;
    h.data_is_csr_order = d->data_is_csr_order;
    h.codes_packed4 = d->codes_packed4;
    h.use_residuals = d->use_residuals;
    h.partitions_to_search = d->partitions_to_search;
    h.pre_reorder_multiplier = d->pre_reorder_multiplier;
    std::vector<PendingSection> secs;
    if (d->data) secs.push_back({"data", DT_F32, d->data, (uint64_t)d->n_rows * d->stride * 4});
    if (pj) {
        const uint64_t in_dim = pj->meta[1], out_dim = pj->meta[2];
        if (pj->rows) secs.push_back({"data", DT_F32, pj->rows, (uint64_t)d->n_rows * pj->meta[4] * 4});
        secs.push_back({"proj_meta", DT_U32, pj->meta, 5 * 4});
        if (pj->matrix) secs.push_back({"proj_matrix", DT_F32, pj->matrix, out_dim * in_dim * 4});
        if (pj->mean) secs.push_back({"proj_mean", DT_F32, pj->mean, in_dim * 4});
    }
    uint32_t q_meta[2] = {(uint32_t)rows_q_fmt, 0u};
    std::memcpy(&q_meta[1], &rows_q_inv, 4);
    if (rows_q) {
        secs.push_back({"rows_q", DT_U8, rows_q, rows_q_bytes});
        secs.push_back({"rows_q_meta", DT_U32, q_meta, sizeof(q_meta)});
    }
    if (!ah) {
        secs.push_back({"centers", DT_F32, d->centers, (uint64_t)d->num_partitions * d->dim * 4});
        secs.push_back({"leaf_offsets", DT_U32, d->leaf_offsets, ((uint64_t)d->num_partitions + 1) * 4});
        secs.push_back({"leaf_ids", DT_U32, d->leaf_ids, d->n_local * 4});
        if (d->leaf_sizes_global)
            secs.push_back({"leaf_sizes_global", DT_U32, d->leaf_sizes_global, (uint64_t)d->num_partitions * 4});
    }
    if (!exact) {
        const uint64_t bpp = d->codes_packed4 ? (d->num_subspaces + 1) / 2 : d->num_subspaces;
        secs.push_back({"codebook", DT_F32, d->codebook,
                        (uint64_t)d->num_subspaces * d->num_codes * d->dims_per_subspace * 4});
        secs.push_back({"codes", DT_U8, d->codes, d->n_local * bpp});
    }
    return write_container(path, h, secs);
}

}  // namespace

extern "C" {

int scann_hip_txh_write_file(const char *path, const scann_hip_txh_desc *d) {
    return write_txh(path, d, nullptr, 0, 0, 1.0f);
}

int scann_hip_bf_write_file(const char *path, const float *data, uint64_t n, uint32_t dim, uint32_t stride,
                            int measure) {
    if (!path || (n && !data)) return fail(SCANN_HIP_INVALID_ARGUMENT, "path/data is null");
    if (stride < dim) return fail(SCANN_HIP_INVALID_ARGUMENT, "stride < dim");
    FileHeader h = blank_header(0);
    h.n_rows = n;
    h.n_local = n;
    h.dim = dim;
    h.stride = stride;
    h.distance_measure = measure;
    std::vector<PendingSection> secs;
    secs.push_back({"data", DT_F32, data, n * stride * 4});
    return write_container(path, h, secs);
}

int scann_hip_index_write_file(const scann_hip_index *index, const char *path) {
    if (!index || !path) return fail(SCANN_HIP_INVALID_ARGUMENT, "index/path is null");
    scann::IndexHostArrays a;
    SCANN_TRY(scann::index_download(index, &a));
    if (a.brute_force)
        return scann_hip_bf_write_file(path, a.d.data, a.d.n_rows, a.d.dim, a.d.stride, a.d.distance_measure);
    if (a.rows_q_fmt) return write_txh(path, &a.d, a.rows_q.data(), a.rows_q.size(), a.rows_q_fmt, a.rows_q_inv);
    if (a.proj_meta[0]) {
        ProjSections pj;
        pj.meta = a.proj_meta;
        pj.matrix = a.proj_matrix.empty() ? nullptr : a.proj_matrix.data();
        pj.mean = a.proj_mean.empty() ? nullptr : a.proj_mean.data();
        pj.rows = a.data.empty() ? nullptr : a.data.data();
        return write_txh(path, &a.d, nullptr, 0, 0, 1.0f, &pj);
    }
    return scann_hip_txh_write_file(path, &a.d);
}

int scann_hip_index_file_info(const char *path, scann_hip_file_info *out) {
    if (!out) return fail(SCANN_HIP_INVALID_ARGUMENT, "out_info is null");
    Mapping m;
    SCANN_TRY(open_mapping(path, &m));
    const FileHeader &h = m.header();
    std::memset(out, 0, sizeof(*out));
    out->version = h.version;
    out->kind = h.kind;
    out->n_rows = h.n_rows;
    out->n_local = h.n_local;
    out->file_bytes = h.file_bytes;
    out->dim = h.dim;
    out->stride = h.stride;
    out->num_partitions = h.num_partitions;
    out->num_subspaces = h.num_subspaces;
    out->num_codes = h.num_codes;
    out->dims_per_subspace = h.dims_per_subspace;
    out->distance_measure = h.distance_measure;
    out->data_is_csr_order = h.data_is_csr_order;
    out->codes_packed4 = h.codes_packed4;
    out->use_residuals = h.use_residuals;
    out->partitions_to_search = h.partitions_to_search;
    out->pre_reorder_multiplier = h.pre_reorder_multiplier;
    out->has_data = m.find("data") ? 1 : 0;
    return SCANN_HIP_OK;
}

int scann_hip_index_load_file(scann_hip_ctx *ctx, const char *path, scann_hip_index **out) {
    if (!ctx || !out) return fail(SCANN_HIP_INVALID_ARGUMENT, "null ctx/out_index");
    Mapping m;
    SCANN_TRY(open_mapping(path, &m));
    const FileHeader &h = m.header();
    // Pin the mapping so the uploads DMA straight from the page cache.  Best effort: a driver
    // that cannot pin a read-only file mapping leaves the (staged) pageable copy path.
    if (scann::read_knobs().load_pin) {
        if (hipHostRegister(m.base, m.bytes, hipHostRegisterReadOnly) == hipSuccess) m.pinned = true;
        else scann::clear_last_hip_error();
    }
    const void *p = nullptr;
    if (h.kind == 0) {
        SCANN_TRY(section(m, path, "data", bytes3(h.n_rows, h.stride, 4), true, &p));
        return scann_hip_bf_create(ctx, static_cast<const float *>(p), h.n_rows, h.dim, h.stride,
                                   h.distance_measure, out);
    }
    scann_hip_txh_desc d;
    std::memset(&d, 0, sizeof(d));
    d.n_rows = h.n_rows;
    d.n_local = h.n_local;
    d.dim = h.dim;
    d.stride = h.stride;
    d.num_partitions = h.num_partitions;
    d.num_subspaces = h.num_subspaces;
    d.num_codes = h.num_codes;
    d.dims_per_subspace = h.dims_per_subspace;
    d.distance_measure = h.distance_measure;
    d.data_is_csr_order = h.data_is_csr_order;
    d.codes_packed4 = h.codes_packed4;
    d.use_residuals = h.use_residuals;
    d.partitions_to_search = h.partitions_to_search;
    d.pre_reorder_multiplier = h.pre_reorder_multiplier;
    // a projected handle: `data` holds the original rows at proj_meta's row_stride, not at the header's stride
    uint32_t pmeta[5] = {0, 0, 0, 0, 0};
    const bool projected = m.find("proj_meta") != nullptr;
    if (projected) {
        SCANN_TRY(section(m, path, "proj_meta", sizeof(pmeta), true, &p));
        std::memcpy(pmeta, p, sizeof(pmeta));
        const uint32_t kind = pmeta[0], in_dim = pmeta[1], out_dim = pmeta[2], start = pmeta[3], row_stride = pmeta[4];
        const bool known = kind == SCANN_HIP_PROJ_MATRIX || kind == SCANN_HIP_PROJ_PCA || kind == SCANN_HIP_PROJ_TRUNCATE;
        if (!known || in_dim == 0 || out_dim != h.dim || row_stride < in_dim ||
            (kind == SCANN_HIP_PROJ_TRUNCATE ? (uint64_t)start + out_dim > in_dim : start != 0))
            return fail(SCANN_HIP_DATA_LOSS, std::string(path) + ": proj_meta disagrees with the header or with itself");
        if (m.find("rows_q")) return fail(SCANN_HIP_DATA_LOSS, std::string(path) + ": both 'proj_meta' and 'rows_q' sections");
    }
    SCANN_TRY(section(m, path, "data", bytes3(h.n_rows, projected ? pmeta[4] : h.stride, 4), false, &p));
    const float *data = static_cast<const float *>(p);
    if (!projected) d.data = data;
    if (h.num_partitions) {
        SCANN_TRY(section(m, path, "centers", bytes3(h.num_partitions, h.dim, 4), true, &p));
        d.centers = static_cast<const float *>(p);
        SCANN_TRY(section(m, path, "leaf_offsets", ((uint64_t)h.num_partitions + 1) * 4, true, &p));
        d.leaf_offsets = static_cast<const uint32_t *>(p);
        SCANN_TRY(section(m, path, "leaf_ids", bytes3(h.n_local, 4, 1), true, &p));
        d.leaf_ids = static_cast<const uint32_t *>(p);
        SCANN_TRY(section(m, path, "leaf_sizes_global", (uint64_t)h.num_partitions * 4, false, &p));
        d.leaf_sizes_global = static_cast<const uint32_t *>(p);
    }
    if (h.num_subspaces) {
        const uint64_t bpp = h.codes_packed4 ? (h.num_subspaces + 1) / 2 : h.num_subspaces;
        SCANN_TRY(section(m, path, "codebook", bytes3(bytes3(h.num_subspaces, h.num_codes, h.dims_per_subspace), 4, 1),
                          true, &p));
        d.codebook = static_cast<const float *>(p);
        SCANN_TRY(section(m, path, "codes", bytes3(h.n_local, bpp, 1), true, &p));
        d.codes = static_cast<const uint8_t *>(p);
    }
    if (m.find("rows_q")) {   // a handle over quantized rows: the rows as stored, their format and inv_multiplier
        SCANN_TRY(section(m, path, "rows_q_meta", 8, true, &p));
        uint32_t meta[2];
        std::memcpy(meta, p, 8);
        const int fmt = (int)meta[0];
        float inv;
        std::memcpy(&inv, &meta[1], 4);
        if (fmt != SCANN_HIP_ROWS_BF16 && fmt != SCANN_HIP_ROWS_FP8_E4M3 && fmt != SCANN_HIP_ROWS_INT8)
            return fail(SCANN_HIP_DATA_LOSS, std::string(path) + ": rows_q_meta names no row format");
        if (fmt == SCANN_HIP_ROWS_INT8 && !std::isfinite(inv))
            return fail(SCANN_HIP_DATA_LOSS, std::string(path) + ": rows_q_meta holds a non-finite inv_multiplier");
        if (d.data) return fail(SCANN_HIP_DATA_LOSS, std::string(path) + ": both 'data' and 'rows_q' sections");
        SCANN_TRY(section(m, path, "rows_q", bytes3(h.n_rows, h.stride, fmt == SCANN_HIP_ROWS_BF16 ? 2 : 1), true, &p));
        SCANN_TRY(scann::txh_quantized_args(&d, p, fmt, inv));
        return scann::txh_create_checked(ctx, &d, out, SCANN_HIP_DATA_LOSS, p, fmt, inv);
    }
    if (projected) {
        const uint32_t kind = pmeta[0], in_dim = pmeta[1], out_dim = pmeta[2];
        const void *pm = nullptr, *pmean = nullptr;
        const bool dense = kind != SCANN_HIP_PROJ_TRUNCATE;
        SCANN_TRY(section(m, path, "proj_matrix", bytes3(out_dim, in_dim, 4), dense, &pm));
        SCANN_TRY(section(m, path, "proj_mean", (uint64_t)in_dim * 4, kind == SCANN_HIP_PROJ_PCA, &pmean));
        if (!dense && (pm || pmean))
            return fail(SCANN_HIP_DATA_LOSS, std::string(path) + ": a TRUNCATE projection with a matrix or a mean");
        if (kind == SCANN_HIP_PROJ_MATRIX && pmean)
            return fail(SCANN_HIP_DATA_LOSS, std::string(path) + ": a MATRIX projection with a mean");
        scann_hip_projection *proj = nullptr;
        SCANN_TRY(scann_hip_projection_create(ctx, (int)kind, in_dim, out_dim, static_cast<const float *>(pm),
                                              static_cast<const float *>(pmean), pmeta[3], &proj));
        const int s = scann::txh_create_projected_checked(ctx, &d, proj, data, h.n_rows, in_dim, pmeta[4], out,
                                                          SCANN_HIP_DATA_LOSS);
        scann_hip_projection_destroy(proj);
        return s;
    }
    return scann::txh_create_checked(ctx, &d, out, SCANN_HIP_DATA_LOSS);
}

}  // extern "C"

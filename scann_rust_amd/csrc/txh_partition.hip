// txh_partition.hip -- K1, K3 and K4 of the tree / flat-hasher search (see txh.hip for the pipeline): centroid scores,
// the flat hasher's tokens, work lists and the lookup tables, with their launchers.  K2, the leaf selection, stays in
// txh.hip: the one-launch small and wide pipelines there run select_leaves_body inside their own kernels.
#include "launch.h"
#include "txh_stages.h"

namespace scann {

// =====================================================================================
// K1: centroid scores.  partitioning/tree_partitioner.rs:175-192: strictly sequential
// scalar sum of (q_j - c_j)^2, no FMA.  One thread per centroid, QT queries per block
// broadcast from LDS.
// =====================================================================================
template <int kCsQT>
__global__ __launch_bounds__(64) void centroid_scores_kernel(
    const float *__restrict__ centers, uint32_t L, uint32_t dim,
    const float *__restrict__ queries, uint32_t nq, uint32_t q_stride,
    float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float qs[];  // [kCsQT][dim]
    const uint32_t q0 = blockIdx.y * kCsQT;
    for (uint32_t i = threadIdx.x; i < kCsQT * dim; i += blockDim.x) {
        uint32_t qi = i / dim, j = i - qi * dim;
        qs[i] = (q0 + qi < nq) ? queries[(size_t)(q0 + qi) * q_stride + j] : 0.0f;
    }
    __syncthreads();
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= L) return;
    float acc[kCsQT];
#pragma unroll
    for (int qi = 0; qi < kCsQT; ++qi) acc[qi] = 0.0f;
    const float *crow = centers + (size_t)c * dim;
    if ((dim & 3u) == 0) {
        for (uint32_t j = 0; j < dim; j += 4) {
            const float4 cv = *reinterpret_cast<const float4 *>(crow + j);
#pragma unroll
            for (int qi = 0; qi < kCsQT; ++qi) {
                const float4 qv = *reinterpret_cast<const float4 *>(qs + qi * dim + j);
                float d0 = qv.x - cv.x, d1 = qv.y - cv.y, d2 = qv.z - cv.z, d3 = qv.w - cv.w;
                float a = acc[qi];
                a = a + d0 * d0;
                a = a + d1 * d1;
                a = a + d2 * d2;
                a = a + d3 * d3;
                acc[qi] = a;
            }
        }
    } else {
        for (uint32_t j = 0; j < dim; ++j) {
            const float cv = crow[j];
#pragma unroll
            for (int qi = 0; qi < kCsQT; ++qi) {
                float d = qs[qi * dim + j] - cv;
                acc[qi] = acc[qi] + d * d;
            }
        }
    }
#pragma unroll
    for (int qi = 0; qi < kCsQT; ++qi)
        if (q0 + qi < nq) out[(size_t)(q0 + qi) * L + c] = acc[qi];
}

// AsymmetricHasher mode: one implicit leaf (id 0) for every query.
__global__ void ah_tokens_kernel(uint32_t nq, const uint32_t *__restrict__ leaf_gsize,
                                 const uint32_t *__restrict__ leaf_off, uint32_t st,
                                 uint32_t *__restrict__ tokens, float *__restrict__ token_dists,
                                 uint32_t *__restrict__ vbase, uint32_t *__restrict__ sbase) {
    uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    tokens[q] = 0;
    token_dists[q] = 0.0f;
    vbase[2 * q] = 0;
    vbase[2 * q + 1] = leaf_gsize[0];
    const uint32_t sz = leaf_off[1] - leaf_off[0];
    sbase[3 * q] = 0;
    sbase[3 * q + 1] = (sz + st - 1) / st;
    sbase[3 * q + 2] = sz;
}

// =====================================================================================
// K3: worklist -- group (query, rank) pairs by leaf so that every leaf's codes are read
// once per batch and shared by all queries that selected it.
// =====================================================================================
// One launch instead of five memsets: zero the per-batch counters, mark all pair slots free.
__global__ void txh_init_kernel(uint32_t L, uint32_t nq, uint32_t max_slots,
                                uint32_t *__restrict__ leaf_cnt, uint32_t *__restrict__ leaf_cursor,
                                uint32_t *__restrict__ counters, uint32_t *__restrict__ cand_cnt,
                                uint32_t *__restrict__ cand32_cnt, uint32_t *__restrict__ pair_q) {
    const uint32_t i0 = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    for (uint32_t i = i0; i < L; i += step) {
        leaf_cnt[i] = 0;
        leaf_cursor[i] = 0;
    }
    for (uint32_t i = i0; i < nq; i += step) {
        cand_cnt[i] = 0;
        if (cand32_cnt) cand32_cnt[i] = 0;
    }
    for (uint32_t i = i0; i < max_slots; i += step) pair_q[i] = kInvalid;
    for (uint32_t i = i0; i < CNT_WORDS; i += step) counters[i] = 0;
}

// ah != 0: one implicit leaf selected by every query -- no atomics (1024 same-address global
// atomics cost more than the whole LUT build).
__global__ void worklist_count_kernel(uint32_t npairs, int ah, const uint32_t *__restrict__ tokens,
                                      const uint32_t *__restrict__ leaf_off,
                                      uint32_t *__restrict__ leaf_cnt) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (ah) {
        if (i == 0) leaf_cnt[0] = leaf_off[1] > leaf_off[0] ? npairs : 0u;
        return;
    }
    if (i >= npairs) return;
    uint32_t leaf = tokens[i];
    if (leaf_off[leaf + 1] > leaf_off[leaf]) atomicAdd(&leaf_cnt[leaf], 1u);
}

__global__ __launch_bounds__(1024) void worklist_scan_kernel(
    uint32_t L, const uint32_t *__restrict__ leaf_cnt, const uint32_t *__restrict__ leaf_off,
    uint32_t tp, uint32_t quads_per_tile, uint32_t chunks_per_tile, uint32_t stp, uint32_t st,
    uint32_t squads_per_tile,
    uint32_t *__restrict__ pair_off, uint32_t *__restrict__ tile_off,
    uint32_t *__restrict__ stile_off, uint32_t *__restrict__ counters) {
    __shared__ uint32_t s_pairs[1024], s_tiles[1024], s_stiles[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (L + 1023) / 1024;
    const uint32_t b = t * per, e = min(L, b + per);
    // tiles of the scan (all points) and of the sample pass (every st-th point)
    auto tiles_of = [&](uint32_t c, uint32_t pad, uint32_t sz, uint32_t *smp) {
        if (!c) { *smp = 0; return 0u; }
        const uint32_t ssz = (sz + st - 1) / st;
        *smp = ((ssz + stp - 1) / stp) * ((pad / 4 + squads_per_tile - 1) / squads_per_tile);
        const uint32_t nch = (sz + tp - 1) / tp;
        return ((nch + chunks_per_tile - 1) / chunks_per_tile) * ((pad / 4 + quads_per_tile - 1) / quads_per_tile);
    };
    uint32_t sp = 0, stl = 0, sst = 0;
    for (uint32_t l = b; l < e; ++l) {
        uint32_t c = leaf_cnt[l];
        uint32_t pad = (c + 3u) & ~3u;
        uint32_t sz = leaf_off[l + 1] - leaf_off[l];
        uint32_t smp;
        sp += pad;
        stl += tiles_of(c, pad, sz, &smp);
        sst += smp;
    }
    s_pairs[t] = sp;
    s_tiles[t] = stl;
    s_stiles[t] = sst;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {  // Hillis-Steele inclusive scan
        uint32_t a = 0, c2 = 0, c3 = 0;
        if (t >= off) {
            a = s_pairs[t - off];
            c2 = s_tiles[t - off];
            c3 = s_stiles[t - off];
        }
        __syncthreads();
        s_pairs[t] += a;
        s_tiles[t] += c2;
        s_stiles[t] += c3;
        __syncthreads();
    }
    uint32_t bp = s_pairs[t] - sp, bt = s_tiles[t] - stl, bs = s_stiles[t] - sst;
    for (uint32_t l = b; l < e; ++l) {
        uint32_t c = leaf_cnt[l];
        uint32_t pad = (c + 3u) & ~3u;
        uint32_t sz = leaf_off[l + 1] - leaf_off[l];
        uint32_t smp;
        pair_off[l] = bp;
        tile_off[l] = bt;
        stile_off[l] = bs;
        bp += pad;
        bt += tiles_of(c, pad, sz, &smp);
        bs += smp;
    }
    if (t == 1023) {
        pair_off[L] = s_pairs[1023];
        tile_off[L] = s_tiles[1023];
        stile_off[L] = s_stiles[1023];
        counters[CNT_TOTAL_QUADS] = s_pairs[1023] / 4;
        counters[CNT_TOTAL_TILES] = s_tiles[1023];
        counters[CNT_TOTAL_STILES] = s_stiles[1023];
    }
}

// AsymmetricHasher mode (one leaf, every query's only token): everything txh_init_kernel, ah_tokens_kernel and
// the three worklist kernels write is known from nq alone -- one single-workgroup kernel instead of five
// launches (~4.5 us of dispatch each).  Same arrays, same values.
struct AhSetupArgs {
    uint32_t nq, max_slots, st, tp, quads_per_tile, chunks_per_tile, stp, squads_per_tile;
    const uint32_t *leaf_gsize, *leaf_off;
    uint32_t *leaf_cnt, *leaf_cursor, *counters, *cand_cnt, *cand32_cnt, *pair_q, *pair_leaf, *pair_vbase, *pair_sbase,
        *slot_of, *tokens, *vbase, *sbase, *pair_off, *tile_off, *stile_off;
    float *token_dists;
};

__global__ __launch_bounds__(1024) void ah_setup_kernel(AhSetupArgs a) {
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    const uint32_t sz = a.leaf_off[1] - a.leaf_off[0], gs = a.leaf_gsize[0];
    const uint32_t c = sz ? a.nq : 0u, pad = (c + 3u) & ~3u;
    const uint32_t ssz = (sz + a.st - 1) / a.st;
    for (uint32_t i = tid; i < a.max_slots; i += nt) a.pair_q[i] = (sz && i < a.nq) ? i : kInvalid;   // slot of query i = i
    for (uint32_t i = tid; i < CNT_WORDS; i += nt) {
        uint32_t v = 0;
        if (c) {
            const uint32_t nch = (sz + a.tp - 1) / a.tp;
            if (i == CNT_TOTAL_QUADS) v = pad / 4;
            if (i == CNT_TOTAL_TILES)
                v = ((nch + a.chunks_per_tile - 1) / a.chunks_per_tile) * ((pad / 4 + a.quads_per_tile - 1) / a.quads_per_tile);
            if (i == CNT_TOTAL_STILES)
                v = ((ssz + a.stp - 1) / a.stp) * ((pad / 4 + a.squads_per_tile - 1) / a.squads_per_tile);
        }
        a.counters[i] = v;
    }
    for (uint32_t q = tid; q < a.nq; q += nt) {
        a.cand_cnt[q] = 0;
        if (a.cand32_cnt) a.cand32_cnt[q] = 0;
        a.tokens[q] = 0;
        a.token_dists[q] = 0.0f;
        a.vbase[2 * q] = 0;
        a.vbase[2 * q + 1] = gs;
        a.sbase[3 * q] = 0;
        a.sbase[3 * q + 1] = ssz;
        a.sbase[3 * q + 2] = sz;
        if (sz) {
            a.pair_leaf[q] = 0;
            a.pair_vbase[q] = 0;
            a.pair_sbase[q] = 0;
        }
        a.slot_of[q] = sz ? q : kInvalid;
    }
    if (tid == 0) {
        a.leaf_cnt[0] = c;
        a.leaf_cursor[0] = 0;
        uint32_t tiles = 0, stiles = 0;
        if (c) {
            const uint32_t nch = (sz + a.tp - 1) / a.tp;
            tiles = ((nch + a.chunks_per_tile - 1) / a.chunks_per_tile) * ((pad / 4 + a.quads_per_tile - 1) / a.quads_per_tile);
            stiles = ((ssz + a.stp - 1) / a.stp) * ((pad / 4 + a.squads_per_tile - 1) / a.squads_per_tile);
        }
        a.pair_off[0] = 0;
        a.pair_off[1] = pad;
        a.tile_off[0] = 0;
        a.tile_off[1] = tiles;
        a.stile_off[0] = 0;
        a.stile_off[1] = stiles;
    }
}

__global__ void worklist_fill_kernel(uint32_t nq, uint32_t P, int ah, const uint32_t *__restrict__ tokens,
                                     const uint32_t *__restrict__ vbase,
                                     const uint32_t *__restrict__ sbase,
                                     const uint32_t *__restrict__ leaf_off,
                                     const uint32_t *__restrict__ pair_off,
                                     uint32_t *__restrict__ leaf_cursor,
                                     uint32_t *__restrict__ pair_q, uint32_t *__restrict__ pair_leaf,
                                     uint32_t *__restrict__ pair_vbase,
                                     uint32_t *__restrict__ pair_sbase,
                                     uint32_t *__restrict__ slot_of) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq * P) return;
    uint32_t q = i / P, r = i - q * P;
    uint32_t leaf = tokens[i];
    uint32_t slot = kInvalid;
    if (leaf_off[leaf + 1] > leaf_off[leaf]) {
        slot = pair_off[leaf] + (ah ? i : atomicAdd(&leaf_cursor[leaf], 1u));
        pair_q[slot] = q;
        pair_leaf[slot] = leaf;
        pair_vbase[slot] = vbase[(size_t)q * (P + 1) + r];
        pair_sbase[slot] = sbase[(size_t)q * (P + 2) + r];
    }
    slot_of[i] = slot;
}

// =====================================================================================
// K4: LUT build.  tree_x_hybrid/mod.rs:309-319 + hashes/lut.rs:47-70 +
// hashes/codebook.rs:98-115: q' = q - centroid (if residual); LUT[s][c] = sequential
// scalar sum over dsub of (q'_j - cb_j)^2.  Output layout is quad-interleaved
// [quad][s][kp][4] (kp = 16 or 256 slots) so that the scan reads four queries' entries with
// one ds_read_b128.
// =====================================================================================
__global__ __launch_bounds__(256) void lut_build_kernel(
    TxhIndexDev ix, const float *__restrict__ queries, uint32_t q_stride,
    const uint32_t *__restrict__ pair_q, const uint32_t *__restrict__ pair_leaf,
    const uint32_t *__restrict__ counters, float *__restrict__ lutq) {
    extern __shared__ float qres[];  // [4][dim]
    const uint32_t quad = blockIdx.x;
    if (quad >= counters[CNT_TOTAL_QUADS]) return;
    const uint32_t dim = ix.dim;
    for (uint32_t i = threadIdx.x; i < 4 * dim; i += blockDim.x) {
        uint32_t p = i / dim, j = i - p * dim;
        uint32_t q = pair_q[quad * 4 + p];
        float v = 0.0f;
        if (q != kInvalid) {
            v = queries[(size_t)q * q_stride + j];
            if (ix.use_residuals) v = v - ix.centers[(size_t)pair_leaf[quad * 4 + p] * dim + j];
        }
        qres[i] = v;
    }
    __syncthreads();
    const uint32_t S = ix.S, K = ix.K, dsub = ix.dsub, kp = ix.kp;   // kp = 16 or 256 table slots
    float4 *out = reinterpret_cast<float4 *>(lutq) + (size_t)quad * S * kp;
    for (uint32_t e = threadIdx.x; e < S * kp; e += blockDim.x) {
        uint32_t s = e / kp, c = e - s * kp;
        float r[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (c < K) {
            const float *cb = ix.codebook + ((size_t)s * K + c) * dsub;
            for (uint32_t j = 0; j < dsub; ++j) {
                float cv = cb[j];
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    float d = qres[p * dim + s * dsub + j] - cv;
                    r[p] = r[p] + d * d;
                }
            }
        }
        out[e] = make_float4(r[0], r[1], r[2], r[3]);
    }
}

// Plain LookupTable::from_query for callers/tests: out [nq][S][K].
__global__ __launch_bounds__(256) void lut_from_query_kernel(
    TxhIndexDev ix, const float *__restrict__ queries, uint32_t q_stride,
    const uint32_t *__restrict__ leaf_for_query, float *__restrict__ out) {
    extern __shared__ float qres[];  // [dim]
    const uint32_t q = blockIdx.x, dim = ix.dim;
    for (uint32_t j = threadIdx.x; j < dim; j += blockDim.x) {
        float v = queries[(size_t)q * q_stride + j];
        if (leaf_for_query) v = v - ix.centers[(size_t)leaf_for_query[q] * dim + j];
        qres[j] = v;
    }
    __syncthreads();
    const uint32_t S = ix.S, K = ix.K, dsub = ix.dsub;
    for (uint32_t e = threadIdx.x; e < S * K; e += blockDim.x) {
        uint32_t s = e / K;
        const float *cb = ix.codebook + (size_t)e * dsub;
        float r = 0.0f;
        for (uint32_t j = 0; j < dsub; ++j) {
            float d = qres[s * dsub + j] - cb[j];
            r = r + d * d;
        }
        out[(size_t)q * S * K + e] = r;
    }
}

// =====================================================================================
// launchers
// =====================================================================================
int launch_ah_tokens(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st) {
    SCANN_TRY(launch(ah_tokens_kernel, dim3(ceil_div_u32(w.nq, 256)), dim3(256), 0, st, w.nq,
                     ix.leaf_gsize, ix.leaf_off, w.st, w.tokens, w.token_dists, w.vbase, w.sbase));
    return SCANN_HIP_OK;
}

int launch_centroid_scores(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st) {
    // queries per single-wave block: fewer when the grid would not fill the chip (one thread per
    // centroid, so a block's work is 64 centroids x QT queries), and 4 where 16 queries exceed the LDS (dim > 2560):
    // the per-pair arithmetic is the same, so a dim that one batch size accepts every batch size accepts
    const uint64_t waves16 = (uint64_t)ceil_div_u32(ix.L, 64) * ceil_div_u32(w.nq, 16);
    const bool fits16 = (size_t)16 * ix.dim * sizeof(float) <= kMaxLdsBytes;
    return with_value<16, 4>(waves16 >= 8192 && fits16 ? 16 : 4, [&](auto qt) {
        const size_t lds1 = (size_t)qt() * ix.dim * sizeof(float);
        return launch(centroid_scores_kernel<qt()>, dim3(ceil_div_u32(ix.L, 64), ceil_div_u32(w.nq, qt())), dim3(64), lds1,
                      st, ix.centers, ix.L, ix.dim, w.queries, w.nq, w.q_stride, w.cdist);
    });
}

int launch_ah_setup(const TxhIndexDev &ix, const TxhWork &w, const WorkTiling &t, hipStream_t st) {
    const bool mfma = txh_scan_is_mfma(w.scan);
    AhSetupArgs h;
    h.nq = w.nq; h.max_slots = w.max_slots; h.st = w.st; h.tp = t.tp; h.quads_per_tile = t.qpt;
    h.chunks_per_tile = t.cpt; h.stp = scan_tile_points(ix); h.squads_per_tile = w.sqpt;
    h.leaf_gsize = ix.leaf_gsize; h.leaf_off = ix.leaf_off; h.leaf_cnt = w.leaf_cnt; h.leaf_cursor = w.leaf_cursor;
    h.counters = w.counters; h.cand_cnt = w.cand_cnt; h.cand32_cnt = mfma ? w.cand32_cnt : nullptr;
    h.pair_q = w.pair_q; h.pair_leaf = w.pair_leaf; h.pair_vbase = w.pair_vbase; h.pair_sbase = w.pair_sbase;
    h.slot_of = w.slot_of; h.tokens = w.tokens; h.vbase = w.vbase; h.sbase = w.sbase; h.pair_off = w.pair_off;
    h.tile_off = w.tile_off; h.stile_off = w.stile_off; h.token_dists = w.token_dists;
    SCANN_TRY(launch(ah_setup_kernel, dim3(1), dim3(1024), 0, st, h));
    return SCANN_HIP_OK;
}

int launch_work_init(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st) {
    const uint32_t work = std::max(std::max(ix.L, w.nq), w.max_slots);
    SCANN_TRY(launch(txh_init_kernel, dim3(std::min(1024u, ceil_div_u32(work, 256))), dim3(256), 0, st,
                     ix.L, w.nq, w.max_slots, w.leaf_cnt, w.leaf_cursor, w.counters, w.cand_cnt,
                     txh_scan_is_mfma(w.scan) ? w.cand32_cnt : nullptr, w.pair_q));
    return SCANN_HIP_OK;
}

int launch_work_lists(const TxhIndexDev &ix, const TxhWork &w, const WorkTiling &t, hipStream_t st) {
    const uint32_t npairs = w.nq * w.P;
    SCANN_TRY(launch(worklist_count_kernel, dim3(ceil_div_u32(npairs, 256)), dim3(256), 0, st,
                     npairs, ix.ah_mode, w.tokens, ix.leaf_off, w.leaf_cnt));
    SCANN_TRY(launch(worklist_scan_kernel, dim3(1), dim3(1024), 0, st, ix.L, w.leaf_cnt,
                     ix.leaf_off, t.tp, t.qpt, t.cpt, scan_tile_points(ix), w.st,
                     w.sqpt, w.pair_off, w.tile_off,
                     w.stile_off, w.counters));
    SCANN_TRY(launch(worklist_fill_kernel, dim3(ceil_div_u32(npairs, 256)), dim3(256), 0, st, w.nq,
                     w.P, ix.ah_mode, w.tokens, w.vbase, w.sbase, ix.leaf_off, w.pair_off, w.leaf_cursor, w.pair_q,
                     w.pair_leaf, w.pair_vbase, w.pair_sbase, w.slot_of));
    return SCANN_HIP_OK;
}

int launch_lut_build(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st) {
    const size_t lds_lut = (size_t)4 * ix.dim * sizeof(float);
    SCANN_TRY(launch(lut_build_kernel, dim3(w.max_quads), dim3(256), lds_lut, st, ix, w.queries,
                     w.q_stride, w.pair_q, w.pair_leaf, w.counters, w.lutq));
    return SCANN_HIP_OK;
}

int txh_launch_lut_from_query(const TxhIndexDev &ix, const float *d_queries, uint32_t nq,
                              uint32_t q_stride, const uint32_t *d_leaf_for_query,
                              float *d_out_lut, hipStream_t st) {
    if (nq == 0) return SCANN_HIP_OK;
    const size_t lds = (size_t)ix.dim * sizeof(float);
    SCANN_TRY(launch(lut_from_query_kernel, dim3(nq), dim3(256), lds, st, ix, d_queries, q_stride,
                     d_leaf_for_query, d_out_lut));
    return SCANN_HIP_OK;
}

__global__ __launch_bounds__(256) void transpose_centers_kernel(const float *__restrict__ centers, uint32_t L,
                                                                uint32_t dim, uint32_t pitch, float *__restrict__ out) {
    const uint64_t total = (uint64_t)dim * pitch;
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (uint64_t)gridDim.x * 256) {
        const uint32_t j = (uint32_t)(e / pitch), c = (uint32_t)(e - (uint64_t)j * pitch);
        out[e] = c < L ? centers[(size_t)c * dim + j] : 0.0f;
    }
}

int launch_transpose_centers(const float *d_centers, uint32_t L, uint32_t dim, uint32_t pitch, float *d_out,
                             hipStream_t st) {
    if (L == 0 || dim == 0) return SCANN_HIP_OK;
    SCANN_TRY(launch(transpose_centers_kernel, dim3((uint32_t)std::min<uint64_t>(ceil_div_u64((uint64_t)dim * pitch, 256), 4096)),
                     dim3(256), 0, st, d_centers, L, dim, pitch, d_out));
    return SCANN_HIP_OK;
}

}  // namespace scann

// stacked.hip -- stacked / additive quantizer handles: StackedQuantizer and AdditiveQuantizer of the
// reference (hashes/stacked.rs) as one handle kind: L levels of codebooks, level l with S_l subspaces of K_l codes; a row
// is T = sum S_l code bytes.  Encode, decode and an exhaustive asymmetric-distance scan over resident codes.
//
//   stacked_encode_kernel     one workgroup per tile of R rows, every level in the one launch.  The residuals live in
//                             LDS as f32 [R][dim | 1]; a level's centroids pass through a 32 KB LDS stage in slabs
//                             (groups of whole subspaces, or runs of codes of one subspace when a subspace alone does
//                             not fit: the additive form); every squared distance is one sequential chain owned by one
//                             lane; the owner subtracts the chosen centroid in place.  Writes codes row-major (encode)
//                             or in the scan layout with the rows' norms (set_rows).
//   stacked_set_codes_kernel  one thread per row: checks the codes, transposes them into the scan layout, norms.
//   stacked_decode_kernel     one thread per element.
//   stacked_lut_kernel        per query quad the tables lut[t][c] as float4 (four queries per entry), and qq.
//   stacked_scan_kernel       grid (query groups of one or two quads, row chunks), 8 waves.  A lane keeps 4 rows x 4 or 8
//                             queries of accumulators in registers and walks the code positions in ascending order;
//                             the tables pass through LDS in slabs of whole code dwords, double-buffered, prefetched into
//                             registers while the current slab is gathered (one ds_read_b128 per row, position and quad).
//                             Epilogue: the measure, the allow bit, the append-and-bitonic selection of sparse_dev.h.
//   sparse.hip's merge kernel sorts the chunk partials.
// No matrix instructions: every sum has a fixed order of f32 additions and the scan is bound by LDS gathers.
#include <memory>
#include <vector>

#include "comm.h"   // ctx_device
#include "launch.h"
#include "sparse_dev.h"
#include "stacked.h"

struct scann_hip_stacked {
    int device = 0;
    scann::StackedShape sh{};
    int measure = SCANN_HIP_DOT_PRODUCT;
    uint64_t n = 0;
    bool has_rows = false;
    uint32_t tile_rows = 0;
    scann::DevBuf cb, eoff, codes, xx;   // codebooks, entry offsets; the scan layout [block][dword][64] and the rows' norms
    // calls: one stream and grow-only buffers, one call at a time
    std::mutex mu;
    hipStream_t stream = nullptr;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // encode 0-1; lut, scan, merge 2-5
    float encode_ms = 0.0f;
    bool timed = false;
    uint64_t last[5] = {0, 0, 0, 0, 0};   // of the last scan: slabs, chunk rows, chunks, quads per workgroup, query groups
    scann::DevBuf rows_in, codes_io, res, queries, lut, qq, slab_dw, allow, partial, out_idx, out_dist, out_count, dist, flag;
    ~scann_hip_stacked() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace scann {
namespace {

constexpr uint32_t kSmallThreads = 256;
constexpr uint32_t kBufEntries = kStackedSlabBytes / 16;

struct StackedEncArgs {
    StackedShape sh;
    const float *cb;
    const float *rows;      // this launch's rows, `stride` floats apart
    uint32_t n, stride, tile_rows;
    uint8_t *out_codes;     // encode: [n][T]
    float *out_res;         // encode: [n], or null
    uint32_t *scan_codes;   // set_rows: the handle's scan layout (null for an encode)
    float *xx;              // set_rows: the handle's norms
    uint64_t row_base;      // set_rows: the handle row of this launch's first row (a multiple of 64)
};

__global__ __launch_bounds__(kStackedEncThreads) void stacked_encode_kernel(const StackedEncArgs a) {
    extern __shared__ __align__(16) unsigned char stacked_lds[];
    __shared__ float s_best[kStackedEncThreads];
    __shared__ uint32_t s_idx[kStackedEncThreads];
    const StackedShape &sh = a.sh;
    const uint32_t tid = threadIdx.x, R = a.tile_rows, dim = sh.dim, T = sh.T, rs = dim | 1u;
    float *tile = reinterpret_cast<float *>(stacked_lds);            // [R][rs]
    float *stage = tile + (size_t)R * rs;                            // one slab of centroids
    uint8_t *codes = reinterpret_cast<uint8_t *>(stage + kStackedEncStageBytes / 4);   // [R][T]
    const uint32_t row0 = blockIdx.x * R;
    const uint32_t nr = a.n - row0 < R ? a.n - row0 : R;

    for (uint32_t i = tid; i < nr * dim; i += kStackedEncThreads) {
        const uint32_t r = i / dim, j = i - r * dim;
        tile[r * rs + j] = a.rows[(size_t)(row0 + r) * a.stride + j];
    }
    for (uint32_t l = 0; l < sh.levels; ++l) {
        const uint32_t S = sh.S[l], K = sh.K[l], dsub = sh.dsub[l], per = K * dsub, toff = sh.toff[l];
        const float *cbl = a.cb + sh.cboff[l];
        if (per <= kStackedEncStageBytes / 4) {
            // groups of whole subspaces: one (row, subspace) per thread and turn, every code of the subspace in the stage
            const uint32_t group = (kStackedEncStageBytes / 4) / per;
            for (uint32_t s0 = 0; s0 < S; s0 += group) {
                const uint32_t gs = S - s0 < group ? S - s0 : group;
                __syncthreads();   // the tile is loaded; the stage's readers are done
                for (uint32_t i = tid; i < gs * per; i += kStackedEncThreads) stage[i] = cbl[(size_t)s0 * per + i];
                __syncthreads();
                for (uint32_t it = tid; it < nr * gs; it += kStackedEncThreads) {
                    const uint32_t sg = it / nr, r = it - sg * nr;
                    float *x = tile + r * rs + (s0 + sg) * dsub;
                    const float *cs = stage + sg * per;
                    float best = INFINITY;
                    uint32_t bi = 0;
                    for (uint32_t c = 0; c < K; ++c) {
                        float d = 0.0f;
                        for (uint32_t j = 0; j < dsub; ++j) {
                            const float df = x[j] - cs[c * dsub + j];
                            d += df * df;
                        }
                        if (d < best) {
                            best = d;
                            bi = c;
                        }
                    }
                    codes[r * T + toff + s0 + sg] = (uint8_t)bi;
                    for (uint32_t j = 0; j < dsub; ++j) x[j] = x[j] - cs[bi * dsub + j];
                }
            }
        } else {
            // one subspace's centroids exceed the stage: runs of codes, ascending.  Thread (row r, part p) scans its share
            // of every run and carries (best, index) across the runs; the parts meet in LDS on (distance, index).
            const uint32_t run = (kStackedEncStageBytes / 4) / dsub, P = kStackedEncThreads / R;
            const uint32_t p = tid / R, r = tid - p * R;
            const bool mine = p < P && r < nr;
            for (uint32_t s = 0; s < S; ++s) {
                float best = INFINITY;
                uint32_t bi = 0;
                for (uint32_t c0 = 0; c0 < K; c0 += run) {
                    const uint32_t rc = K - c0 < run ? K - c0 : run;
                    __syncthreads();
                    for (uint32_t i = tid; i < rc * dsub; i += kStackedEncThreads) stage[i] = cbl[((size_t)s * K + c0) * dsub + i];
                    __syncthreads();
                    if (mine) {
                        const float *x = tile + r * rs + s * dsub;
                        for (uint32_t c = rc * p / P; c < rc * (p + 1) / P; ++c) {
                            float d = 0.0f;
                            for (uint32_t j = 0; j < dsub; ++j) {
                                const float df = x[j] - stage[c * dsub + j];
                                d += df * df;
                            }
                            if (d < best) {   // (a part meets its codes in ascending order, run after run)
                                best = d;
                                bi = c0 + c;
                            }
                        }
                    }
                }
                s_best[tid] = best;
                s_idx[tid] = bi;
                __syncthreads();
                if (mine && p == 0) {
                    // the parts' codes interleave, so an equal distance goes to the lower index; a part that saw no
                    // distance below +inf holds (+inf, 0) and never wins: all of them -> code 0
                    for (uint32_t pp = 1; pp < P; ++pp) {
                        const float d = s_best[pp * R + r];
                        const uint32_t ci = s_idx[pp * R + r];
                        if (d < best || (d == best && d < INFINITY && ci < bi)) {
                            best = d;
                            bi = ci;
                        }
                    }
                    codes[r * T + toff + s] = (uint8_t)bi;
                    float *x = tile + r * rs + s * dsub;
                    const float *cc = cbl + ((size_t)s * K + bi) * dsub;
                    for (uint32_t j = 0; j < dsub; ++j) x[j] = x[j] - cc[j];
                }
            }
        }
    }
    __syncthreads();
    if (a.out_res && tid < nr) {
        float s = 0.0f;
        for (uint32_t j = 0; j < dim; ++j) s += tile[tid * rs + j] * tile[tid * rs + j];
        a.out_res[row0 + tid] = s;
    }
    if (!a.scan_codes) {
        for (uint32_t i = tid; i < nr * T; i += kStackedEncThreads) a.out_codes[(size_t)row0 * T + i] = codes[i];
        return;
    }
    // set_rows: the decoded rows take the residuals' place (sums of centroids, level by level from 0.0f), then their norms
    __syncthreads();
    for (uint32_t i = tid; i < nr * dim; i += kStackedEncThreads) {
        const uint32_t r = i / dim, j = i - r * dim;
        float x = 0.0f;
        for (uint32_t l = 0; l < sh.levels; ++l) {
            const uint32_t s = j / sh.dsub[l], c = codes[r * T + sh.toff[l] + s];
            x += a.cb[sh.cboff[l] + ((size_t)s * sh.K[l] + c) * sh.dsub[l] + (j - s * sh.dsub[l])];
        }
        tile[r * rs + j] = x;
    }
    __syncthreads();
    if (tid < nr) {
        float s = 0.0f;
        for (uint32_t j = 0; j < dim; ++j) s += tile[tid * rs + j] * tile[tid * rs + j];
        a.xx[a.row_base + row0 + tid] = s;
    }
    for (uint32_t i = tid; i < nr * sh.dwords; i += kStackedEncThreads) {
        const uint32_t g = i / nr, r = i - g * nr;
        uint32_t dw = 0;
        for (uint32_t tt = 0; tt < 4 && 4 * g + tt < T; ++tt) dw |= (uint32_t)codes[r * T + 4 * g + tt] << (8 * tt);
        const uint64_t row = a.row_base + row0 + r;
        a.scan_codes[((row >> 6) * sh.dwords + g) * 64 + (row & 63u)] = dw;
    }
}

// the sequential f32 squared norm of the row that `code(t)` decodes to
template <typename Code>
__device__ __forceinline__ float stacked_decoded_norm(const StackedShape &sh, const float *__restrict__ cb, Code code) {
    float xx = 0.0f;
    for (uint32_t j = 0; j < sh.dim; ++j) {
        float x = 0.0f;
        for (uint32_t l = 0; l < sh.levels; ++l) {
            const uint32_t s = j / sh.dsub[l];
            x += cb[sh.cboff[l] + ((size_t)s * sh.K[l] + code(sh.toff[l] + s)) * sh.dsub[l] + (j - s * sh.dsub[l])];
        }
        xx += x * x;
    }
    return xx;
}

__global__ __launch_bounds__(kSmallThreads) void stacked_set_codes_kernel(const StackedShape sh, const float *__restrict__ cb,
                                                                          const uint8_t *__restrict__ codes, uint32_t n, uint64_t row_base,
                                                                          uint32_t *__restrict__ scan_codes, float *__restrict__ xx,
                                                                          uint32_t *bad) {
    const uint32_t r = blockIdx.x * kSmallThreads + threadIdx.x;
    if (r >= n) return;
    const uint8_t *c = codes + (size_t)r * sh.T;
    bool ok = true;
    for (uint32_t l = 0; l < sh.levels; ++l)
        for (uint32_t s = 0; s < sh.S[l]; ++s) ok = ok && c[sh.toff[l] + s] < sh.K[l];
    if (!ok) {   // (no centroid is fetched through a code that is out of range)
        atomicOr(bad, 1u);
        return;
    }
    const uint64_t row = row_base + r;
    for (uint32_t g = 0; g < sh.dwords; ++g) {
        uint32_t dw = 0;
        for (uint32_t tt = 0; tt < 4 && 4 * g + tt < sh.T; ++tt) dw |= (uint32_t)c[4 * g + tt] << (8 * tt);
        scan_codes[((row >> 6) * sh.dwords + g) * 64 + (row & 63u)] = dw;
    }
    xx[row] = stacked_decoded_norm(sh, cb, [&](uint32_t t) { return (uint32_t)c[t]; });
}

__global__ __launch_bounds__(kSmallThreads) void stacked_decode_kernel(const StackedShape sh, const float *__restrict__ cb,
                                                                       const uint8_t *__restrict__ codes, uint64_t elems,
                                                                       float *__restrict__ out, uint32_t *bad) {
    const uint64_t i = (uint64_t)blockIdx.x * kSmallThreads + threadIdx.x;
    if (i >= elems) return;
    const uint64_t r = i / sh.dim;
    const uint32_t j = (uint32_t)(i - r * sh.dim);
    float x = 0.0f;
    for (uint32_t l = 0; l < sh.levels; ++l) {
        const uint32_t s = j / sh.dsub[l], c = codes[r * sh.T + sh.toff[l] + s];
        if (c >= sh.K[l]) {
            atomicOr(bad, 1u);
            return;
        }
        x += cb[sh.cboff[l] + ((size_t)s * sh.K[l] + c) * sh.dsub[l] + (j - s * sh.dsub[l])];
    }
    out[i] = x;
}

// grid (entries / 256, quads): entry e of quad y is lut[t][c] of the quad's four queries, a sequential dot product
// from 0.0f each; queries past nq and the pad positions' entries are +0.0f.  Block x == 0 also writes the quad's qq.
__global__ __launch_bounds__(kSmallThreads) void stacked_lut_kernel(const StackedShape sh, const float *__restrict__ cb,
                                                                    const float *__restrict__ queries, uint32_t nq, uint32_t q_stride,
                                                                    float4 *__restrict__ lut, float *__restrict__ qq) {
    const uint32_t e = blockIdx.x * kSmallThreads + threadIdx.x, quad = blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x < 4 && quad * 4 + threadIdx.x < nq) {
        const float *q = queries + (size_t)(quad * 4 + threadIdx.x) * q_stride;
        float s = 0.0f;
        for (uint32_t j = 0; j < sh.dim; ++j) s += q[j] * q[j];
        qq[quad * 4 + threadIdx.x] = s;
    }
    if (e >= sh.entries) return;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t l = sh.levels - 1;
    while (l > 0 && sh.eoff[l] > e) --l;
    const uint32_t s = (e - sh.eoff[l]) / sh.K[l], c = e - sh.eoff[l] - s * sh.K[l];
    if (s < sh.S[l]) {   // (else: a pad position)
        const uint32_t dsub = sh.dsub[l];
        const float *cc = cb + sh.cboff[l] + ((size_t)s * sh.K[l] + c) * dsub;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            if (quad * 4 + i >= nq) continue;
            const float *q = queries + (size_t)(quad * 4 + i) * q_stride + s * dsub;
            for (uint32_t j = 0; j < dsub; ++j) acc[i] += q[j] * cc[j];
        }
    }
    lut[(size_t)quad * sh.entries + e] = float4{acc[0], acc[1], acc[2], acc[3]};
}

struct StackedScanArgs {
    const uint32_t *codes;        // [blocks of 64 rows][dwords][64]
    const float *xx;
    uint32_t n, chunk_rows, dwords;
    const float4 *lut;            // [quads][entries]
    const float *qq;
    uint32_t nq, entries;
    const uint32_t *eoff;         // [dwords * 4 + 1]
    const uint32_t *slab_dw;      // [slabs + 1]
    uint32_t slabs;
    int measure;
    const uint64_t *allow;
    uint32_t allow_bits;
    uint32_t k, cap_log, chunks;
    uint64_t *partial;            // [nq][chunks][k]
    float *out;                   // the distances entry: [nq][n]
};

template <uint32_t QUADS, bool SELECT>
__global__ __launch_bounds__(kStackedScanThreads) void stacked_scan_kernel(const StackedScanArgs a) {
    constexpr uint32_t NQ = QUADS * 4, RPL = kStackedRowsPerLane;
    extern __shared__ __align__(16) unsigned char stacked_lds[];
    float4 *tab = reinterpret_cast<float4 *>(stacked_lds);   // [2][kBufEntries] (one buffer when there is one slab)
    uint64_t *buf = reinterpret_cast<uint64_t *>(stacked_lds + (size_t)kStackedSlabBytes * (a.slabs > 1 ? 2 : 1));   // [NQ][1 << cap_log]
    __shared__ uint32_t s_cnt[NQ];
    __shared__ uint64_t s_thr[NQ];

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t quad0 = blockIdx.x * QUADS, chunk = blockIdx.y, slabs = a.slabs, dwords = a.dwords;
    const uint32_t c0 = chunk * a.chunk_rows;
    const uint32_t c1 = a.n - c0 < a.chunk_rows ? a.n : c0 + a.chunk_rows;
    const uint32_t rounds = (c1 - c0 + kStackedRoundRows - 1) / kStackedRoundRows, total = rounds * slabs;
    const uint32_t cap_log = a.cap_log;
    if (SELECT && tid < NQ) {
        s_cnt[tid] = 0;
        s_thr[tid] = SCANN_KEY_MAX;
    }

    const float4 zero4 = float4{0.0f, 0.0f, 0.0f, 0.0f};
    float4 pre0 = zero4, pre1 = zero4, pre2 = zero4, pre3 = zero4;
    // entries [e0, e0 + cnt) of every quad of the group: slab sl's tables, quad after quad in a buffer
    auto slab_range = [&](uint32_t sl, uint32_t *g0, uint32_t *g1, uint32_t *e0, uint32_t *cnt) {
        *g0 = uniform_load(a.slab_dw + sl);
        *g1 = uniform_load(a.slab_dw + sl + 1);
        *e0 = uniform_load(a.eoff + 4 * *g0);
        *cnt = uniform_load(a.eoff + 4 * *g1) - *e0;
    };
    // a thread's share of a slab: at most four entries, in four named registers (never an indexed array)
    auto fetch_one = [&](float4 &dst, uint32_t idx, uint32_t e0, uint32_t cnt) {
        if (idx < QUADS * cnt) {
            const uint32_t qd = idx / cnt;
            dst = a.lut[(size_t)(quad0 + qd) * a.entries + e0 + (idx - qd * cnt)];
        }
    };
    auto slab_fetch = [&](uint32_t sl) {
        uint32_t g0, g1, e0, cnt;
        slab_range(sl, &g0, &g1, &e0, &cnt);
        fetch_one(pre0, tid, e0, cnt);
        fetch_one(pre1, tid + kStackedScanThreads, e0, cnt);
        fetch_one(pre2, tid + 2 * kStackedScanThreads, e0, cnt);
        fetch_one(pre3, tid + 3 * kStackedScanThreads, e0, cnt);
        return QUADS * cnt;
    };
    auto slab_store = [&](float4 *dst, uint32_t filled) {
        if (tid < filled) dst[tid] = pre0;
        if (tid + kStackedScanThreads < filled) dst[tid + kStackedScanThreads] = pre1;
        if (tid + 2 * kStackedScanThreads < filled) dst[tid + 2 * kStackedScanThreads] = pre2;
        if (tid + 3 * kStackedScanThreads < filled) dst[tid + 3 * kStackedScanThreads] = pre3;
    };

    slab_store(tab, slab_fetch(0));
    __syncthreads();

    float4 acc[RPL][QUADS];
    uint32_t blk[RPL];
    uint32_t sl = 0, round = 0;
    for (uint32_t it = 0; it < total; ++it) {
        if (sl == 0) {
#pragma unroll
            for (uint32_t i = 0; i < RPL; ++i) {
                blk[i] = (c0 + round * kStackedRoundRows) / 64 + wave * RPL + i;
#pragma unroll
                for (uint32_t qd = 0; qd < QUADS; ++qd) acc[i][qd] = float4{0.0f, 0.0f, 0.0f, 0.0f};
            }
        }
        const bool has_next = slabs > 1 && it + 1 < total;
        uint32_t filled = 0;
        if (has_next) filled = slab_fetch(sl + 1 == slabs ? 0 : sl + 1);   // in flight while this slab is gathered

        uint32_t g0, g1, e0, cnt;
        slab_range(sl, &g0, &g1, &e0, &cnt);
        const float4 *tb = tab + (slabs > 1 ? (it & 1u) * kBufEntries : 0u);
        for (uint32_t g = g0; g < g1; ++g) {
            uint32_t dw[RPL];
#pragma unroll
            for (uint32_t i = 0; i < RPL; ++i)   // (rows past the chunk gather entry 0 and are dropped in the epilogue)
                dw[i] = (uint64_t)blk[i] * 64 < c1 ? a.codes[((size_t)blk[i] * dwords + g) * 64 + lane] : 0u;
#pragma unroll
            for (uint32_t tt = 0; tt < 4; ++tt) {
                const uint32_t base = uniform_load(a.eoff + 4 * g + tt) - e0;
#pragma unroll
                for (uint32_t i = 0; i < RPL; ++i) {
                    const uint32_t c = (dw[i] >> (8 * tt)) & 255u;
#pragma unroll
                    for (uint32_t qd = 0; qd < QUADS; ++qd) {
                        const float4 v = tb[qd * cnt + base + c];
                        acc[i][qd].x += v.x;
                        acc[i][qd].y += v.y;
                        acc[i][qd].z += v.z;
                        acc[i][qd].w += v.w;
                    }
                }
            }
        }
        if (has_next) slab_store(tab + ((it + 1) & 1u) * kBufEntries, filled);

        if (sl + 1 == slabs) {
            // ---- epilogue of the round: one row per thread and turn ------------------------------------------------
#pragma unroll
            for (uint32_t i = 0; i < RPL; ++i) {
                const uint32_t row = blk[i] * 64 + lane;
                const bool live = (uint64_t)blk[i] * 64 < c1 && row < c1;
                const float xx = live && a.measure == SCANN_HIP_SQUARED_L2 ? a.xx[row] : 0.0f;
                const bool allowed = live && (!a.allow || (row < a.allow_bits && ((a.allow[row >> 6] >> (row & 63u)) & 1ull)));
#pragma unroll
                for (uint32_t qd = 0; qd < QUADS; ++qd) {
#pragma unroll
                    for (uint32_t m = 0; m < 4; ++m) {
                        const uint32_t j = qd * 4 + m, q = quad0 * 4 + j;
                        if (!live || q >= a.nq) continue;
                        const float sum = m == 0 ? acc[i][qd].x : m == 1 ? acc[i][qd].y : m == 2 ? acc[i][qd].z : acc[i][qd].w;
                        const float d = a.measure == SCANN_HIP_SQUARED_L2 ? (a.qq[q] + xx) - 2.0f * sum : -sum;
                        if (!SELECT) {
                            a.out[(size_t)q * a.n + row] = d;
                        } else if (allowed) {
                            const uint64_t key = make_key(d, row);
                            // (the buffer has room: it held at most cap - threads keys when the turn began)
                            if (key < s_thr[j]) buf[((size_t)j << cap_log) + atomicAdd(&s_cnt[j], 1u)] = key;
                        }
                    }
                }
                if (SELECT) {
                    __syncthreads();   // the turn's appends are done
                    const int full = __syncthreads_or(tid < NQ && s_cnt[tid] > (1u << cap_log) - kStackedScanThreads);
                    if (full) sparse_compact<NQ, kStackedScanThreads>(buf, cap_log, a.k, s_cnt, s_thr);
                }
            }
        }
        __syncthreads();   // the next slab is stored; this one's readers are done
        if (++sl == slabs) {
            sl = 0;
            ++round;
        }
    }
    if (SELECT) {
        __syncthreads();
        sparse_compact<NQ, kStackedScanThreads>(buf, cap_log, a.k, s_cnt, s_thr);
        for (uint32_t i = tid; i < NQ * a.k; i += kStackedScanThreads) {
            const uint32_t j = i / a.k, ii = i - j * a.k, q = quad0 * 4 + j;
            if (q < a.nq) a.partial[((size_t)q * a.chunks + chunk) * a.k + ii] = buf[((size_t)j << cap_log) + ii];
        }
    }
}

// rows of one upload of an encode: about 256 MB of floats, whole blocks of 64
uint64_t batch_rows(uint32_t stride) {
    const uint64_t r = ((1ull << 26) / stride) & ~63ull;
    return r < 64 ? 64 : r;
}

int check_rows(const scann_hip_stacked *sq, const void *rows, uint64_t n, uint32_t stride) {
    if (n >= 0xFFFFFFFFull) return fail(SCANN_HIP_OUT_OF_RANGE, "n must be below 2^32 - 1");
    if (stride < sq->sh.dim) return fail(SCANN_HIP_INVALID_ARGUMENT, "stride is below dim");
    if (n && !rows) return fail(SCANN_HIP_INVALID_ARGUMENT, "rows is null");
    return SCANN_HIP_OK;
}

// the fused encode of host rows, batch by batch: to the caller's arrays (out_codes) or into `codes` / `xx` of a handle
int encode_rows(scann_hip_stacked *sq, const float *rows, uint64_t n, uint32_t stride, uint8_t *out_codes, float *out_res,
                DevBuf *codes, DevBuf *xx) {
    const StackedShape &sh = sq->sh;
    hipStream_t st = sq->stream;
    sq->encode_ms = 0.0f;
    const uint64_t per = batch_rows(stride);
    for (uint64_t b0 = 0; b0 < n; b0 += per) {
        const uint32_t bn = (uint32_t)(n - b0 < per ? n - b0 : per);
        const size_t floats = (size_t)(bn - 1) * stride + sh.dim;
        SCANN_TRY(sq->rows_in.ensure(floats * 4));
        SCANN_HIP_CHECK(hipMemcpyAsync(sq->rows_in.p, rows + b0 * stride, floats * 4, hipMemcpyHostToDevice, st));
        StackedEncArgs a{};
        a.sh = sh;
        a.cb = sq->cb.as<float>();
        a.rows = sq->rows_in.as<float>();
        a.n = bn;
        a.stride = stride;
        a.tile_rows = sq->tile_rows;
        if (codes) {
            a.scan_codes = codes->as<uint32_t>();
            a.xx = xx->as<float>();
            a.row_base = b0;
        } else {
            SCANN_TRY(sq->codes_io.ensure((size_t)bn * sh.T));
            SCANN_TRY(sq->res.ensure((size_t)bn * 4));
            a.out_codes = sq->codes_io.as<uint8_t>();
            a.out_res = out_res ? sq->res.as<float>() : nullptr;
        }
        SCANN_HIP_CHECK(hipEventRecord(sq->ev[0], st));
        SCANN_TRY(launch(stacked_encode_kernel, dim3(ceil_div_u32(bn, sq->tile_rows)), dim3(kStackedEncThreads),
                         stacked_enc_lds(sh.dim, sh.T, sq->tile_rows), st, a));
        SCANN_HIP_CHECK(hipEventRecord(sq->ev[1], st));
        if (!codes) {
            SCANN_HIP_CHECK(hipMemcpyAsync(out_codes + b0 * sh.T, sq->codes_io.p, (size_t)bn * sh.T, hipMemcpyDeviceToHost, st));
            if (out_res) SCANN_HIP_CHECK(hipMemcpyAsync(out_res + b0, sq->res.p, (size_t)bn * 4, hipMemcpyDeviceToHost, st));
        }
        SCANN_HIP_CHECK(hipStreamSynchronize(st));   // the batch has left rows_in
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, sq->ev[0], sq->ev[1]) == hipSuccess) sq->encode_ms += ms;
        else clear_last_hip_error();
    }
    return SCANN_HIP_OK;
}

// fresh scan-layout and norm buffers for n rows, the codes cleared (rows past n and pad bytes read as code 0)
int new_row_buffers(scann_hip_stacked *sq, uint64_t n, DevBuf *codes, DevBuf *xx) {
    const size_t bytes = (size_t)ceil_div_u64(n, 64) * sq->sh.dwords * 64 * 4;
    SCANN_TRY(codes->ensure(bytes));
    SCANN_TRY(xx->ensure(n * 4));
    SCANN_HIP_CHECK(hipMemsetAsync(codes->p, 0, codes->bytes, sq->stream));
    return SCANN_HIP_OK;
}

void adopt_rows(scann_hip_stacked *sq, uint64_t n, DevBuf *codes, DevBuf *xx) {
    sq->codes.take(*codes);
    sq->xx.take(*xx);
    sq->n = n;
    sq->has_rows = true;
}

// queries uploaded, tables built, the scan launched (with k: the selection and the merge), results copied back
int stacked_run(scann_hip_stacked *sq, const float *queries, uint32_t nq, uint32_t q_stride, uint32_t k, const uint64_t *allow,
                uint64_t allow_bits, uint32_t *out_idx, float *out_dist, uint32_t *out_count, float *out) {
    const bool select = out == nullptr;
    const StackedShape &sh = sq->sh;
    if (q_stride < sh.dim) return fail(SCANN_HIP_INVALID_ARGUMENT, "q_stride is below dim");
    if (nq && !queries) return fail(SCANN_HIP_INVALID_ARGUMENT, "queries is null");
    std::lock_guard<std::mutex> lock(sq->mu);
    if (!sq->has_rows) return fail(SCANN_HIP_FAILED_PRECONDITION, "no rows: call scann_hip_stacked_set_rows or _set_codes first");
    sq->timed = false;
    for (uint64_t &p : sq->last) p = 0;
    if (select) {   // what a search that launches nothing leaves: no rows, the halves of the all-ones key
        for (uint32_t i = 0; i < nq; ++i) out_count[i] = 0;
        for (size_t i = 0; i < (size_t)nq * k; ++i) {
            out_idx[i] = 0xFFFFFFFFu;
            out_dist[i] = ordered_to_f32(0xFFFFFFFFu);
        }
    }
    if (sq->n == 0 || nq == 0) return SCANN_HIP_OK;
    const uint32_t n = (uint32_t)sq->n;
    const uint32_t quads = nq > 4 ? kStackedMaxQuads : 1, groups = ceil_div_u32(nq, quads * 4);
    uint32_t chunk_rows = 0, chunks = 0;
    stacked_chunks(n, select ? kStackedMergeKeys / k : 65535u, &chunk_rows, &chunks);
    std::vector<uint32_t> eoff, slab_dw;
    stacked_entry_offsets(sh, &eoff);
    stacked_plan_slabs(sh, eoff, quads, &slab_dw);
    const uint32_t slabs = (uint32_t)slab_dw.size() - 1;
    if (allow_bits > n) allow_bits = n;

    SCANN_HIP_CHECK(hipSetDevice(sq->device));
    hipStream_t st = sq->stream;
    const size_t qfloats = (size_t)(nq - 1) * q_stride + sh.dim;
    SCANN_TRY(sq->queries.ensure(qfloats * 4));
    SCANN_TRY(sq->lut.ensure((size_t)groups * quads * sh.entries * 16));
    SCANN_TRY(sq->qq.ensure((size_t)groups * quads * 4 * 4));
    SCANN_TRY(sq->slab_dw.ensure(slab_dw.size() * 4));
    SCANN_HIP_CHECK(hipMemcpyAsync(sq->queries.p, queries, qfloats * 4, hipMemcpyHostToDevice, st));
    SCANN_HIP_CHECK(hipMemcpyAsync(sq->slab_dw.p, slab_dw.data(), slab_dw.size() * 4, hipMemcpyHostToDevice, st));
    const size_t allow_words = allow ? (size_t)((allow_bits + 63) / 64) : 0;
    if (allow) {
        SCANN_TRY(sq->allow.ensure(allow_words * 8));
        if (allow_words) SCANN_HIP_CHECK(hipMemcpyAsync(sq->allow.p, allow, allow_words * 8, hipMemcpyHostToDevice, st));
    }
    if (select) {
        SCANN_TRY(sq->partial.ensure((size_t)nq * chunks * k * 8));
        SCANN_TRY(sq->out_idx.ensure((size_t)nq * k * 4));
        SCANN_TRY(sq->out_dist.ensure((size_t)nq * k * 4));
        SCANN_TRY(sq->out_count.ensure((size_t)nq * 4));
    } else {
        SCANN_TRY(sq->dist.ensure((size_t)nq * n * 4));
    }
    SCANN_HIP_CHECK(hipStreamSynchronize(st));   // the pageable copies have left the host vectors

    StackedScanArgs a{};
    a.codes = sq->codes.as<uint32_t>();
    a.xx = sq->xx.as<float>();
    a.n = n;
    a.chunk_rows = chunk_rows;
    a.dwords = sh.dwords;
    a.lut = sq->lut.as<float4>();
    a.qq = sq->qq.as<float>();
    a.nq = nq;
    a.entries = sh.entries;
    a.eoff = sq->eoff.as<uint32_t>();
    a.slab_dw = sq->slab_dw.as<uint32_t>();
    a.slabs = slabs;
    a.measure = sq->measure;
    a.allow = allow ? sq->allow.as<uint64_t>() : nullptr;
    a.allow_bits = (uint32_t)allow_bits;
    a.k = k;
    a.chunks = chunks;
    a.partial = sq->partial.as<uint64_t>();
    a.out = sq->dist.as<float>();
    uint32_t cap_log = 0;
    while ((1u << cap_log) < stacked_select_cap(k)) ++cap_log;
    a.cap_log = cap_log;

    SCANN_HIP_CHECK(hipEventRecord(sq->ev[2], st));
    SCANN_TRY(launch(stacked_lut_kernel, dim3(ceil_div_u32(sh.entries, kSmallThreads), groups * quads), dim3(kSmallThreads), 0, st, sh,
                     sq->cb.as<float>(), sq->queries.as<float>(), nq, q_stride, sq->lut.as<float4>(), sq->qq.as<float>()));
    SCANN_HIP_CHECK(hipEventRecord(sq->ev[3], st));
    const dim3 grid(groups, chunks), block(kStackedScanThreads);
    const size_t lds = stacked_scan_lds(quads, k, select, slabs);
    if (quads == 1) {
        if (select) SCANN_TRY(launch(stacked_scan_kernel<1, true>, grid, block, lds, st, a));
        else SCANN_TRY(launch(stacked_scan_kernel<1, false>, grid, block, lds, st, a));
    } else {
        if (select) SCANN_TRY(launch(stacked_scan_kernel<kStackedMaxQuads, true>, grid, block, lds, st, a));
        else SCANN_TRY(launch(stacked_scan_kernel<kStackedMaxQuads, false>, grid, block, lds, st, a));
    }
    SCANN_HIP_CHECK(hipEventRecord(sq->ev[4], st));
    if (select)
        SCANN_TRY(sparse_merge(sq->partial.as<uint64_t>(), nq, chunks, k, sq->out_idx.as<uint32_t>(), sq->out_dist.as<float>(),
                               sq->out_count.as<uint32_t>(), st));
    SCANN_HIP_CHECK(hipEventRecord(sq->ev[5], st));
    if (select) {
        SCANN_HIP_CHECK(hipMemcpyAsync(out_idx, sq->out_idx.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost, st));
        SCANN_HIP_CHECK(hipMemcpyAsync(out_dist, sq->out_dist.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost, st));
        SCANN_HIP_CHECK(hipMemcpyAsync(out_count, sq->out_count.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    } else {
        SCANN_HIP_CHECK(hipMemcpyAsync(out, sq->dist.p, (size_t)nq * n * 4, hipMemcpyDeviceToHost, st));
    }
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    sq->timed = true;
    sq->last[0] = slabs;
    sq->last[1] = chunk_rows;
    sq->last[2] = chunks;
    sq->last[3] = quads;
    sq->last[4] = groups;
    return SCANN_HIP_OK;
}

}  // namespace
}  // namespace scann

using namespace scann;

extern "C" {

int scann_hip_stacked_create(scann_hip_ctx *ctx, uint32_t dim, uint32_t num_levels, const uint32_t *subspaces, const uint32_t *num_codes,
                             const float *codebooks, int measure, scann_hip_stacked **out) {
    if (!out) return fail(SCANN_HIP_INVALID_ARGUMENT, "out is null");
    *out = nullptr;
    if (!ctx) return fail(SCANN_HIP_INVALID_ARGUMENT, "context is null");
    if (!subspaces || !num_codes || !codebooks) return fail(SCANN_HIP_INVALID_ARGUMENT, "null subspaces / num_codes / codebooks");
    switch (measure) {
        case SCANN_HIP_DOT_PRODUCT:
        case SCANN_HIP_SQUARED_L2: break;
        case SCANN_HIP_L2:
        case SCANN_HIP_L1:
        case SCANN_HIP_COSINE: return fail(SCANN_HIP_UNIMPLEMENTED, "stacked handles score DotProduct and SquaredL2 only");
        default: return fail(SCANN_HIP_INVALID_ARGUMENT, "unknown measure");
    }
    std::unique_ptr<scann_hip_stacked> sq(new scann_hip_stacked());
    const char *why = "";
    const int status = stacked_shape(dim, num_levels, subspaces, num_codes, &sq->sh, &why);
    if (status != SCANN_HIP_OK) return fail(status, why);
    sq->tile_rows = stacked_tile_rows(dim, sq->sh.T);
    if (sq->tile_rows < kStackedEncMinRows) return fail(SCANN_HIP_UNIMPLEMENTED, "dim above SCANN_HIP_STACKED_MAX_DIM (4095)");
    sq->device = ctx_device(ctx);
    sq->measure = measure;
    SCANN_HIP_CHECK(hipSetDevice(sq->device));
    SCANN_HIP_CHECK(hipStreamCreateWithFlags(&sq->stream, hipStreamNonBlocking));
    for (hipEvent_t &e : sq->ev) SCANN_HIP_CHECK(hipEventCreate(&e));
    std::vector<uint32_t> eoff;
    stacked_entry_offsets(sq->sh, &eoff);
    SCANN_TRY(upload(sq->cb, codebooks, (size_t)sq->sh.cb_floats * 4));
    SCANN_TRY(upload(sq->eoff, eoff.data(), eoff.size() * 4));
    SCANN_TRY(sq->flag.ensure(4));
    *out = sq.release();
    return SCANN_HIP_OK;
}

void scann_hip_stacked_destroy(scann_hip_stacked *sq) {
    if (!sq) return;
    (void)hipSetDevice(sq->device);
    delete sq;
}

int scann_hip_stacked_encode(scann_hip_stacked *sq, const float *rows, uint64_t n, uint32_t stride, uint8_t *out_codes,
                             float *out_residual_sq) {
    if (!sq) return fail(SCANN_HIP_INVALID_ARGUMENT, "handle is null");
    SCANN_TRY(check_rows(sq, rows, n, stride));
    if (n && !out_codes) return fail(SCANN_HIP_INVALID_ARGUMENT, "out_codes is null");
    std::lock_guard<std::mutex> lock(sq->mu);
    SCANN_HIP_CHECK(hipSetDevice(sq->device));
    return encode_rows(sq, rows, n, stride, out_codes, out_residual_sq, nullptr, nullptr);
}

int scann_hip_stacked_decode(scann_hip_stacked *sq, const uint8_t *codes, uint64_t n, float *out_rows) {
    if (!sq) return fail(SCANN_HIP_INVALID_ARGUMENT, "handle is null");
    if (n >= 0xFFFFFFFFull) return fail(SCANN_HIP_OUT_OF_RANGE, "n must be below 2^32 - 1");
    if (n && (!codes || !out_rows)) return fail(SCANN_HIP_INVALID_ARGUMENT, "null codes / out_rows");
    std::lock_guard<std::mutex> lock(sq->mu);
    SCANN_HIP_CHECK(hipSetDevice(sq->device));
    const StackedShape &sh = sq->sh;
    hipStream_t st = sq->stream;
    const uint64_t per = batch_rows(sh.dim);
    SCANN_HIP_CHECK(hipMemsetAsync(sq->flag.p, 0, 4, st));
    for (uint64_t b0 = 0; b0 < n; b0 += per) {
        const uint64_t bn = n - b0 < per ? n - b0 : per, elems = bn * sh.dim;
        SCANN_TRY(sq->codes_io.ensure(bn * sh.T));
        SCANN_TRY(sq->rows_in.ensure(elems * 4));
        SCANN_HIP_CHECK(hipMemcpyAsync(sq->codes_io.p, codes + b0 * sh.T, bn * sh.T, hipMemcpyHostToDevice, st));
        SCANN_TRY(launch(stacked_decode_kernel, dim3((uint32_t)ceil_div_u64(elems, kSmallThreads)), dim3(kSmallThreads), 0, st, sh,
                         sq->cb.as<float>(), sq->codes_io.as<uint8_t>(), elems, sq->rows_in.as<float>(), sq->flag.as<uint32_t>()));
        SCANN_HIP_CHECK(hipMemcpyAsync(out_rows + b0 * sh.dim, sq->rows_in.p, elems * 4, hipMemcpyDeviceToHost, st));
        SCANN_HIP_CHECK(hipStreamSynchronize(st));
    }
    uint32_t bad = 0;
    SCANN_HIP_CHECK(hipMemcpyAsync(&bad, sq->flag.p, 4, hipMemcpyDeviceToHost, st));   // (behind the flag's clearing, n == 0 included)
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    if (bad) return fail(SCANN_HIP_INVALID_ARGUMENT, "a code is not below its level's num_codes");
    return SCANN_HIP_OK;
}

int scann_hip_stacked_set_rows(scann_hip_stacked *sq, const float *rows, uint64_t n, uint32_t stride) {
    if (!sq) return fail(SCANN_HIP_INVALID_ARGUMENT, "handle is null");
    SCANN_TRY(check_rows(sq, rows, n, stride));
    std::lock_guard<std::mutex> lock(sq->mu);
    SCANN_HIP_CHECK(hipSetDevice(sq->device));
    DevBuf codes, xx;
    SCANN_TRY(new_row_buffers(sq, n, &codes, &xx));
    SCANN_TRY(encode_rows(sq, rows, n, stride, nullptr, nullptr, &codes, &xx));
    SCANN_HIP_CHECK(hipStreamSynchronize(sq->stream));
    adopt_rows(sq, n, &codes, &xx);
    return SCANN_HIP_OK;
}

int scann_hip_stacked_set_codes(scann_hip_stacked *sq, const uint8_t *codes_in, uint64_t n) {
    if (!sq) return fail(SCANN_HIP_INVALID_ARGUMENT, "handle is null");
    if (n >= 0xFFFFFFFFull) return fail(SCANN_HIP_OUT_OF_RANGE, "n must be below 2^32 - 1");
    if (n && !codes_in) return fail(SCANN_HIP_INVALID_ARGUMENT, "codes is null");
    std::lock_guard<std::mutex> lock(sq->mu);
    SCANN_HIP_CHECK(hipSetDevice(sq->device));
    const StackedShape &sh = sq->sh;
    hipStream_t st = sq->stream;
    DevBuf codes, xx;
    SCANN_TRY(new_row_buffers(sq, n, &codes, &xx));
    SCANN_HIP_CHECK(hipMemsetAsync(sq->flag.p, 0, 4, st));
    const uint64_t per = 1ull << 22;
    for (uint64_t b0 = 0; b0 < n; b0 += per) {
        const uint32_t bn = (uint32_t)(n - b0 < per ? n - b0 : per);
        SCANN_TRY(sq->codes_io.ensure((size_t)bn * sh.T));
        SCANN_HIP_CHECK(hipMemcpyAsync(sq->codes_io.p, codes_in + b0 * sh.T, (size_t)bn * sh.T, hipMemcpyHostToDevice, st));
        SCANN_TRY(launch(stacked_set_codes_kernel, dim3(ceil_div_u32(bn, kSmallThreads)), dim3(kSmallThreads), 0, st, sh, sq->cb.as<float>(),
                         sq->codes_io.as<uint8_t>(), bn, b0, codes.as<uint32_t>(), xx.as<float>(), sq->flag.as<uint32_t>()));
        SCANN_HIP_CHECK(hipStreamSynchronize(st));
    }
    uint32_t bad = 0;
    SCANN_HIP_CHECK(hipMemcpyAsync(&bad, sq->flag.p, 4, hipMemcpyDeviceToHost, st));   // (behind the flag's clearing, n == 0 included)
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    if (bad) return fail(SCANN_HIP_INVALID_ARGUMENT, "a code is not below its level's num_codes");   // (the handle keeps its rows)
    adopt_rows(sq, n, &codes, &xx);
    return SCANN_HIP_OK;
}

int scann_hip_stacked_distances(scann_hip_stacked *sq, const float *queries, uint32_t nq, uint32_t q_stride, float *out) {
    if (!sq) return fail(SCANN_HIP_INVALID_ARGUMENT, "handle is null");
    if (!out) return fail(SCANN_HIP_INVALID_ARGUMENT, "out is null");
    return stacked_run(sq, queries, nq, q_stride, 1, nullptr, 0, nullptr, nullptr, nullptr, out);
}

int scann_hip_stacked_search_batched(scann_hip_stacked *sq, const float *queries, uint32_t nq, uint32_t q_stride, uint32_t k,
                                     const uint64_t *allow_bitmap, uint64_t allow_bitmap_bits, uint32_t *out_idx, float *out_dist,
                                     uint32_t *out_count) {
    if (!sq) return fail(SCANN_HIP_INVALID_ARGUMENT, "handle is null");
    if (k == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "k must be at least 1");
    if (k > kStackedMaxK) return fail(SCANN_HIP_INVALID_ARGUMENT, "k above SCANN_HIP_STACKED_MAX_K");
    if (nq && (!out_idx || !out_dist || !out_count)) return fail(SCANN_HIP_INVALID_ARGUMENT, "null output pointer");
    return stacked_run(sq, queries, nq, q_stride, k, allow_bitmap, allow_bitmap_bits, out_idx, out_dist, out_count, nullptr);
}

uint64_t scann_hip_stacked_size(const scann_hip_stacked *sq) { return sq ? sq->n : 0; }

void scann_hip_stacked_info(const scann_hip_stacked *sq, uint64_t *out) {
    if (!out) return;
    for (int i = 0; i < 9; ++i) out[i] = 0;
    if (!sq) return;
    out[0] = sq->sh.levels;
    out[1] = sq->sh.T;
    out[2] = sq->cb.bytes + sq->eoff.bytes + (sq->has_rows ? sq->codes.bytes + sq->xx.bytes : 0);
    out[3] = sq->tile_rows;
    for (int i = 0; i < 5; ++i) out[4 + i] = sq->last[i];
}

void scann_hip_stacked_last_kernel_ms(scann_hip_stacked *sq, float *out_ms) {
    if (!out_ms) return;
    out_ms[0] = out_ms[1] = out_ms[2] = out_ms[3] = 0.0f;
    if (!sq) return;
    std::lock_guard<std::mutex> lock(sq->mu);
    out_ms[0] = sq->encode_ms;
    if (!sq->timed) return;
    for (int i = 0; i < 3; ++i) {
        if (hipEventElapsedTime(&out_ms[1 + i], sq->ev[2 + i], sq->ev[3 + i]) != hipSuccess) {
            clear_last_hip_error();
            out_ms[1 + i] = 0.0f;
        }
    }
}

}  // extern "C"

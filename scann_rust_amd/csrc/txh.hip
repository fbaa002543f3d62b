// txh.hip -- HIP kernels of the Tree-X-Hybrid / AsymmetricHasher search path (gfx950).
//
// Pipeline per query batch (reference: tree_x_hybrid/mod.rs:245-364):
//   centroid_scores -> select_leaves            TreePartitioner::partition            (K1: txh_partition.hip)
//   count/scan/fill worklist                    (groups (query, leaf) pairs by leaf)  (txh_partition.hip)
//   lut_build                                   residual + LookupTable::from_query    (txh_partition.hip)
//   sample_threshold                            valid upper bound of the m-th best key
//   adc_scan (dominant, LDS-staged LUT16)       LookupTable::compute_distance + FastTopNeighbors
//   select_rerank                               merge/sort/truncate + reorder_results
//
// All arithmetic that the reference performs in a fixed order is performed in the same
// order here; this file is compiled with -ffp-contract=off and uses fmaf() only where
// the reference uses _mm256_fmadd_ps.
#include <type_traits>

#include "launch.h"
#include "pair.h"
#include "txh_dev.h"
#include "txh_stages.h"

namespace scann {

// =====================================================================================
// K2: select leaves.  tree_partitioner.rs:206-228: stable sort of ALL L (dist, id) by
// OrderedFloat(dist), take the first P.  Key = (ordered(dist) << 32 | id) makes the
// stable order explicit; NaN sorts last as OrderedFloat does.
// =====================================================================================
// centers_inline != nullptr (small batches): the block scores the centroids itself first, with
// centroid_scores_kernel's arithmetic (sequential scalar sum of (q_j - c_j)^2, no FMA), instead of reading
// a matrix another launch produced.
// Bin of 1-based rank `rank` in a complete histogram of `bins` bins (1024 or 4096) in LDS (counts synchronised by the caller; the
// histogram holds >= rank entries); s_w[49] = the rank inside that bin.  Every thread of an NT-thread block calls; two
// barriers; s_w: LDS u32[>= 50].
template <uint32_t NT = kSelectThreads>
__device__ __forceinline__ uint32_t block_hist_rank_bin(const uint32_t *s_hist, uint32_t *s_w, uint32_t rank,
                                                        uint32_t bins = kSelBinsMax) {
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t per = bins / NT;   // bins per thread (1 or 4; 8 with 512 threads)
    uint32_t mine = 0;
    for (uint32_t j = 0; j < per; ++j) mine += s_hist[tid * per + j];
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
        if ((int)lane >= o) incl += up;
    }
    if (lane == 63) s_w[32 + wave] = incl;
    __syncthreads();
    uint32_t wbase = 0;
    for (uint32_t w2 = 0; w2 < wave; ++w2) wbase += s_w[32 + w2];
    incl += wbase;
    const uint32_t excl = incl - mine;
    if (excl < rank && rank <= incl) {   // exactly one thread
        uint32_t c = excl;
        for (uint32_t j = 0; j < per; ++j) {
            const uint32_t h = s_hist[tid * per + j];
            if (c + h >= rank) {
                s_w[48] = tid * per + j;
                s_w[49] = rank - c;   // 1-based rank inside the bin
                break;
            }
            c += h;
        }
    }
    __syncthreads();
    return s_w[48];
}

// The kernel's body: also the first stage of small_fused_kernel, where EVERY workgroup of a query runs it
// (write_out: only one of them stores the global outputs; s_tok_out / s_vb_out: LDS copies of the tokens
// and the P + 1 key bases for the stages that follow in the same workgroup).
__device__ __forceinline__ void select_leaves_body(
    uint64_t *skeys, uint32_t q, bool write_out, uint32_t *s_tok_out, uint32_t *s_vb_out,
    float *__restrict__ cdist, uint32_t L, uint32_t n_pow2, uint32_t P, uint32_t p_pow2,
    const uint32_t *__restrict__ leaf_gsize, const uint32_t *__restrict__ leaf_off, uint32_t st,
    uint32_t *__restrict__ tokens, float *__restrict__ token_dists, uint32_t *__restrict__ vbase,
    uint32_t *__restrict__ sbase, const float *__restrict__ centers_inline, const float *__restrict__ queries,
    uint32_t q_stride, uint32_t dim, uint32_t centers_pitch) {
    uint64_t *s_top = skeys + n_pow2;                                   // [p_pow2] (select path)
    const SelCfg cfg = sel_cfg(L);
    uint32_t *s_hist = reinterpret_cast<uint32_t *>(s_top + p_pow2);    // [cfg.bins]
    uint64_t *s_list = reinterpret_cast<uint64_t *>(s_hist + cfg.bins); // [cfg.list]
    uint64_t *s_red = s_list + cfg.list;                                // [48]
    uint32_t *s_scan = reinterpret_cast<uint32_t *>(s_red + 48);        // [3][kSelectThreads / 64] + cursor
    const uint32_t tid = threadIdx.x, nt = blockDim.x;
    const uint32_t lane = tid & 63u, wave = tid >> 6, nwaves = nt >> 6;
    const bool select_path = p_pow2 != 0;
    const uint32_t nfill = select_path ? L : n_pow2;
    // inline mode (small batches): the leaf size tables of this index live in LDS behind the scan words,
    // so nothing after the scoring waits on global memory
#ifdef SCANN_WIDE_TIMING
    uint64_t tl[6];
    tl[0] = wall_clock64();
#endif
    uint32_t *s_lsz = s_scan + 64, *s_lgs = s_lsz + (centers_inline ? L : 0u);
    float *s_qv = reinterpret_cast<float *>((reinterpret_cast<uintptr_t>(s_lgs + (centers_inline ? L : 0u)) + 15u) & ~(uintptr_t)15u);
    if (centers_inline) {
        // centers_inline is the TRANSPOSED centroid matrix [dim][centers_pitch]: thread c reads element
        // (j, c), so a wave's load covers two cache lines instead of 64 (row-major rows made the kernel
        // wait on the L1's line-request rate: 15 us for 1000 x 128 centroids).  16 loads in flight; the sum is
        // the reference's sequential one.
        for (uint32_t j = tid; j < dim; j += nt) s_qv[j] = queries[(size_t)q * q_stride + j];
        for (uint32_t l = tid; l < L; l += nt) {
            s_lsz[l] = leaf_off[l + 1] - leaf_off[l];
            s_lgs[l] = leaf_gsize[l];
        }
        __syncthreads();
        for (uint32_t c = tid; c < L; c += nt) {
            const float *col = centers_inline + c;
            float acc = 0.0f;
            for (uint32_t j0 = 0; j0 < dim; j0 += 64) {   // 64 loads in flight: one memory round trip per 64 dims
                float cv[64];
#pragma unroll
                for (int u = 0; u < 64; ++u)
                    cv[u] = j0 + (uint32_t)u < dim ? col[(size_t)(j0 + u) * centers_pitch] : 0.0f;
#pragma unroll
                for (int u = 0; u < 64; ++u)
                    if (j0 + (uint32_t)u < dim) {
                        const float d = s_qv[j0 + u] - cv[u];
                        acc = acc + d * d;
                    }
            }
            if (write_out) cdist[(size_t)q * L + c] = acc;   // (kept for NaN payloads: see token_dists below)
            skeys[c] = ((uint64_t)((acc != acc) ? 0xFFFFFFFFu : f32_to_ordered(acc)) << 32) | c;
        }
        for (uint32_t i = L + tid; i < nfill; i += nt) skeys[i] = SCANN_KEY_MAX;
    } else {
        for (uint32_t i = tid; i < nfill; i += nt) {
            uint64_t key = SCANN_KEY_MAX;
            if (i < L) {
                float d = cdist[(size_t)q * L + i];
                uint32_t o = (d != d) ? 0xFFFFFFFFu : f32_to_ordered(d);
                key = ((uint64_t)o << 32) | i;
            }
            skeys[i] = key;
        }
    }
#ifdef SCANN_WIDE_TIMING
    tl[1] = wall_clock64();
#endif
    __syncthreads();
    const uint64_t *sorted = skeys;
#ifdef SCANN_WIDE_TIMING
    tl[2] = tl[3] = wall_clock64();
#endif
    if (select_path) {
        // P << L: the P-th smallest key by histogram select, then sort only the P survivors
        // (keys are unique: exactly P of them are <= the P-th smallest)
        // (Tried for P <= 16: per-wave tournaments of 64-bit wave minima, P rounds per wave and P over the finalists,
        // which also yields the sorted order -- 12 cross-lane shuffles per round, no faster than this.)
        const uint64_t T = block_select<uint64_t>(skeys, L, P, cfg, s_hist, s_list, s_red);
        for (uint32_t i = tid; i < p_pow2; i += nt) s_top[i] = SCANN_KEY_MAX;
        if (tid == 0) s_scan[48] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < L; i += nt) {
            const uint64_t key = skeys[i];
            if (key <= T) s_top[atomicAdd(&s_scan[48], 1u)] = key;
        }
        __syncthreads();
#ifdef SCANN_WIDE_TIMING
        tl[3] = wall_clock64();
#endif
        bitonic_sort_lds(s_top, p_pow2);
        sorted = s_top;
    } else {
        bitonic_sort_lds(skeys, n_pow2);
    }
#ifdef SCANN_WIDE_TIMING
    tl[4] = wall_clock64();
#endif
    for (uint32_t r = tid; r < P; r += nt) {
        uint64_t key = sorted[r];
        uint32_t id = (uint32_t)key;
        if (s_tok_out) s_tok_out[r] = id;
        if (write_out) {
            tokens[(size_t)q * P + r] = id;
            // inline mode: the distance is the key's high word (a NaN keeps its payload through cdist)
            const uint32_t ob = (uint32_t)(key >> 32);
            token_dists[(size_t)q * P + r] = (centers_inline && ob != 0xFFFFFFFFu) ? ordered_to_f32(ob)
                                                                                  : cdist[(size_t)q * L + id];
        }
    }
    // exclusive prefixes over the P tokens: global leaf sizes (merge-key base), sample counts
    // (every st-th local point of each selected leaf) and local points
    const uint32_t per = (P + nt - 1) / nt;
    const uint32_t r0 = min(P, tid * per), r1 = min(P, r0 + per);
    uint32_t a_g = 0, a_s = 0, a_t = 0;
    for (uint32_t r = r0; r < r1; ++r) {
        const uint32_t leaf = (uint32_t)sorted[r];
        const uint32_t sz = centers_inline ? s_lsz[leaf] : leaf_off[leaf + 1] - leaf_off[leaf];
        a_g += centers_inline ? s_lgs[leaf] : leaf_gsize[leaf];
        a_s += (sz + st - 1) / st;
        a_t += sz;
    }
    uint32_t i_g = a_g, i_s = a_s, i_t = a_t;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u_g = (uint32_t)__shfl_up((int)i_g, o), u_s = (uint32_t)__shfl_up((int)i_s, o),
                       u_t = (uint32_t)__shfl_up((int)i_t, o);
        if ((int)lane >= o) {
            i_g += u_g;
            i_s += u_s;
            i_t += u_t;
        }
    }
    if (lane == 63) {
        s_scan[wave] = i_g;
        s_scan[16 + wave] = i_s;
        s_scan[32 + wave] = i_t;
    }
    __syncthreads();
    uint32_t b_g = 0, b_s = 0, t_g = 0, t_s = 0, t_t = 0;
    for (uint32_t w2 = 0; w2 < nwaves; ++w2) {
        if (w2 < wave) {
            b_g += s_scan[w2];
            b_s += s_scan[16 + w2];
        }
        t_g += s_scan[w2];
        t_s += s_scan[16 + w2];
        t_t += s_scan[32 + w2];
    }
    uint32_t vb = b_g + i_g - a_g, sb = b_s + i_s - a_s;
    for (uint32_t r = r0; r < r1; ++r) {
        const uint32_t leaf = (uint32_t)sorted[r];
        const uint32_t sz = centers_inline ? s_lsz[leaf] : leaf_off[leaf + 1] - leaf_off[leaf];
        if (s_vb_out) s_vb_out[r] = vb;
        if (write_out) {
            vbase[(size_t)q * (P + 1) + r] = vb;
            sbase[(size_t)q * (P + 2) + r] = sb;
        }
        vb += centers_inline ? s_lgs[leaf] : leaf_gsize[leaf];
        sb += (sz + st - 1) / st;
    }
    if (tid == 0) {
        if (s_vb_out) s_vb_out[P] = t_g;
        if (write_out) {
            vbase[(size_t)q * (P + 1) + P] = t_g;
            sbase[(size_t)q * (P + 2) + P] = t_s;
            sbase[(size_t)q * (P + 2) + P + 1] = t_t;
        }
    }
#ifdef SCANN_WIDE_TIMING
    tl[5] = wall_clock64();
    if (tid == 0 && write_out && q == 0) printf("leaves: score %.2f sync %.2f select %.2f sort %.2f prefix %.2f us\n", (tl[1] - tl[0]) * 0.01, (tl[2] - tl[1]) * 0.01, (tl[3] - tl[2]) * 0.01, (tl[4] - tl[3]) * 0.01, (tl[5] - tl[4]) * 0.01);
#endif
}

__global__ __launch_bounds__(kSelectThreads) void select_leaves_kernel(
    float *__restrict__ cdist, uint32_t L, uint32_t n_pow2, uint32_t P, uint32_t p_pow2,
    const uint32_t *__restrict__ leaf_gsize, const uint32_t *__restrict__ leaf_off, uint32_t st,
    uint32_t *__restrict__ tokens, float *__restrict__ token_dists, uint32_t *__restrict__ vbase,
    uint32_t *__restrict__ sbase, const float *__restrict__ centers_inline, const float *__restrict__ queries,
    uint32_t q_stride, uint32_t dim, uint32_t centers_pitch) {
    extern __shared__ __attribute__((aligned(16))) uint64_t skeys[];    // [n_pow2] ...
    select_leaves_body(skeys, blockIdx.x, true, nullptr, nullptr, cdist, L, n_pow2, P, p_pow2, leaf_gsize, leaf_off, st,
                       tokens, token_dists, vbase, sbase, centers_inline, queries, q_stride, dim, centers_pitch);
}

// =====================================================================================
// K6: ADC scan -- the dominant kernel.  hashes/lut.rs:74-82 driven by the loop at
// tree_x_hybrid/mod.rs:324-336 / hashes/hasher.rs:179-182.
//
// A tile = (leaf, chunk of kScanTP points, group of <= kScanQuadsPerTile query quads).
// Each lane keeps the packed codes of PPT points in VGPRs (coalesced 16-B loads), and
// for every quad reads one ds_read_b128 per (point, subspace): the 16-entry table of a
// subspace is 16 x 16 B = all 64 LDS banks, lanes with equal codes broadcast, so the
// gather is conflict-free.  Distances are accumulated in subspace order (bit-exact with
// the reference) and compared with the per-query threshold; survivors are appended to
// the query's candidate list.  Tiles are pulled from an atomic queue so ragged leaves
// balance across the 256 CUs.
// =====================================================================================
// Points G .. G+NP-1 of the lane against the quad's tables.
template <typename C, int NP, int BUF, int G>
__device__ __forceinline__ void scan_quad_compute(const float4 *lut_base,
                                                  uint32_t (&regs)[C::PPT][C::REGS],
                                                  float (&acc)[4][C::PPT]) {
    constexpr int S = C::S;
    const char *lb = reinterpret_cast<const char *>(lut_base + BUF * C::LUT4);
    // The byte extractions below are invariant across the quad loop; without this
    // (instruction-free) barrier LICM hoists all S*NP of them into registers and spills.
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int ri = 0; ri < C::REGS; ++ri) asm volatile("" : "+v"(regs[G + i][ri]));
    // Software pipeline, kScanDepth subspaces deep: the NP ds_read_b128 of subspaces
    // s+1 .. s+D are in flight while subspace s is accumulated.  sched_barrier(0) pins the
    // stage order so the scheduler cannot hoist every gather to the top (256 VGPRs,
    // occupancy 1).
    constexpr int D = (int)kScanDepth;
    float4 v[D + 1][NP];
    auto issue = [&](int s, int slot) {
#pragma unroll
        for (int i = 0; i < NP; ++i)
            v[slot][i] = *reinterpret_cast<const float4 *>(lb + s * C::SUB_BYTES + C::offset(regs[G + i], s));
    };
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (d < S) issue(d, d);
#pragma unroll
    for (int s = 0; s < S; ++s) {
        if (s + D < S) issue(s + D, (s + D) % (D + 1));
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const float4 t = v[s % (D + 1)][i];
            if (s == 0) {
                acc[0][G + i] = t.x; acc[1][G + i] = t.y; acc[2][G + i] = t.z; acc[3][G + i] = t.w;
            } else {
                acc[0][G + i] = acc[0][G + i] + t.x;
                acc[1][G + i] = acc[1][G + i] + t.y;
                acc[2][G + i] = acc[2][G + i] + t.z;
                acc[3][G + i] = acc[3][G + i] + t.w;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <typename C, int BUF>
__device__ __forceinline__ void scan_quad_dispatch(const float4 *lut_s, uint32_t nsub,
                                                   uint32_t (&regs)[C::PPT][C::REGS],
                                                   float (&acc)[4][C::PPT]) {
    if constexpr (C::PPT <= 2) {
        switch (nsub) {
            case 1: scan_quad_compute<C, 1, BUF, 0>(lut_s, regs, acc); break;
            default: scan_quad_compute<C, (C::PPT < 2 ? 1 : 2), BUF, 0>(lut_s, regs, acc); break;
        }
    } else {   // pairs of points; a pair past nsub is skipped (wave-uniform)
        static_assert(C::PPT == 8, "point-pair groups are spelled out for 8 points per thread");
        scan_quad_compute<C, 2, BUF, 0>(lut_s, regs, acc);
        if (nsub > 2) scan_quad_compute<C, 2, BUF, 2>(lut_s, regs, acc);
        if (nsub > 4) scan_quad_compute<C, 2, BUF, 4>(lut_s, regs, acc);
        if (nsub > 6) scan_quad_compute<C, 2, BUF, 6>(lut_s, regs, acc);
    }
}

#ifndef SCANN_SCAN_STAGE
#define SCANN_SCAN_STAGE 128
#endif
constexpr uint32_t kScanStage = SCANN_SCAN_STAGE;   // LDS-staged survivors per (quad, query); <= kScanThreads
static_assert(kScanStage <= kScanThreads, "the flush copies one survivor per thread");

struct ScanArgs {
    const uint32_t *pair_off, *tile_off, *pair_q, *pair_vbase;
    uint32_t *counters;
    const float *lutq;
    const uint64_t *pair_thr;
    uint32_t *cand_cnt;
    uint64_t *cand;
    uint32_t cap;
    uint32_t qpt;            // query quads per tile
    uint32_t res_cl;         // resident-table kernel: chunks per tile
    const uint64_t *allow;   // optional allow-bitmap (device), bit = datapoint index
    uint64_t allow_bits;
};

// LDS of the scan kernels (dynamic: two LUT buffers first, 16-byte aligned)
template <typename C>
__host__ __device__ constexpr size_t scan_lds_bytes() {
    return (size_t)2 * C::LUT4 * 16 + (size_t)2 * 4 * kScanStage * 8 + 8 * 4 + 3 * 4 * 4 + 16;
}

template <typename C>
__device__ __forceinline__ void adc_scan_body(TxhIndexDev ix, ScanArgs a, const uint64_t allow_stride) {
    constexpr int LUT4 = C::LUT4;                                   // float4 per quad
    constexpr int STG = (LUT4 + kScanThreads - 1) / kScanThreads;   // staged float4 / thread
    extern __shared__ __attribute__((aligned(16))) float4 lut_s[];  // [2 * LUT4]
    // Survivors are staged per (quad, query) in LDS and flushed one quad later with ONE
    // returning global atomic per query, issued before the next quad's gather so its
    // latency hides under the compute (a per-lane returning atomic stalls the wave ~1 us).
    uint64_t (*ckey_s)[4][kScanStage] = reinterpret_cast<uint64_t (*)[4][kScanStage]>(lut_s + 2 * LUT4);
    uint32_t (*ccnt_s)[4] = reinterpret_cast<uint32_t (*)[4]>(ckey_s + 2);   // live counters (LDS atomics)
    uint32_t *cfrozen_s = reinterpret_cast<uint32_t *>(ccnt_s + 2);            // counts of the buffer being flushed
    uint32_t *cbase_s = cfrozen_s + 4;                                         // its global base slots
    uint32_t *cq_s = cbase_s + 4;                                              // its query ids
    uint32_t &tile_sh = cq_s[4];
    const uint32_t tid = threadIdx.x;
    const uint32_t total_tiles = a.counters[CNT_TOTAL_TILES];
    if (tid < 8) ccnt_s[tid >> 2][tid & 3u] = 0;

    for (;;) {
        if (tid == 0) tile_sh = grab_tile(a.counters + CNT_XQ, total_tiles);
        __syncthreads();
        const uint32_t tile = __builtin_amdgcn_readfirstlane(tile_sh);
        if (tile == kInvalid) break;

        const WorkItem item = decode_item(ix, a.tile_off, a.pair_off, tile);
        const uint32_t lb = item.lb, size = item.size, local = item.local, slot0 = item.slot0, slot_end = item.slot_end;
        const uint32_t nchunks = (size + (uint32_t)C::TP - 1) / (uint32_t)C::TP;
        const uint32_t chunk = local % nchunks, qg = local / nchunks;
        const uint32_t nquads = (slot_end - slot0) >> 2;
        const uint32_t q0 = qg * a.qpt;
        const uint32_t q1 = min(q0 + a.qpt, nquads);
        const uint32_t c0 = chunk * (uint32_t)C::TP;
        const uint32_t npts = min((uint32_t)C::TP, size - c0);
        const uint32_t nsub = (npts + kScanThreads - 1) / kScanThreads;

        // packed codes of this lane's points in the codec's register form
        uint32_t regs[C::PPT][C::REGS];
#pragma unroll
        for (int i = 0; i < C::PPT; ++i) {
            const uint32_t j = c0 + tid + kScanThreads * i;
            uint32_t w[C::NWORDS];
            C::load_words(ix.codes + (size_t)(lb + (j < size ? j : 0)) * C::NWORDS, w);
            C::unpack(w, regs[i]);
        }

        const float4 *gl = reinterpret_cast<const float4 *>(a.lutq) +
                           (size_t)((slot0 >> 2) + q0) * LUT4;
        // stage the first quad's LUT
        {
            float4 r[STG];
#pragma unroll
            for (int t = 0; t < STG; ++t) {
                uint32_t e = tid + t * kScanThreads;
                if (e < (uint32_t)LUT4) r[t] = gl[e];
            }
#pragma unroll
            for (int t = 0; t < STG; ++t) {
                uint32_t e = tid + t * kScanThreads;
                if (e < (uint32_t)LUT4) lut_s[e] = r[t];
            }
        }
        // wave-uniform filter parameters of a quad (SGPRs via s_load): query, key base, bound
        uint32_t f_pq[4], f_vb[4], f_thi[4], f_tlo[4];
        auto fetch_params = [&](uint32_t qd) {
            const uint32_t slot = slot0 + qd * 4;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                f_pq[p] = uniform_load(a.pair_q + slot + p);
                f_vb[p] = uniform_load(a.pair_vbase + slot + p);
                const uint64_t T = uniform_load(a.pair_thr + slot + p);
                f_thi[p] = (uint32_t)(T >> 32);
                f_tlo[p] = (uint32_t)T;
            }
        };
        if (q0 < q1) fetch_params(q0);
        __syncthreads();

        for (uint32_t qd = q0; qd <= q1; ++qd) {   // one extra trip flushes the last quad
            const uint32_t buf = (qd - q0) & 1u;
            const bool live = qd < q1;
            const bool more = qd + 1 < q1;
            const bool flush = qd > q0;             // buffer buf^1 holds quad qd-1's survivors
            // A. reserve global slots for the previous quad's survivors (not waited for yet)
            uint32_t gbase = 0, gq = kInvalid, gn = 0;
            if (flush && tid < 4) {
                gn = min(ccnt_s[buf ^ 1u][tid], kScanStage);
                gq = a.pair_q[slot0 + (qd - 1) * 4 + tid];
                if (gn) gbase = atomicAdd(&a.cand_cnt[gq], gn);
            }
            // A2. prefetch the next quad's LUT straight into the idle LDS buffer (LDS-DMA:
            // no VGPR staging; destination = wave-uniform base + lane * 16).
            if (more) {
                const float4 *g2 = gl + (size_t)(qd + 1 - q0) * LUT4;
#pragma unroll
                for (int t = 0; t < STG; ++t) {
                    const uint32_t e0 = (tid & ~63u) + t * kScanThreads;   // wave-uniform
                    if (e0 < (uint32_t)LUT4)
                        __builtin_amdgcn_global_load_lds(
                            (const __attribute__((address_space(1))) void *)(g2 + e0 + (tid & 63u)),
                            (__attribute__((address_space(3))) void *)(&lut_s[(buf ^ 1u) * LUT4 + e0]),
                            16, 0, 0);
                }
            }

            if (live) {
                // B. gather + accumulate
                float acc[4][C::PPT];
                if (buf == 0) scan_quad_dispatch<C, 0>(lut_s, nsub, regs, acc);
                else scan_quad_dispatch<C, 1>(lut_s, nsub, regs, acc);
                // threshold filter: survivors go to the LDS stage of this quad
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const uint32_t pq = f_pq[p];
                    if (pq == kInvalid) continue;   // wave-uniform
                    const uint64_t T = ((uint64_t)f_thi[p] << 32) | f_tlo[p];
                    const uint32_t Thi = f_thi[p];
                    const float Tf = (Thi == 0xFFFFFFFFu) ? __builtin_inff() : ordered_to_f32(Thi);
                    const uint32_t vb = f_vb[p];
#pragma unroll
                    for (int i = 0; i < C::PPT; ++i) {
                        if (i < (int)nsub && acc[p][i] <= Tf) {
                            const uint32_t j = c0 + tid + kScanThreads * i;
                            if (j < size) {
                                const uint64_t key = make_key(acc[p][i], vb + j);
                                if (key <= T && row_allowed(ix, a.allow, allow_stride, pq, a.allow_bits, lb + j)) {
                                    const uint32_t sl = atomicAdd(&ccnt_s[buf][p], 1u);
                                    if (sl < kScanStage) {
                                        ckey_s[buf][p][sl] = key;
                                    } else {   // stage full: direct (slow) append
                                        const uint32_t pos = atomicAdd(&a.cand_cnt[pq], 1u);
                                        if (pos < a.cap) a.cand[(size_t)pq * a.cap + pos] = key;
                                    }
                                }
                            }
                        }
                    }
                }
            }
            // A3. the next quad's filter parameters (in flight across the barrier below)
            if (more) fetch_params(qd + 1);

            // C. publish the flush parameters, reset the flushed buffer's live counters
            if (tid < 4) {
                cfrozen_s[tid] = gn;
                cbase_s[tid] = gbase;
                cq_s[tid] = gq;
                if (flush) ccnt_s[buf ^ 1u][tid] = 0;
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the LDS-DMA prefetch has landed
            __syncthreads();
            // D. copy the previous quad's survivors to the per-query candidate lists
            if (flush) {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const uint32_t n_p = cfrozen_s[p];
                    if (tid < n_p) {
                        const uint32_t pos = cbase_s[p] + tid;
                        if (pos < a.cap) a.cand[(size_t)cq_s[p] * a.cap + pos] = ckey_s[buf ^ 1u][p][tid];
                    }
                }
            }
            __syncthreads();
        }
    }
}
// One bitmap for the batch, or none: the kernel every search without allow_bitmap_stride runs (its code is that of the
// body with the stride folded to 0).  _pq: one bitmap per query, allow_stride words apart.
template <typename C>
__global__ __launch_bounds__(kScanThreads, C::WGS) void adc_scan_kernel(TxhIndexDev ix, ScanArgs a) {
    adc_scan_body<C>(ix, a, 0);
}
template <typename C>
__global__ __launch_bounds__(kScanThreads, C::WGS) void adc_scan_pq_kernel(TxhIndexDev ix, ScanArgs a, uint64_t allow_stride) {
    adc_scan_body<C>(ix, a, allow_stride);
}

// =====================================================================================
// K6b: ADC scan with RESIDENT tables, for long leaves (AsymmetricHasher mode, big partitions).
//
// adc_scan_kernel above re-stages a quad's table for every 512-point chunk and synchronises
// the workgroup twice per quad.  Here a tile = (leaf, kResQuads quads, a RANGE of chunks): the
// quads' tables are loaded into LDS once per tile and stay read-only while the workgroup (8
// waves) walks the chunk range, so the steady state has NO workgroup barrier and no table
// traffic: waves drift freely and the LDS gather and the VALU adds of different waves overlap.
// Survivors are staged per WAVE (kResStage slots per (wave, query), double-buffered by chunk):
// the wave reserves global slots for chunk c-1's survivors with one returning atomic per query
// issued BEFORE chunk c's gather and writes them out after it, so the atomic's latency hides
// under the compute.  Arithmetic, keys and the filter are those of adc_scan_kernel.
// =====================================================================================
constexpr uint32_t kResStage = 8;      // staged survivors per (wave, query, chunk)

template <typename C>
__host__ __device__ constexpr size_t res_lds_bytes() {
    return (size_t)kResQuads * C::LUT4 * 16 + (size_t)(kResThreads / 64) * 2 * kResQuads * 4 * kResStage * 8 +
           (size_t)(kResThreads / 64) * 2 * kResQuads * 4 * 4 + kResQuads * 4 * 4 + 16;
}

template <typename C>
__global__ __launch_bounds__(kResThreads, 6) void adc_scan_res_kernel(TxhIndexDev ix, ScanArgs a) {
    // (PqCodec<C>: one bitmap per query; the launch packs the stride next to the capacity, see pq_allow_bits)
    constexpr bool PQ = C::PQ;
    const uint64_t allow_bits = pq_capacity<PQ>(a.allow_bits), allow_stride = pq_stride<PQ>(a.allow_bits);
    static_assert(C::PPT == 2, "resident-table scan: 2 points per thread");
    constexpr int LUT4 = C::LUT4;
    constexpr int NQS = kResQuads * 4;                                   // resident (query, leaf) pairs
    constexpr int NWV = kResThreads / 64;
    constexpr uint32_t TPR = kResThreads * C::PPT;                       // points per chunk
    extern __shared__ __attribute__((aligned(16))) float4 lut_s[];       // [kResQuads * LUT4]
    uint64_t (*skey)[2][NQS][kResStage] =
        reinterpret_cast<uint64_t (*)[2][NQS][kResStage]>(lut_s + kResQuads * LUT4);   // [NWV]
    uint32_t (*scnt)[2][NQS] = reinterpret_cast<uint32_t (*)[2][NQS]>(skey + NWV);      // [NWV]
    uint32_t *sq = reinterpret_cast<uint32_t *>(scnt + NWV);                             // [NQS] query ids
    uint32_t &tile_sh = sq[NQS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t total_tiles = a.counters[CNT_TOTAL_TILES];

    for (;;) {
        __syncthreads();                       // the previous tile's table reads are done
        if (tid == 0) tile_sh = grab_tile(a.counters + CNT_XQ, total_tiles);
        __syncthreads();
        const uint32_t tile = __builtin_amdgcn_readfirstlane(tile_sh);
        if (tile == kInvalid) break;

        const WorkItem item = decode_item(ix, a.tile_off, a.pair_off, tile);
        const uint32_t lb = item.lb, size = item.size, local = item.local, slot0 = item.slot0, slot_end = item.slot_end;
        const uint32_t nchunks = (size + TPR - 1) / TPR;
        const uint32_t nranges = (nchunks + a.res_cl - 1) / a.res_cl;
        const uint32_t range = local % nranges, qg = local / nranges;
        const uint32_t nquads = (slot_end - slot0) >> 2;
        const uint32_t q0 = qg * kResQuads;
        const uint32_t nq_t = min(kResQuads, nquads - q0);       // resident quads of this tile
        const uint32_t c_begin = range * a.res_cl, c_end = min(nchunks, c_begin + a.res_cl);

        // tables of the tile's quads -> LDS (LDS-DMA, destination = wave-uniform base + lane * 16)
        {
            const float4 *gl = reinterpret_cast<const float4 *>(a.lutq) + (size_t)((slot0 >> 2) + q0) * LUT4;
            const uint32_t n4 = nq_t * LUT4;
            for (uint32_t e0 = (tid & ~63u); e0 < n4; e0 += kResThreads)
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void *)(gl + e0 + lane),
                    (__attribute__((address_space(3))) void *)(&lut_s[e0]), 16, 0, 0);
        }
        if (tid < (uint32_t)NQS) sq[tid] = tid < nq_t * 4 ? a.pair_q[slot0 + q0 * 4 + tid] : kInvalid;
        if (lane < (uint32_t)NQS) {
            scnt[wave][0][lane] = 0;
            scnt[wave][1][lane] = 0;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();

        // this lane's slot of the wave-level flush: pair j = lane (lanes 0 .. NQS-1)
        const uint32_t my_q = lane < (uint32_t)NQS ? sq[lane] : kInvalid;
        uint32_t raw[C::PPT][C::NWORDS];
        auto fetch_codes = [&](uint32_t c) {
#pragma unroll
            for (int i = 0; i < C::PPT; ++i) {
                const uint32_t j = c * TPR + tid + kResThreads * i;
                C::load_words(ix.codes + (size_t)(lb + (j < size ? j : 0)) * C::NWORDS, raw[i]);
            }
        };
        fetch_codes(c_begin);
        for (uint32_t c = c_begin; c <= c_end; ++c) {      // one extra trip flushes the last chunk
            const uint32_t buf = (c - c_begin) & 1u;
            const bool live = c < c_end;
            const bool flush = c > c_begin;                // stage buf^1 holds chunk c-1's survivors
            uint32_t regs[C::PPT][C::REGS];
            if (live) {
#pragma unroll
                for (int i = 0; i < C::PPT; ++i) C::unpack(raw[i], regs[i]);
                if (c + 1 < c_end) fetch_codes(c + 1);     // in flight during this chunk's gathers
            }
            // A. reserve global slots for the previous chunk's survivors (result used in C)
            uint32_t fcnt = 0, fbase = 0;
            if (flush && my_q != kInvalid) {
                fcnt = min(scnt[wave][buf ^ 1u][lane], kResStage);
                if (fcnt) fbase = atomicAdd(&a.cand_cnt[my_q], fcnt);
            }
            // B. gather + accumulate + filter, quad after quad against the resident tables
            if (live) {
                const uint32_t c0 = c * TPR;
                const uint32_t npts = min(TPR, size - c0);
                const uint32_t nsub = (npts + kResThreads - 1) / kResThreads;
                for (uint32_t qd = 0; qd < nq_t; ++qd) {
                    const uint32_t slot = slot0 + (q0 + qd) * 4;
                    uint32_t f_pq[4], f_vb[4], f_thi[4], f_tlo[4];
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        f_pq[p] = uniform_load(a.pair_q + slot + p);
                        f_vb[p] = uniform_load(a.pair_vbase + slot + p);
                        const uint64_t T = uniform_load(a.pair_thr + slot + p);
                        f_thi[p] = (uint32_t)(T >> 32);
                        f_tlo[p] = (uint32_t)T;
                    }
                    float acc[4][C::PPT];
                    const float4 *lq = lut_s + qd * LUT4;
                    if (nsub == 1) scan_quad_compute<C, 1, 0, 0>(lq, regs, acc);
                    else scan_quad_compute<C, 2, 0, 0>(lq, regs, acc);
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const uint32_t pq = f_pq[p];
                        if (pq == kInvalid) continue;   // wave-uniform
                        const uint64_t T = ((uint64_t)f_thi[p] << 32) | f_tlo[p];
                        const uint32_t Thi = f_thi[p];
                        const float Tf = (Thi == 0xFFFFFFFFu) ? __builtin_inff() : ordered_to_f32(Thi);
                        const uint32_t vb = f_vb[p];
#pragma unroll
                        for (int i = 0; i < C::PPT; ++i) {
                            if (i < (int)nsub && acc[p][i] <= Tf) {
                                const uint32_t j = c0 + tid + kResThreads * i;
                                if (j < size) {
                                    const uint64_t key = make_key(acc[p][i], vb + j);
                                    if (key <= T && row_allowed_if<PQ>(ix, a.allow, allow_stride, pq, allow_bits, lb + j)) {
                                        const uint32_t sl = atomicAdd(&scnt[wave][buf][qd * 4 + p], 1u);
                                        if (sl < kResStage) {
                                            skey[wave][buf][qd * 4 + p][sl] = key;
                                        } else {   // stage full: direct (slow) append
                                            const uint32_t pos = atomicAdd(&a.cand_cnt[pq], 1u);
                                            if (pos < a.cap) a.cand[(size_t)pq * a.cap + pos] = key;
                                        }
                                    }
                                }
                            }
                        }
                    }
                }
            }
            // C. write the previous chunk's survivors: lane = (pair j, entry e)
            if (flush) {
                constexpr int PER = 64 / NQS;                          // entries per pair per pass
#pragma unroll
                for (int e0 = 0; e0 < (int)kResStage; e0 += PER) {
                    const uint32_t j = lane / PER, e = e0 + lane % PER;
                    const uint32_t cj = (uint32_t)__shfl((int)fcnt, (int)j);
                    const uint32_t bj = (uint32_t)__shfl((int)fbase, (int)j);
                    const uint32_t qj = (uint32_t)__shfl((int)my_q, (int)j);
                    if (e < cj) {
                        const uint32_t pos = bj + e;
                        if (pos < a.cap) a.cand[(size_t)qj * a.cap + pos] = skey[wave][buf ^ 1u][j][e];
                    }
                }
                if (lane < (uint32_t)NQS) scnt[wave][buf ^ 1u][lane] = 0;
            }
        }
    }
}

// =====================================================================================
// K5: threshold from a strided sample (plan: sample_stride / sample_plan / sample_rank).
//
// K5a adc_sample_kernel: the scan's tiled LUT16 gather over every st-th point of each
// selected leaf.  Tiles = (leaf, chunk of (uint32_t)C::TP SAMPLED points, group of a.qpt query
// quads); the ordered approximate distance of sample i of (query, leaf) goes to
// samp[query][sbase(query, leaf) + i].  Points the allow-bitmap rejects are written as
// 0xFFFFFFFF (absent).
// K5b threshold_select_kernel: block per query; the j-th smallest sample by one LDS
// histogram over [min, max] of the sample + an exact rank inside the j-th's bin.
// =====================================================================================
struct SampleArgs {
    const uint32_t *pair_off, *stile_off, *pair_q, *pair_sbase;
    uint32_t *counters;
    const float *lutq;
    uint32_t *samp;
    uint32_t scap, st, qpt;
    const uint64_t *allow;
    uint64_t allow_bits;
};

template <typename C>
__global__ __launch_bounds__(kScanThreads, C::WGS) void adc_sample_kernel(TxhIndexDev ix, SampleArgs a) {
    // (PqCodec<C>: one bitmap per query; the launch packs the stride next to the capacity, see pq_allow_bits)
    constexpr bool PQ = C::PQ;
    const uint64_t allow_bits = pq_capacity<PQ>(a.allow_bits), allow_stride = pq_stride<PQ>(a.allow_bits);
    constexpr int LUT4 = C::LUT4;
    constexpr int STG = (LUT4 + kScanThreads - 1) / kScanThreads;
    extern __shared__ __attribute__((aligned(16))) float4 lut_s[];   // [2 * LUT4] + tile slot
    uint32_t &tile_sh = *reinterpret_cast<uint32_t *>(lut_s + 2 * LUT4);
    const uint32_t tid = threadIdx.x;
    const uint32_t total_tiles = a.counters[CNT_TOTAL_STILES];
    const uint32_t st = a.st;

    for (;;) {
        if (tid == 0) tile_sh = grab_tile(a.counters + CNT_XS, total_tiles);
        __syncthreads();
        const uint32_t tile = __builtin_amdgcn_readfirstlane(tile_sh);
        if (tile == kInvalid) break;

        const WorkItem item = decode_item(ix, a.stile_off, a.pair_off, tile);
        const uint32_t lb = item.lb, size = item.size, local = item.local, slot0 = item.slot0, slot_end = item.slot_end;
        const uint32_t ssize = (size + st - 1) / st;            // sampled points of the leaf
        const uint32_t nchunks = (ssize + (uint32_t)C::TP - 1) / (uint32_t)C::TP;
        const uint32_t chunk = local % nchunks, qg = local / nchunks;
        const uint32_t nquads = (slot_end - slot0) >> 2;
        const uint32_t q0 = qg * a.qpt;
        const uint32_t q1 = min(q0 + a.qpt, nquads);
        const uint32_t c0 = chunk * (uint32_t)C::TP;
        const uint32_t npts = min((uint32_t)C::TP, ssize - c0);
        const uint32_t nsub = (npts + kScanThreads - 1) / kScanThreads;

        uint32_t regs[C::PPT][C::REGS];
        bool ok[C::PPT];
#pragma unroll
        for (int i = 0; i < C::PPT; ++i) {
            const uint32_t j = c0 + tid + kScanThreads * i;
            const uint32_t row = lb + (j < ssize ? j * st : 0u);
            // (per-query bitmaps: the sample's own bit is tested where it is written, once per query of the quad)
            ok[i] = j < ssize && (PQ || row_allowed(ix, a.allow, allow_bits, row));
            uint32_t w[C::NWORDS];
            C::load_words(ix.codes + (size_t)row * C::NWORDS, w);
            C::unpack(w, regs[i]);
        }

        const float4 *gl = reinterpret_cast<const float4 *>(a.lutq) +
                           (size_t)((slot0 >> 2) + q0) * LUT4;
        {
            float4 r[STG];
#pragma unroll
            for (int t = 0; t < STG; ++t) {
                uint32_t e = tid + t * kScanThreads;
                if (e < (uint32_t)LUT4) r[t] = gl[e];
            }
#pragma unroll
            for (int t = 0; t < STG; ++t) {
                uint32_t e = tid + t * kScanThreads;
                if (e < (uint32_t)LUT4) lut_s[e] = r[t];
            }
        }
        __syncthreads();

        for (uint32_t qd = q0; qd < q1; ++qd) {
            const uint32_t buf = (qd - q0) & 1u;
            if (qd + 1 < q1) {   // LDS-DMA prefetch of the next quad's LUT into the idle buffer
                const float4 *g2 = gl + (size_t)(qd + 1 - q0) * LUT4;
#pragma unroll
                for (int t = 0; t < STG; ++t) {
                    const uint32_t e0 = (tid & ~63u) + t * kScanThreads;   // wave-uniform
                    if (e0 < (uint32_t)LUT4)
                        __builtin_amdgcn_global_load_lds(
                            (const __attribute__((address_space(1))) void *)(g2 + e0 + (tid & 63u)),
                            (__attribute__((address_space(3))) void *)(&lut_s[(buf ^ 1u) * LUT4 + e0]),
                            16, 0, 0);
                }
            }
            const uint32_t slot = slot0 + qd * 4;
            uint32_t f_pq[4], f_sb[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                f_pq[p] = __builtin_amdgcn_readfirstlane(a.pair_q[slot + p]);
                f_sb[p] = __builtin_amdgcn_readfirstlane(a.pair_sbase[slot + p]);
            }
            float acc[4][C::PPT];
            if (buf == 0) scan_quad_dispatch<C, 0>(lut_s, nsub, regs, acc);
            else scan_quad_dispatch<C, 1>(lut_s, nsub, regs, acc);
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (f_pq[p] == kInvalid) continue;   // wave-uniform
                uint32_t *dst = a.samp + (size_t)f_pq[p] * a.scap + f_sb[p];
#pragma unroll
                for (int i = 0; i < C::PPT; ++i) {
                    const uint32_t j = c0 + tid + kScanThreads * i;
                    if constexpr (PQ) {   // the sample is absent for this query only
                        if (i < (int)nsub && j < ssize)
                            dst[j] = row_allowed(ix, a.allow, allow_stride, f_pq[p], allow_bits, lb + j * st)
                                         ? f32_to_ordered(acc[p][i]) : 0xFFFFFFFFu;
                    } else {
                        if (i < (int)nsub && j < ssize) dst[j] = ok[i] ? f32_to_ordered(acc[p][i]) : 0xFFFFFFFFu;
                    }
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the LDS-DMA prefetch has landed
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kSelectThreads) void threshold_select_kernel(
    uint32_t P, uint32_t m, uint32_t st, int no_threshold, const uint32_t *__restrict__ sbase,
    const uint32_t *__restrict__ samp, uint32_t scap, const uint32_t *__restrict__ slot_of,
    uint64_t *__restrict__ thr, uint64_t *__restrict__ pair_thr, const uint32_t *__restrict__ vbase) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_vals[];   // [scap rounded to 4]
    const SelCfg cfg = sel_cfg(scap);
    uint32_t *s_hist = s_vals + ((scap + 3u) & ~3u);                    // [cfg.bins]
    uint32_t *s_list = s_hist + cfg.bins;                               // [cfg.list]
    uint64_t *s_red = reinterpret_cast<uint64_t *>(s_list + cfg.list);  // [48]
    const uint32_t q = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const uint32_t ns = min(sbase[(size_t)q * (P + 2) + P], scap);
    const uint32_t total = sbase[(size_t)q * (P + 2) + P + 1];
    const uint32_t J = (no_threshold || total <= m) ? 0u : sample_rank(m, st);
    // the scan reads the bound per (query, leaf) pair slot: no dependent pair_q -> thr load
    auto publish = [&](uint64_t T) {
        if (tid == 0) thr[q] = T;
        for (uint32_t r = tid; r < P; r += nt) {
            const uint32_t sl = slot_of[(size_t)q * P + r];
            if (sl != kInvalid) pair_thr[sl] = T;
        }
    };
    if (J == 0 || ns < J) {   // block-uniform
        publish(SCANN_KEY_MAX);
        return;
    }
    // sample -> LDS (16-byte loads; rows of samp are 16-byte aligned: scap % 4 == 0)
    const uint4 *src = reinterpret_cast<const uint4 *>(samp + (size_t)q * scap);
    const uint32_t n4 = (ns + 3u) >> 2;
    for (uint32_t i0 = 0; i0 < n4; i0 += 4 * nt) {
        uint4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t i = i0 + u * nt + tid;
            v[u] = i < n4 ? src[i] : make_uint4(~0u, ~0u, ~0u, ~0u);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t i = i0 + u * nt + tid;
            if (i < n4) {
                // entries past ns (row padding) count as absent
                if (4 * i + 1 >= ns) v[u].y = ~0u;
                if (4 * i + 2 >= ns) v[u].z = ~0u;
                if (4 * i + 3 >= ns) v[u].w = ~0u;
                reinterpret_cast<uint4 *>(s_vals)[i] = v[u];
            }
        }
    }
    __syncthreads();
    // absent samples (0xFFFFFFFF: rejected by the allow-bitmap, padding) sort last; the bound
    // is MAX if the J-th smallest is one of them
    const uint32_t v = block_select<uint32_t>(s_vals, 4 * n4, J, cfg, s_hist, s_list, s_red);
    if (v == 0xFFFFFFFFu) {
        publish(SCANN_KEY_MAX);
        return;
    }
    // Ties at the bound.  Coarse codes over clustered data give thousands of points the SAME approximate
    // distance; a bound on the distance alone lets the whole tie group through (measured: 2.5x the expected
    // survivors, candidate buffers overflowing).  The merge keys (distance, stream position) are unique, so the
    // bound is the J-th smallest sample KEY: among the samples that tie on the distance, the one with the
    // (J - #smaller)-th smallest stream position (sample i of token r is point i * st of that leaf).
    __syncthreads();
    uint32_t *s_cnt2 = reinterpret_cast<uint32_t *>(s_red);   // [0] smaller, [1] tied, [2] cursor, [3] result
    if (tid < 4) s_cnt2[tid] = tid == 3 ? 0xFFFFFFFFu : 0u;
    __syncthreads();
    uint32_t less = 0, tied = 0;
    for (uint32_t i = tid; i < 4 * n4; i += nt) {
        const uint32_t x = s_vals[i];
        less += x < v ? 1u : 0u;
        tied += x == v ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        less += (uint32_t)__shfl_xor((int)less, o);
        tied += (uint32_t)__shfl_xor((int)tied, o);
    }
    if ((tid & 63u) == 0) {
        atomicAdd(&s_cnt2[0], less);
        atomicAdd(&s_cnt2[1], tied);
    }
    __syncthreads();
    const uint32_t a_less = s_cnt2[0], b_tied = s_cnt2[1];
    uint32_t low = 0xFFFFFFFFu;   // (a single sample at the bound, or a tie group too large to rank: all of it passes)
    if (vbase && b_tied > 1 && b_tied <= cfg.list && J > a_less) {   // block-uniform
        uint32_t *s_vp = s_hist;                                   // [b_tied] stream positions of the tied samples
        const uint32_t *sb = sbase + (size_t)q * (P + 2), *vb = vbase + (size_t)q * (P + 1);
        for (uint32_t i = tid; i < 4 * n4; i += nt) {
            if (s_vals[i] == v) {
                uint32_t lo = 0, hi = P;   // token of sample slot i: largest r with sb[r] <= i
                while (hi - lo > 1) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (sb[mid] <= i) lo = mid; else hi = mid;
                }
                s_vp[atomicAdd(&s_cnt2[2], 1u)] = vb[lo] + (i - sb[lo]) * st;
            }
        }
        __syncthreads();
        const uint32_t need = J - a_less;                          // 1-based rank inside the tie group
        for (uint32_t i = tid; i < b_tied; i += nt) {
            const uint32_t x = s_vp[i];
            uint32_t r = 0;
            for (uint32_t j2 = 0; j2 < b_tied; ++j2) r += s_vp[j2] < x ? 1u : 0u;
            if (r + 1 == need) s_cnt2[3] = x;                      // (positions are unique)
        }
        __syncthreads();
        low = s_cnt2[3];
    }
    publish(((uint64_t)v << 32) | low);
}

// K5c: the same bound from the LOW TAIL of the sample only.  The bound is the J-th smallest of ~32 k sample keys with
// J a few hundred: the full histogram select above stages all of them in LDS (128 KB: one workgroup per compute unit,
// 1024 threads, ~10 workgroup barriers per pass) and makes five passes over them.  Here a 256-thread workgroup (eight
// per compute unit: every query of a 1024-query batch is resident at once) reads the sample from global memory (L2-hot:
// the sample pass has just written it) with 16-byte loads; every thread keeps the TWO smallest of its samples, and
// the J-th smallest of those 512 kept values is a pivot at or above the J-th smallest sample (any subset's J-th
// smallest is) and within a few percent of it; one more pass collects the (value, slot) keys at or under the pivot --
// a little over J of them -- and the J-th smallest of THOSE is the bound.  Sample slots grow with the stream position
// (sbase and vbase are prefixes in the same token order, samples of a leaf are st points apart), so ordering by
// (value, slot) IS ordering by the merge key (value, position): no separate ranking of the tie group.  If ties flood
// the list (more than kThrTailList samples at or under the pivot) the bound is (pivot, MAX): valid (pivot >= the J-th
// smallest), merely looser.
constexpr uint32_t kThrTailThreads = 256;
constexpr uint32_t kThrTailList = 2048;

__global__ __launch_bounds__(kThrTailThreads) void threshold_tail_kernel(
    uint32_t P, uint32_t m, uint32_t st, const uint32_t *__restrict__ sbase, const uint32_t *__restrict__ samp,
    uint32_t scap, const uint32_t *__restrict__ slot_of, uint64_t *__restrict__ thr, uint64_t *__restrict__ pair_thr,
    const uint32_t *__restrict__ vbase) {
    __shared__ uint32_t s_kept[2 * kThrTailThreads];
    __shared__ uint32_t s_hist[1024];
    __shared__ uint64_t s_slist[256];
    __shared__ uint64_t s_red[48];
    __shared__ uint64_t s_keys[kThrTailList];
    __shared__ uint32_t s_cnt[2];
    const uint32_t q = blockIdx.x, tid = threadIdx.x, nt = kThrTailThreads;
    const uint32_t ns = min(sbase[(size_t)q * (P + 2) + P], scap);
    const uint32_t total = sbase[(size_t)q * (P + 2) + P + 1];
    const uint32_t J = total <= m ? 0u : sample_rank(m, st);
    auto publish = [&](uint64_t T) {
        if (tid == 0) thr[q] = T;
        for (uint32_t r = tid; r < P; r += nt) {
            const uint32_t sl = slot_of[(size_t)q * P + r];
            if (sl != kInvalid) pair_thr[sl] = T;
        }
    };
    if (J == 0 || ns < J) {   // block-uniform
        publish(SCANN_KEY_MAX);
        return;
    }
    // rows of samp are 16-byte aligned (scap % 4 == 0); entries past ns count as absent
    const uint4 *src = reinterpret_cast<const uint4 *>(samp + (size_t)q * scap);
    const uint32_t n4 = (ns + 3u) >> 2;
    auto load4 = [&](uint32_t i) {
        uint4 v = make_uint4(~0u, ~0u, ~0u, ~0u);
        if (i < n4) {
            v = src[i];
            if (4 * i + 1 >= ns) v.y = ~0u;
            if (4 * i + 2 >= ns) v.z = ~0u;
            if (4 * i + 3 >= ns) v.w = ~0u;
        }
        return v;
    };
    uint32_t m0 = 0xFFFFFFFFu, m1 = 0xFFFFFFFFu;   // the two smallest of this thread's samples, m0 <= m1
    auto keep = [&](uint32_t x) {
        const uint32_t hi = x > m0 ? x : m0;
        m0 = x < m0 ? x : m0;
        m1 = hi < m1 ? hi : m1;
    };
    constexpr int LU = 8;   // 16-byte loads in flight per thread
    for (uint32_t i0 = 0; i0 < n4; i0 += LU * nt) {
        uint4 v[LU];
#pragma unroll
        for (int u = 0; u < LU; ++u) v[u] = load4(i0 + u * nt + tid);
#pragma unroll
        for (int u = 0; u < LU; ++u) {
            keep(v[u].x); keep(v[u].y); keep(v[u].z); keep(v[u].w);
        }
    }
    s_kept[2 * tid] = m0;
    s_kept[2 * tid + 1] = m1;
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    const SelCfg cfg = sel_cfg(kThrTailList);   // bins 1024, list 256
    uint32_t pivot = block_select<uint32_t>(s_kept, 2 * nt, J, cfg, s_hist, reinterpret_cast<uint32_t *>(s_slist), s_red);
    __syncthreads();
    // (absent samples -- rejected by the allow-bitmap -- sort last: with fewer than J kept values present the pivot is
    // "every present value")
    if (pivot == 0xFFFFFFFFu) pivot = 0xFFFFFFFEu;
    for (uint32_t i0 = 0; i0 < n4; i0 += LU * nt) {
        uint4 v[LU];
#pragma unroll
        for (int u = 0; u < LU; ++u) v[u] = load4(i0 + u * nt + tid);
#pragma unroll
        for (int u = 0; u < LU; ++u) {
            const uint32_t i = 4 * (i0 + u * nt + tid);
            const uint32_t x[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (x[c] <= pivot) {
                    const uint32_t pos = atomicAdd(&s_cnt[0], 1u);
                    if (pos < kThrTailList) s_keys[pos] = ((uint64_t)x[c] << 32) | (i + c);
                }
        }
    }
    __syncthreads();
    const uint32_t n_le = s_cnt[0];
    if (n_le < J) {   // fewer than J present samples in all: no bound
        publish(SCANN_KEY_MAX);
        return;
    }
    if (n_le > kThrTailList) {   // ties flood the list: the pivot is >= the J-th smallest value; all of that distance pass
        publish(((uint64_t)pivot << 32) | 0xFFFFFFFFu);
        return;
    }
    const uint64_t key = block_select<uint64_t>(s_keys, n_le, J, cfg, s_hist, s_slist, s_red);
    const uint32_t v = (uint32_t)(key >> 32), slot = (uint32_t)key;
    if (!vbase) {   // diagnostic mode: the bound on the distance alone, whole tie group
        publish(((uint64_t)v << 32) | 0xFFFFFFFFu);
        return;
    }
    // stream position of that sample: token r = the largest with sb[r] <= slot
    const uint32_t *sb = sbase + (size_t)q * (P + 2), *vb = vbase + (size_t)q * (P + 1);
    uint32_t lo = 0, hi = P;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sb[mid] <= slot) lo = mid; else hi = mid;
    }
    publish(((uint64_t)v << 32) | (vb[lo] + (slot - sb[lo]) * st));
}

// =====================================================================================
// K5d: the flat hasher's sample on the matrix cores, K5e: its bound from the low tail.
//
// adc_sample_kernel scores the sample with the f32 LDS gather and threshold_tail_kernel reads every one of those
// f32 values twice -- to find ONE number per query, the J-th smallest sample key, which only the lowest ~1 % of the
// samples can influence.  In front of an MFMA prefilter (flat hasher, 4-bit codes, plan: sample_mfma) the sample is
// scored the way the prefilter scores the scan: lut8_build_kernel(fold < 0) quantises the plain tables before any
// bound exists, adc_sample_mfma_kernel writes the integer sums u = sum q_s in [0, 255 S] as u16 (half the bytes),
// and threshold_tail16_kernel applies the reference's f32 arithmetic to the few hundred samples whose sums are low
// enough to matter.  The published bound is the J-th smallest f32 sample key, bit for bit what K5a + K5c publish:
//   * pivot P = the J-th smallest of the 512 values the threads keep (two smallest each): at least J samples have
//     u <= P, and a sample with sum u has f32 distance D <= (bias + sc (u + S (0.5 + 1e-9))) (1 + S 2^-23) (every
//     table entry v satisfies |v - (mn_s + sc q)| <= sc (0.5 + 1e-9); the factor covers the sequential f32 adds of
//     non-negative terms), so Dmax = that expression at u = P is an upper bound of the J-th smallest f32 distance;
//   * a sample with D <= Dmax has u <= qlim = floor((Dmax (1 + S 2^-23) - bias) / sc + S / 2 + 1) (the pass bound
//     of mfma_pass_bound): the samples with u <= qlim contain every sample at or under the J-th smallest f32
//     distance, and the J-th smallest exact key among them is the J-th smallest of the whole sample.
// More than kThrTailList samples under qlim (tie-heavy or badly scaled tables): the bound is (Dmax, MAX), valid and
// looser, as threshold_tail_kernel's flood case.  A table that cannot be quantised (scale = 0: NaN, negative or
// infinite entries, all entries equal) takes threshold_tail_kernel's two passes over f32 distances computed on the
// fly, sample to thread as there: the same bound in every case, for that query only.
// One leaf, one pair per query (P = 1, the plan guarantees it): sample i is point i * st, sample slot = sample index,
// slot_of[q] is valid wherever the index has points (an empty index has no samples: J = 0).  The publish loop over
// tokens and the token search at the end of threshold_tail16_kernel only mirror threshold_tail_kernel's skeleton.
// Under an allow-bitmap every column lane of a tile tests the same 16 sample rows (32 x redundant, L1-served reads): the
// filtered sample is still a few percent of the scan's work, so the mask is not shared across lanes.
// =====================================================================================
constexpr uint32_t kSmpTiles = 8;   // 32-sample tiles per item (wave) of adc_sample_mfma_kernel

struct SampleMfmaArgs {
    const uint32_t *pair_off, *pair_q, *pair_sbase;
    const int8_t *lut8;
    uint16_t *samp16;         // [nq][scap]
    uint32_t scap, st;
    const uint64_t *allow;
    uint64_t allow_bits;
};

// Operands as adc_mfma_kernel: lane (col, h) holds the table fragments of pair slot `col` of the item's 32-pair tile
// (subspaces of parity h), the A fragment of a (sample, subspace pair) is one row of the LDS identity table, register
// r of the result is sample row (r & 3) + 8 (r >> 2) + 4 h of the tile: four consecutive samples of one query per
// register group, one 8-byte store.  Items = (pair tile, kSmpTiles sample tiles), one per wave, grid-strided.
template <int S_>
__device__ __forceinline__ void adc_sample_mfma_body(TxhIndexDev ix, SampleMfmaArgs a, const uint64_t allow_stride) {
    typedef int v4i __attribute__((ext_vector_type(4)));
    typedef int v16i __attribute__((ext_vector_type(16)));
    constexpr int S = S_, KS = S / 2, NW = S / 8;
    __shared__ __attribute__((aligned(16))) uint32_t s_ident[64];                 // 16 one-hot rows of 16 bytes
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t col = lane & 31u, h = lane >> 5;
    if (tid < 64) {
        const uint32_t c = tid >> 2, wsel = tid & 3u;
        s_ident[tid] = (wsel == (c >> 2)) ? (1u << (8 * (c & 3u))) : 0u;
    }
    __syncthreads();
    const char *ident = reinterpret_cast<const char *>(s_ident);
    const uint32_t lb = uniform_load(ix.leaf_off), size = uniform_load(ix.leaf_off + 1) - lb;
    const uint32_t slot0 = uniform_load(a.pair_off), slot_end = uniform_load(a.pair_off + 1);
    const uint32_t st = a.st, ssize = min((size + st - 1) / st, a.scap);   // sampled points of the leaf
    const uint32_t ntile = (ssize + 31u) >> 5, nrange = (ntile + kSmpTiles - 1) / kSmpTiles;
    const uint32_t npt = (slot_end - slot0 + 31u) >> 5;
    const uint32_t nitems = npt * nrange, nwaves = gridDim.x * 4u;
    for (uint32_t item = blockIdx.x * 4u + wave; item < nitems; item += nwaves) {
        // (neighbouring waves: the same samples against different pair tiles -- their code rows come from L1 / L2)
        const uint32_t pt = item % npt, range = item / npt;
        const uint32_t slot = slot0 + pt * 32u + col;
        const bool pair_ok = slot < slot_end;
        const uint32_t pq = pair_ok ? a.pair_q[slot] : kInvalid;
        const uint32_t sb = pair_ok ? a.pair_sbase[slot] : 0u;
        v4i b[KS];
        {
            const int8_t *bsrc = a.lut8 + ((size_t)(pair_ok ? slot : slot0) * S + h) * 16;   // padding columns: any table
#pragma unroll
            for (int t = 0; t < KS; ++t) b[t] = *reinterpret_cast<const v4i *>(bsrc + (size_t)t * 32);
        }
        uint16_t *dst = a.samp16 + (size_t)(pq == kInvalid ? 0u : pq) * a.scap + sb;
        const uint32_t t0 = range * kSmpTiles, t1 = min(t0 + kSmpTiles, ntile);
        uint32_t wn[NW];
        {
            const uint32_t j = t0 * 32u + col;
            Codec<S, 4>::load_words(ix.codes + (size_t)(lb + (j < ssize ? j * st : 0u)) * NW, wn);
        }
        for (uint32_t t = t0; t < t1; ++t) {
            // nibbles of this lane's subspace parity h, pre-shifted to byte offsets code * 16
            uint32_t rg[NW];
#pragma unroll
            for (int wi = 0; wi < NW; ++wi) rg[wi] = h ? (wn[wi] & 0xF0F0F0F0u) : ((wn[wi] & 0x0F0F0F0Fu) << 4);
            if (t + 1 < t1) {   // the next tile's codes travel under this tile's MFMAs
                const uint32_t j = (t + 1) * 32u + col;
                Codec<S, 4>::load_words(ix.codes + (size_t)(lb + (j < ssize ? j * st : 0u)) * NW, wn);
            }
            v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int kt = 0; kt < KS; ++kt) {
                const uint32_t off = (rg[kt >> 2] >> (8 * (kt & 3))) & 0xFFu;   // code * 16 of subspace 2 kt + h
                const v4i av = *reinterpret_cast<const v4i *>(ident + off);
                acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, b[kt], acc, 0, 0, 0);
            }
            if (pq == kInvalid) continue;   // padding column: nothing to write
            const uint32_t base = t * 32u + 4u * h;
            uint32_t rej = 0;   // search_with_filter: bit r = the sample of register r is rejected (absent)
            if (a.allow) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint32_t i = base + (uint32_t)((r & 3) + 8 * (r >> 2));
                    const bool ok = i < ssize && row_allowed(ix, a.allow, allow_stride, pq, a.allow_bits, lb + i * st);
                    rej |= (ok ? 0u : 1u) << r;
                }
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint32_t i0 = base + 8u * (uint32_t)g;
                if (i0 >= ssize) continue;
                uint32_t u[4];
#pragma unroll
                for (int e = 0; e < 4; ++e)   // [0, 255 S], or the absent mark
                    u[e] = ((rej >> (4 * g + e)) & 1u) ? 0xFFFFu : (uint32_t)(acc[4 * g + e] + 128 * S);
                if (i0 + 3u < ssize) {   // (rows of samp16 and i0 are multiples of four entries: 8-byte aligned)
                    *reinterpret_cast<uint2 *>(dst + i0) = make_uint2(u[0] | (u[1] << 16), u[2] | (u[3] << 16));
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (i0 + e < ssize) dst[i0 + e] = (uint16_t)u[e];
                }
            }
        }
    }
}
// One bitmap for the batch, or none: the kernel every search without allow_bitmap_stride runs (its code is that of the
// body with the stride folded to 0).  _pq: one bitmap per query, allow_stride words apart.
template <int S_>
__global__ __launch_bounds__(256, (S_ <= 32 ? 3 : 2)) void adc_sample_mfma_kernel(TxhIndexDev ix, SampleMfmaArgs a) {
    adc_sample_mfma_body<S_>(ix, a, 0);
}
template <int S_>
__global__ __launch_bounds__(256, (S_ <= 32 ? 3 : 2)) void adc_sample_mfma_pq_kernel(TxhIndexDev ix, SampleMfmaArgs a, uint64_t allow_stride) {
    adc_sample_mfma_body<S_>(ix, a, allow_stride);
}

struct Tail16Args {
    uint32_t P, m, st, scap;
    const uint32_t *sbase, *slot_of, *tokens, *vbase;
    const uint16_t *samp16;
    const float *lutq;
    const Lut8Meta *meta;
    uint64_t *thr, *pair_thr;
};

template <int S_>
__global__ __launch_bounds__(kThrTailThreads) void threshold_tail16_kernel(TxhIndexDev ix, Tail16Args a) {
    constexpr int S = S_, NW = S / 8;
    __shared__ float s_tab[S * 16];   // the query's f32 table, de-interleaved: [s][16]
    __shared__ uint32_t s_kept[2 * kThrTailThreads];
    __shared__ uint32_t s_hist[1024];
    __shared__ uint64_t s_slist[256];
    __shared__ uint64_t s_red[48];
    __shared__ uint64_t s_keys[kThrTailList];
    __shared__ uint32_t s_cnt[2];
    const uint32_t q = blockIdx.x, tid = threadIdx.x, nt = kThrTailThreads, P = a.P;
    const uint32_t *sb = a.sbase + (size_t)q * (P + 2), *vb = a.vbase + (size_t)q * (P + 1);
    const uint32_t ns = min(sb[P], a.scap);
    const uint32_t total = sb[P + 1];
    const uint32_t J = total <= a.m ? 0u : sample_rank(a.m, a.st);
    auto publish = [&](uint64_t T) {
        if (tid == 0) a.thr[q] = T;
        for (uint32_t r = tid; r < P; r += nt) {
            const uint32_t sl = a.slot_of[(size_t)q * P + r];
            if (sl != kInvalid) a.pair_thr[sl] = T;
        }
    };
    if (J == 0 || ns < J) {   // block-uniform (an empty index, whose queries have no pair slot, ends here: J = 0)
        publish(SCANN_KEY_MAX);
        return;
    }
    const uint32_t tslot = a.slot_of[(size_t)q * P];   // P == 1: the query's one pair slot
    for (uint32_t e = tid; e < (uint32_t)S * 16u; e += nt)
        s_tab[e] = a.lutq[((size_t)(tslot >> 2) * S * 16 + e) * 4 + (tslot & 3u)];
    const Lut8Meta mt = a.meta[tslot];
    const bool exact = !(mt.scale > 0.0);   // table not quantised: f32 distances in both passes (block-uniform)
    const uint32_t row0 = ix.leaf_off[a.tokens[(size_t)q * P]];
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    // the reference's distance of sample slot i (hashes/lut.rs:74-82: subspace order)
    auto dist = [&](uint32_t i) {
        uint32_t w[NW];
        Codec<S, 4>::load_words(ix.codes + (size_t)(row0 + (i - sb[0]) * a.st) * NW, w);
        float acc = 0.0f;
#pragma unroll
        for (int s2 = 0; s2 < S; ++s2) {
            const float tv = s_tab[s2 * 16 + ((w[s2 >> 3] >> (4 * (s2 & 7))) & 15u)];
            acc = s2 == 0 ? tv : acc + tv;
        }
        return acc;
    };
    // rows of samp16 are 8-byte aligned (scap % 4 == 0): four samples per load; entries past ns and samples the
    // allow-bitmap rejected (0xFFFF) count as absent
    const uint2 *src = reinterpret_cast<const uint2 *>(a.samp16 + (size_t)q * a.scap);
    const uint32_t n4 = (ns + 3u) >> 2;
    auto value = [&](uint2 v, uint32_t i4, int c) {   // sample 4 i4 + c of the row, as this pass sees it
        const uint32_t x = ((c < 2 ? v.x : v.y) >> (16 * (c & 1))) & 0xFFFFu;
        return (4u * i4 + (uint32_t)c >= ns || x == 0xFFFFu) ? 0xFFFFFFFFu : x;
    };
    uint32_t m0 = 0xFFFFFFFFu, m1 = 0xFFFFFFFFu;   // the two smallest of this thread's samples, m0 <= m1
    auto keep = [&](uint32_t x) {
        const uint32_t hi = x > m0 ? x : m0;
        m0 = x < m0 ? x : m0;
        m1 = hi < m1 ? hi : m1;
    };
    constexpr int LU = 8;   // 8-byte loads in flight per thread
    if (!exact) {
        for (uint32_t i0 = 0; i0 < n4; i0 += LU * nt) {
            uint2 v[LU];
#pragma unroll
            for (int u = 0; u < LU; ++u) {
                const uint32_t i4 = i0 + u * nt + tid;
                v[u] = i4 < n4 ? src[i4] : make_uint2(~0u, ~0u);
            }
#pragma unroll
            for (int u = 0; u < LU; ++u)
#pragma unroll
                for (int c = 0; c < 4; ++c) keep(value(v[u], i0 + u * nt + tid, c));
        }
    } else {   // (thread tid takes the samples threshold_tail_kernel gives it: the same kept values, the same pivot)
        for (uint32_t i4 = tid; i4 < n4; i4 += nt) {
            const uint2 v = src[i4];
#pragma unroll 1
            for (int c = 0; c < 4; ++c)
                keep(value(v, i4, c) == 0xFFFFFFFFu ? 0xFFFFFFFFu : f32_to_ordered(dist(4u * i4 + (uint32_t)c)));
        }
    }
    s_kept[2 * tid] = m0;
    s_kept[2 * tid + 1] = m1;
    __syncthreads();
    const SelCfg cfg = sel_cfg(kThrTailList);   // bins 1024, list 256
    const uint32_t pivot = block_select<uint32_t>(s_kept, 2 * nt, J, cfg, s_hist, reinterpret_cast<uint32_t *>(s_slist), s_red);
    __syncthreads();
    // collect limit (in the unit of the pass's values) and the ordered distance of the flood bound; with fewer than J
    // kept values present the limit is "every present value"
    uint32_t lim, flood;
    if (exact) {
        lim = flood = pivot == 0xFFFFFFFFu ? 0xFFFFFFFEu : pivot;
    } else if (pivot == 0xFFFFFFFFu) {
        lim = 0xFFFEu;
        flood = 0xFFFFFFFEu;
    } else {
        const double Sd = (double)S, eps = Sd * 1.1920928955078125e-07;
        const double Dmax = (mt.bias_sum + mt.scale * ((double)pivot + Sd * (0.5 + 1e-9))) * (1.0 + eps);
        const double ql = floor((Dmax * (1.0 + eps) - mt.bias_sum) / mt.scale + 0.5 * Sd + 1.0);
        lim = ql >= 65534.0 ? 0xFFFEu : (uint32_t)ql;
        float Df = (float)Dmax;   // rounded up: the bound must not fall under Dmax
        if ((double)Df < Dmax) Df = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, Df) + 1u);
        flood = f32_to_ordered(Df);
    }
    if (!exact) {
        for (uint32_t i0 = 0; i0 < n4; i0 += LU * nt) {
            uint2 v[LU];
#pragma unroll
            for (int u = 0; u < LU; ++u) {
                const uint32_t i4 = i0 + u * nt + tid;
                v[u] = i4 < n4 ? src[i4] : make_uint2(~0u, ~0u);
            }
#pragma unroll
            for (int u = 0; u < LU; ++u)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const uint32_t i4 = i0 + u * nt + tid;
                    if (value(v[u], i4, c) <= lim) {
                        const uint32_t pos = atomicAdd(&s_cnt[0], 1u);
                        if (pos < kThrTailList) s_keys[pos] = 4u * i4 + (uint32_t)c;
                    }
                }
        }
    } else {
        for (uint32_t i4 = tid; i4 < n4; i4 += nt) {
            const uint2 v = src[i4];
#pragma unroll 1
            for (int c = 0; c < 4; ++c) {
                if (value(v, i4, c) == 0xFFFFFFFFu) continue;
                const uint32_t i = 4u * i4 + (uint32_t)c, x = f32_to_ordered(dist(i));
                if (x <= lim) {
                    const uint32_t pos = atomicAdd(&s_cnt[0], 1u);
                    if (pos < kThrTailList) s_keys[pos] = ((uint64_t)x << 32) | i;
                }
            }
        }
    }
    __syncthreads();
    const uint32_t n_le = s_cnt[0];
    if (n_le < J) {   // fewer than J present samples in all: no bound
        publish(SCANN_KEY_MAX);
        return;
    }
    if (n_le > kThrTailList) {   // the list floods: (Dmax, MAX) is at or above the J-th smallest key
        publish(((uint64_t)flood << 32) | 0xFFFFFFFFu);
        return;
    }
    if (!exact) {   // the collected slots -> their exact keys (each entry by the thread that rewrites it)
        for (uint32_t e = tid; e < n_le; e += nt) {
            const uint32_t i = (uint32_t)s_keys[e];
            s_keys[e] = make_key(dist(i), i);
        }
        __syncthreads();
    }
    const uint64_t key = block_select<uint64_t>(s_keys, n_le, J, cfg, s_hist, s_slist, s_red);
    const uint32_t v = (uint32_t)(key >> 32), slot = (uint32_t)key;
    // stream position of that sample: token r = the largest with sb[r] <= slot
    uint32_t lo = 0, hi = P;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sb[mid] <= slot) lo = mid; else hi = mid;
    }
    publish(((uint64_t)v << 32) | (vb[lo] + (slot - sb[lo]) * a.st));
}

// =====================================================================================
// K6c: exact leaf scan -- Scann::search_partitioned (scann.rs:213-252).  Every row of the P
// selected leaves is scored with the configured measure's single-pair kernel
// (DistanceMeasure::distance, distance_measures/mod.rs:70-81 -> simd/x86.rs:72-96 / :139-165: 8
// FMA lane chains, fixed hsum tree, scalar tail); candidates in token order then leaf order,
// stable sort, first k.  Tile = (leaf, 256-row chunk, group of quads): a thread owns one row and
// walks the tile's queries eight at a time from LDS, the lane chains as packed-f32 pairs
// (v_pk_fma_f32).  Every (query, stream position) is written exactly once into the query's
// dense key list [vbase[P]], from which select_rerank_kernel takes the k smallest keys.
// =====================================================================================
constexpr uint32_t kExactRows = 256;   // rows per tile chunk (one per thread)
constexpr uint32_t kExactQuadsMax = 16; // quads per tile: all of them staged in LDS once per tile
constexpr int kExactQT = 8;            // queries per pass over the row
// quads per tile for this dimensionality: the tile's queries must fit 48 KB of LDS
static inline uint32_t exact_quads_per_tile(uint32_t dim) {
    const uint32_t dimp = (dim + 3u) & ~3u;
    uint32_t q = (48u * 1024u) / (dimp * 4u) / 8u * 2u;   // whole passes of 8 queries, in quads
    return q < 2u ? 2u : (q > kExactQuadsMax ? kExactQuadsMax : q);
}

struct ExactScanArgs {
    const uint32_t *pair_off, *tile_off, *pair_q, *pair_vbase;
    uint32_t *counters;
    const float *queries;
    uint32_t q_stride;
    uint64_t *cand;
    uint32_t cap;
    uint32_t qpt;   // quads per tile (exact_quads_per_tile)
};

__global__ void stream_counts_kernel(uint32_t nq, uint32_t P, const uint32_t *__restrict__ vbase,
                                     uint32_t *__restrict__ cand_cnt) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nq) cand_cnt[q] = vbase[(size_t)q * (P + 1) + P];
}

template <int MEASURE>
__global__ __launch_bounds__(256) void leaf_exact_scan_kernel(TxhIndexDev ix, ExactScanArgs a) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) float qs_all[];   // [4 * a.qpt][dimp]: the tile's queries
    __shared__ uint32_t s_pq_all[kExactQuadsMax * 4], s_vb_all[kExactQuadsMax * 4], tile_sh;
    const uint32_t tid = threadIdx.x;
    const uint32_t dim = ix.dim, dimp = (dim + 3u) & ~3u, chunks = dim >> 3;
    const uint32_t total_tiles = a.counters[CNT_TOTAL_TILES];
    const bool vec = ((ix.stride & 3u) == 0) && ((reinterpret_cast<uintptr_t>(ix.rows) & 15u) == 0);
    const bool qvec = ((a.q_stride & 3u) == 0) && ((reinterpret_cast<uintptr_t>(a.queries) & 15u) == 0);
    for (;;) {
        __syncthreads();   // the previous tile's LDS reads are done
        if (tid == 0) tile_sh = grab_tile(a.counters + CNT_XQ, total_tiles);
        __syncthreads();
        const uint32_t tile = __builtin_amdgcn_readfirstlane(tile_sh);
        if (tile == kInvalid) break;
        const WorkItem item = decode_item(ix, a.tile_off, a.pair_off, tile);
        const uint32_t lb = item.lb, size = item.size, local = item.local, slot0 = item.slot0, slot_end = item.slot_end;
        const uint32_t nchunks = (size + kExactRows - 1) / kExactRows;
        const uint32_t chunk = local % nchunks, qg = local / nchunks;
        const uint32_t s_begin = slot0 + qg * a.qpt * 4u;
        const uint32_t s_stop = min(s_begin + a.qpt * 4u, slot_end);
        const uint32_t j = chunk * kExactRows + tid;
        const bool valid = j < size;
        const uint32_t csr = lb + (valid ? j : 0u);
        const float *row = ix.rows + (size_t)(ix.rows_csr ? csr : ix.leaf_ids[csr]) * ix.stride;

        // stage every query of the tile once (the passes below then run without a barrier)
        const uint32_t nslots = s_stop - s_begin, nslots8 = (nslots + 7u) & ~7u;
        if (tid < nslots8) {
            const uint32_t sl = s_begin + tid;
            s_pq_all[tid] = sl < s_stop ? a.pair_q[sl] : kInvalid;
            s_vb_all[tid] = sl < s_stop ? a.pair_vbase[sl] : 0u;
        }
        __syncthreads();   // s_pq_all visible
        if (qvec) {
            // 16-byte copies, four independent loads in flight per thread (an element-at-a-time loop
            // serialised two dependent global loads per element: ~50 us per tile)
            const uint32_t dim4 = dimp >> 2, total4 = nslots8 * dim4;
            for (uint32_t i0 = 0; i0 < total4; i0 += 1024u) {
                float4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t i = i0 + 256u * u + tid;
                    v[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (i < total4) {
                        const uint32_t qi = i / dim4, j4 = (i - qi * dim4) * 4u;
                        const uint32_t pq = s_pq_all[qi];
                        if (pq != kInvalid) {
                            v[u] = *reinterpret_cast<const float4 *>(a.queries + (size_t)pq * a.q_stride + j4);
                            if (j4 + 1 >= dim) v[u].y = 0.0f;   // padding of the last piece
                            if (j4 + 2 >= dim) v[u].z = 0.0f;
                            if (j4 + 3 >= dim) v[u].w = 0.0f;
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t i = i0 + 256u * u + tid;
                    if (i < total4) reinterpret_cast<float4 *>(qs_all)[i] = v[u];
                }
            }
        } else {
            for (uint32_t i = tid; i < nslots8 * dimp; i += 256) {
                const uint32_t qi = i / dimp, jj = i - qi * dimp;
                const uint32_t pq = s_pq_all[qi];
                qs_all[i] = (pq != kInvalid && jj < dim) ? a.queries[(size_t)pq * a.q_stride + jj] : 0.0f;
            }
        }
        __syncthreads();

        for (uint32_t sg = 0; sg < nslots; sg += kExactQT) {
            const float *qs = qs_all + sg * dimp;
            const uint32_t *s_pq = s_pq_all + sg, *s_vb = s_vb_all + sg;
            f32x2 accv[kExactQT][4];
            // Cosine (one_to_one.rs:559-604) also sums a.a and b.b lane by lane; the query's chains are
            // recomputed per row like the reference does (same operations, same value every time)
            f32x2 aav[MEASURE == SCANN_HIP_COSINE ? kExactQT : 1][4];
            f32x2 bbv[4] = {f32x2{0.0f, 0.0f}, f32x2{0.0f, 0.0f}, f32x2{0.0f, 0.0f}, f32x2{0.0f, 0.0f}};
#pragma unroll
            for (int qi = 0; qi < kExactQT; ++qi)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    accv[qi][u] = f32x2{0.0f, 0.0f};
                    if (MEASURE == SCANN_HIP_COSINE) aav[MEASURE == SCANN_HIP_COSINE ? qi : 0][u] = f32x2{0.0f, 0.0f};
                }
            // the row streams through registers four 8-dim chunks at a time, the next group in
            // flight while this one computes (a chunk-at-a-time loop exposed one global-load latency
            // per 8 dims)
            constexpr int G = 4;
            float4 xa[G], xb[G], na[G], nb[G];
            auto load_group = [&](uint32_t c0, float4 *pa, float4 *pb) {
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const uint32_t c = c0 + g;
                    if (c < chunks) {
                        if (vec) {
                            pa[g] = *reinterpret_cast<const float4 *>(row + 8 * c);
                            pb[g] = *reinterpret_cast<const float4 *>(row + 8 * c + 4);
                        } else {
                            pa[g] = make_float4(row[8 * c], row[8 * c + 1], row[8 * c + 2], row[8 * c + 3]);
                            pb[g] = make_float4(row[8 * c + 4], row[8 * c + 5], row[8 * c + 6], row[8 * c + 7]);
                        }
                    }
                }
            };
            load_group(0, xa, xb);
            for (uint32_t c0 = 0; c0 < chunks; c0 += G) {
                if (c0 + G < chunks) load_group(c0 + G, na, nb);
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const uint32_t c = c0 + g;
                    if (c >= chunks) break;
                    const f32x2 x[4] = {f32x2{xa[g].x, xa[g].y}, f32x2{xa[g].z, xa[g].w}, f32x2{xb[g].x, xb[g].y},
                                        f32x2{xb[g].z, xb[g].w}};
#pragma unroll
                    for (int qi = 0; qi < kExactQT; ++qi) {
                        const float4 qa = *reinterpret_cast<const float4 *>(qs + qi * dimp + 8 * c);
                        const float4 qb = *reinterpret_cast<const float4 *>(qs + qi * dimp + 8 * c + 4);
                        const f32x2 qv[4] = {f32x2{qa.x, qa.y}, f32x2{qa.z, qa.w}, f32x2{qb.x, qb.y},
                                             f32x2{qb.z, qb.w}};
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            if (MEASURE == SCANN_HIP_DOT_PRODUCT) {
                                accv[qi][u] = __builtin_elementwise_fma(qv[u], x[u], accv[qi][u]);
                            } else if (MEASURE == SCANN_HIP_L1) {       // l1_distance_avx2: add |a - b|, no FMA
                                accv[qi][u] = accv[qi][u] + __builtin_elementwise_abs(qv[u] - x[u]);
                            } else if (MEASURE == SCANN_HIP_COSINE) {   // add(mul): two roundings
                                accv[qi][u] = accv[qi][u] + qv[u] * x[u];
                                if (qi == 0) bbv[u] = bbv[u] + x[u] * x[u];
                                aav[MEASURE == SCANN_HIP_COSINE ? qi : 0][u] = aav[MEASURE == SCANN_HIP_COSINE ? qi : 0][u] + qv[u] * qv[u];
                            } else {
                                const f32x2 d = qv[u] - x[u];
                                accv[qi][u] = __builtin_elementwise_fma(d, d, accv[qi][u]);
                            }
                        }
                    }
                }
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    xa[g] = na[g];
                    xb[g] = nb[g];
                }
            }
#pragma unroll
            for (int qi = 0; qi < kExactQT; ++qi) {
                const uint32_t pq = s_pq[qi];
                if (pq == kInvalid) continue;   // block-uniform
                // hsum tree (x86.rs:31-44): lanes (0+4, 1+5), (2+6, 3+7) -> (s0+s1) + (s2+s3)
                const f32x2 s01 = accv[qi][0] + accv[qi][2], s23 = accv[qi][1] + accv[qi][3];
                float r = (s01.x + s01.y) + (s23.x + s23.y);
                float saa = 0.0f, sbb = 0.0f;
                if (MEASURE == SCANN_HIP_COSINE) {   // wide 0.7 reduce_add (non-AVX build): ((v0+v1)+v2)+v3 per half
                    const f32x2 *av = aav[MEASURE == SCANN_HIP_COSINE ? qi : 0];
                    r = (((accv[qi][0].x + accv[qi][0].y) + accv[qi][1].x) + accv[qi][1].y) +
                        (((accv[qi][2].x + accv[qi][2].y) + accv[qi][3].x) + accv[qi][3].y);
                    saa = (((av[0].x + av[0].y) + av[1].x) + av[1].y) + (((av[2].x + av[2].y) + av[3].x) + av[3].y);
                    sbb = (((bbv[0].x + bbv[0].y) + bbv[1].x) + bbv[1].y) + (((bbv[2].x + bbv[2].y) + bbv[3].x) + bbv[3].y);
                }
                for (uint32_t jj = chunks * 8; jj < dim; ++jj) {   // scalar tail, not fused
                    const float qv = qs[qi * dimp + jj];
                    if (MEASURE == SCANN_HIP_DOT_PRODUCT) {
                        r = r + qv * row[jj];
                    } else if (MEASURE == SCANN_HIP_L1) {
                        r = r + fabsf(qv - row[jj]);
                    } else if (MEASURE == SCANN_HIP_COSINE) {
                        r = r + qv * row[jj];
                        saa = saa + qv * qv;
                        sbb = sbb + row[jj] * row[jj];
                    } else {
                        const float d = qv - row[jj];
                        r = r + d * d;
                    }
                }
                float dist = r;
                if (MEASURE == SCANN_HIP_DOT_PRODUCT) dist = -r;
                if (MEASURE == SCANN_HIP_L2) dist = sqrtf(r);
                if (MEASURE == SCANN_HIP_COSINE) {   // one_to_one.rs:596-612
                    const float na = sqrtf(saa), nb = sqrtf(sbb);
                    dist = 1.0f - ((na == 0.0f || nb == 0.0f) ? 0.0f : r / (na * nb));
                }
                if (valid) {
                    const uint32_t vpos = s_vb[qi] + j;
                    if (vpos < a.cap) a.cand[(size_t)pq * a.cap + vpos] = make_key(dist, vpos);
                }
            }
        }
    }
}

// =====================================================================================
// K7: select + re-rank.  mod.rs:283-293 and :342-364 for one query per block:
//   candidates -> exact m best keys (sorted) -> decode -> exact SquaredL2 with the
//   reference's AVX2 arithmetic (simd/x86.rs:139-165: 8 FMA lane chains, fixed hsum
//   tree, scalar tail) -> stable sort by exact -> first k.
// =====================================================================================

struct SelectArgs {
    uint32_t P, m, k, cap;
    uint32_t lds_keys;   // capacity of the LDS key array (<= kSortCap)
    uint32_t direct;     // unsorted selection straight from the global list (no LDS staging); sel_n sizes its scratch
    uint32_t sel_n;
    int exact_reorder, local_only;
    int unsorted;   // candidates may leave in any order (final stage orders by 96-bit keys)
    const float *queries;
    uint32_t q_stride;
    const uint32_t *tokens, *vbase;
    const uint64_t *thr;
    uint32_t *cand_cnt;
    uint64_t *cand;
    uint32_t *counters;
    uint64_t *cand_key;
    uint32_t *cand_idx;
    float *cand_dist, *cand_exact;
    uint32_t *cand_row;
    uint32_t *cand_count;
    uint32_t *out_idx;
    float *out_dist;
    uint32_t *out_count;
};

// Stable compaction of list[0..cnt) keeping keys <= T into dst (dst == list: in place), by one block.
__device__ static uint32_t block_compact_le(const uint64_t *list, uint64_t *dst, uint32_t cnt, uint64_t T,
                                            uint32_t *s_wave, uint32_t *s_base) {
    const uint32_t tid = threadIdx.x, nt = blockDim.x, wave = tid >> 6, nw = nt >> 6;
    if (tid == 0) *s_base = 0;
    __syncthreads();
    for (uint32_t b = 0; b < cnt; b += nt) {
        const uint32_t i = b + tid;
        uint64_t key = 0;
        bool keep = false;
        if (i < cnt) {
            key = list[i];
            keep = key <= T;
        }
        uint32_t wtot;
        const uint32_t wpre = wave_prefix_count(keep, &wtot);
        if ((tid & 63u) == 0) s_wave[wave] = wtot;
        __syncthreads();
        uint32_t off = *s_base;
        for (uint32_t w = 0; w < wave; ++w) off += s_wave[w];
        if (keep) dst[off + wpre] = key;   // off + wpre <= i: never overtakes unread data
        __syncthreads();
        if (tid == 0) {
            uint32_t t = 0;
            for (uint32_t w = 0; w < nw; ++w) t += s_wave[w];
            *s_base += t;
        }
        __syncthreads();
    }
    return *s_base;
}

__device__ static void select_fail(const SelectArgs &a, uint32_t q, uint32_t status) {
    if (threadIdx.x == 0) {
        atomicMax(&a.counters[CNT_STATUS], status);
        a.cand_count[q] = 0;
        if (!a.local_only) a.out_count[q] = 0;
    }
}

__global__ __launch_bounds__(kSelectThreads) void select_rerank_kernel(TxhIndexDev ix,
                                                                       SelectArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint64_t skeys[];      // [a.lds_keys]
    const uint32_t sort_cap = a.lds_keys;
    const SelCfg cfg = sel_cfg(a.direct ? a.sel_n : sort_cap);
    uint32_t *s_dvb = reinterpret_cast<uint32_t *>(skeys + sort_cap) + (kSelectThreads / 64 + 4) + cfg.bins +
                      2 * cfg.list + 96;                                  // [kDecodeStage]
    uint32_t *s_drow = s_dvb + kDecodeStage;                              // [kDecodeStage]
    uint32_t *s_wave = reinterpret_cast<uint32_t *>(skeys + sort_cap);    // [kSelectThreads/64]
    uint32_t *s_basep = s_wave + kSelectThreads / 64;                     // [4]
    const uint32_t q = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const uint32_t m = a.m, k = a.k;

    uint32_t cnt = a.cand_cnt[q];
    if (cnt > a.cap) {  // candidate buffer overflow: report, never return a wrong row
        select_fail(a, q, (uint32_t)SCANN_HIP_RESOURCE_EXHAUSTED);
        return;
    }
    // A statistical threshold (sample rank j < m) must be verified: with >= m survivors
    // the exact top-m is among them; with fewer the threshold was too tight.
    if (a.thr[q] != SCANN_KEY_MAX && cnt < m) {
        select_fail(a, q, (uint32_t)SCANN_HIP_ABORTED);
        return;
    }
    uint64_t *list = a.cand + (size_t)q * a.cap;

    uint32_t *hist = reinterpret_cast<uint32_t *>(s_basep + 4);
    uint64_t *slist = reinterpret_cast<uint64_t *>(hist + cfg.bins);
    uint64_t *sred = slist + cfg.list;
    bool in_lds = false;   // skeys[0..cnt) already holds the candidates
    if (cnt > sort_cap && !a.direct) {
        // More candidates than LDS holds (no-threshold retry, dense lists of the exact leaf scan):
        // rank-select the m-th smallest key straight from the global list, then keep the keys <= it
        // (keys are unique, so exactly m remain; m <= kMaxPreReorderK <= sort_cap).
        const uint64_t T = block_select<uint64_t>(list, cnt, m, cfg, hist, slist, sred);
        __syncthreads();
        cnt = block_compact_le(list, skeys, cnt, T, s_wave, s_basep);
        __syncthreads();
        in_lds = true;
    }
    if (cnt > sort_cap && !a.direct) {   // cannot happen: m <= sort_cap
        select_fail(a, q, (uint32_t)SCANN_HIP_RESOURCE_EXHAUSTED);
        return;
    }

    const uint32_t nsel = min(m, cnt);   // truncate(pre_reorder_k)  mod.rs:290
    // decode tables of this query (key base and first CSR row of each selected leaf) in LDS:
    // the per-candidate chain vbase -> token -> leaf_off -> leaf_ids is otherwise four
    // dependent global loads
    const uint32_t *vb = a.vbase + (size_t)q * (a.P + 1);
    const bool staged = a.P <= kDecodeStage;
    if (staged) {
        for (uint32_t r = tid; r < a.P; r += nt) {
            s_dvb[r] = vb[r];
            s_drow[r] = ix.leaf_off[a.tokens[(size_t)q * a.P + r]];
        }
        __syncthreads();
    }
    auto decode = [&](uint64_t key, uint32_t i) {
        // merge key -> (rank, position in leaf) -> CSR row -> datapoint index
        const uint32_t vpos = (uint32_t)key;
        uint32_t lo = 0, hi = a.P;
        uint32_t csr;
        if (staged) {
            while (hi - lo > 1) {
                uint32_t mid = (lo + hi) >> 1;
                if (s_dvb[mid] <= vpos) lo = mid; else hi = mid;
            }
            csr = s_drow[lo] + (vpos - s_dvb[lo]);
        } else {
            while (hi - lo > 1) {
                uint32_t mid = (lo + hi) >> 1;
                if (vb[mid] <= vpos) lo = mid; else hi = mid;
            }
            csr = ix.leaf_off[a.tokens[(size_t)q * a.P + lo]] + (vpos - vb[lo]);
        }
        {
        const uint32_t idx = ix.leaf_ids ? ix.leaf_ids[csr] : csr;
        a.cand_row[(size_t)q * m + i] = ix.rows_csr ? csr : idx;
        a.cand_key[(size_t)q * m + i] = key;
        a.cand_idx[(size_t)q * m + i] = idx;
        a.cand_dist[(size_t)q * m + i] = ordered_to_f32((uint32_t)(key >> 32));
        }
    };

    if (a.unsorted) {
        // Selection without a sort: the m-th smallest key by histogram select, keep keys <= it.
        // The final stage orders by (exact, merge key), which equals (exact, approx rank).
        // direct: the keys stay in the (L2-hot) global list -- staging ~10 k keys takes 80-128 KB of LDS, ONE
        // workgroup per compute unit; without it every query's workgroup is resident at once
        const uint64_t *src = a.direct ? list : skeys;
        if (!in_lds && !a.direct)
            for (uint32_t i = tid; i < cnt; i += nt) skeys[i] = list[i];
        __syncthreads();
        const uint64_t T = cnt > m ? block_select<uint64_t>(src, cnt, m, cfg, hist, slist, sred) : SCANN_KEY_MAX;
        __syncthreads();
        uint32_t *s_slot = reinterpret_cast<uint32_t *>(sred);   // output cursor
        if (tid == 0) *s_slot = 0;
        __syncthreads();
        for (uint32_t b = 0; b < cnt; b += nt) {   // wave-aggregated slot allocation, any order
            const uint32_t i = b + tid;
            uint64_t key = 0;
            bool keep = false;
            if (i < cnt) {
                key = src[i];
                keep = key <= T;
            }
            uint32_t wtot;
            const uint32_t wpre = wave_prefix_count(keep, &wtot);
            uint32_t base = 0;
            if ((tid & 63u) == 0 && wtot) base = atomicAdd(s_slot, wtot);
            base = (uint32_t)__shfl((int)base, 0);
            if (keep) decode(key, base + wpre);
        }
        if (tid == 0) a.cand_count[q] = nsel;
        return;
    }

    if (!in_lds)
        for (uint32_t i = tid; i < cnt; i += nt) skeys[i] = list[i];
    __syncthreads();
    if (cnt > 2 * m && cnt > 256) {   // sort only the m best: select the m-th key, compact in place
        const uint64_t T = block_select<uint64_t>(skeys, cnt, m, cfg, hist, slist, sred);
        __syncthreads();
        cnt = block_compact_le(skeys, skeys, cnt, T, s_wave, s_basep);
        __syncthreads();
    }
    uint32_t n2 = 1;
    while (n2 < cnt) n2 <<= 1;
    for (uint32_t i = cnt + tid; i < n2; i += nt) skeys[i] = SCANN_KEY_MAX;
    __syncthreads();
    bitonic_sort_lds(skeys, n2);

    for (uint32_t i = tid; i < nsel; i += nt) decode(skeys[i], i);
    if (tid == 0) a.cand_count[q] = nsel;

    if (!a.exact_reorder) {  // AsymmetricHasher::search: k best by approximate distance
        if (!a.local_only) {
            __syncthreads();
            const uint32_t nout = min(k, nsel);
            for (uint32_t i = tid; i < k; i += nt) {
                a.out_idx[(size_t)q * k + i] = (i < nout) ? a.cand_idx[(size_t)q * m + i] : kInvalid;
                a.out_dist[(size_t)q * k + i] =
                    (i < nout) ? ordered_to_f32((uint32_t)(skeys[i] >> 32)) : __builtin_inff();
            }
            if (tid == 0) a.out_count[q] = nout;
        }
        return;
    }

    // exact re-rank and the final sort run in rerank_kernel / final_sort_kernel
}

// =====================================================================================
// K7r: the unsorted select of a long list (SelectArgs::direct) with the list in registers.  select_rerank_kernel
// sweeps the query's list four times from global memory (min / max, histogram, the rank's bin, keep and decode),
// 16-25 dependent trips per thread each; here every thread loads its VPT keys once, all loads in flight, and
// block_select's scheme runs on that copy as in wide_final_kernel: histogram over [min, max], the bin of rank m,
// its members ranked exactly by counting; a crowded bin becomes the new range and the round repeats on the
// registers.  The keys are unique, so T (the m-th smallest) is the value block_select returns and exactly m keys
// are <= T.  Same checks, same status codes, same outputs as the unsorted branch above, except cand_dist: only a
// caller that asks for stage outputs reads it, and that forces the sorted path (need_sorted_cands).
// Launched when cap <= VPT * kSelRegThreads (launch_select).
// =====================================================================================
// 512 threads: 16 / 26 / 36 keys each, 86 / 103 / 124 VGPRs, two workgroups per CU (1024 threads x 8 / 13 / 18 keys
// measured slower: 80 VGPRs at 13 keys leave room for one 16-wave workgroup per CU)
constexpr uint32_t kSelRegThreads = 512;
constexpr uint32_t kSelRegCaps[3] = {8192, 13312, 18432};   // list capacities of the three instantiations

template <int VPT>
__global__ __launch_bounds__(kSelRegThreads) void select_regs_kernel(TxhIndexDev ix, SelectArgs a) {
    __shared__ uint32_t s_hist[kSelBinsMax];
    __shared__ uint64_t s_slist[kSelListMax], s_mm[2 * (kSelRegThreads / 64)], s_T;
    __shared__ uint32_t s_dvb[kDecodeStage], s_drow[kDecodeStage], s_w[50], s_cn, s_pre[VPT * (kSelRegThreads / 64)];
    constexpr uint32_t nt = kSelRegThreads;
    const uint32_t q = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t m = a.m;

    const uint32_t cnt = a.cand_cnt[q];
    if (cnt > a.cap) {  // candidate buffer overflow: report, never return a wrong row
        select_fail(a, q, (uint32_t)SCANN_HIP_RESOURCE_EXHAUSTED);
        return;
    }
    if (a.thr[q] != SCANN_KEY_MAX && cnt < m) {   // a statistical bound that was too tight (see select_rerank_kernel)
        select_fail(a, q, (uint32_t)SCANN_HIP_ABORTED);
        return;
    }
    // key e * nt + tid of the list lives in this lane's registers (cnt <= cap <= VPT * nt); padding sorts last
    const uint64_t *list = a.cand + (size_t)q * a.cap;
    uint64_t kk[VPT];
#pragma unroll
    for (int e = 0; e < VPT; ++e) {
        const uint32_t i = (uint32_t)e * nt + tid;
        kk[e] = i < cnt ? list[i] : SCANN_KEY_MAX;
    }
    const uint32_t *vb = a.vbase + (size_t)q * (a.P + 1);
    const bool staged = a.P <= kDecodeStage;
    if (staged) {
        for (uint32_t r = tid; r < a.P; r += nt) {
            s_dvb[r] = vb[r];
            s_drow[r] = ix.leaf_off[a.tokens[(size_t)q * a.P + r]];
        }
    }
    auto clear = [&]() {
        for (uint32_t i = tid; i < kSelBinsMax; i += nt) s_hist[i] = 0;
        if (tid == 0) s_cn = 0;
    };
    clear();

    uint64_t T = SCANN_KEY_MAX;   // cnt <= m: everything stays
    if (cnt > m) {                // block-uniform
        uint64_t vmin = SCANN_KEY_MAX, vmax = 0;
#pragma unroll
        for (int e = 0; e < VPT; ++e)
            if (kk[e] != SCANN_KEY_MAX) {
                vmin = kk[e] < vmin ? kk[e] : vmin;
                vmax = kk[e] > vmax ? kk[e] : vmax;
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t x = shfl_xor_t<uint64_t>(vmin, o), y = shfl_xor_t<uint64_t>(vmax, o);
            vmin = x < vmin ? x : vmin;
            vmax = y > vmax ? y : vmax;
        }
        if (lane == 0) {
            s_mm[wave] = vmin;
            s_mm[nt / 64 + wave] = vmax;
        }
        __syncthreads();
        for (uint32_t w2 = 0; w2 < nt / 64; ++w2) {
            vmin = s_mm[w2] < vmin ? s_mm[w2] : vmin;
            vmax = s_mm[nt / 64 + w2] > vmax ? s_mm[nt / 64 + w2] : vmax;
        }
        uint32_t rank = m;
        for (;;) {
            uint32_t sh = 0;
            while (((vmax - vmin) >> sh) >= (uint64_t)kSelBinsMax) ++sh;
#pragma unroll
            for (int e = 0; e < VPT; ++e)
                if (kk[e] >= vmin && kk[e] <= vmax) atomicAdd(&s_hist[(uint32_t)((kk[e] - vmin) >> sh)], 1u);
            __syncthreads();
            const uint32_t bin = block_hist_rank_bin<nt>(s_hist, s_w, rank);
            const uint32_t rk = s_w[49], pop = s_hist[bin];
            const uint64_t lo = vmin + ((uint64_t)bin << sh);
            uint64_t hi = lo + (((uint64_t)1 << sh) - 1);
            if (hi > vmax || hi < lo) hi = vmax;
            if (sh == 0) {
                T = lo;
                break;
            }
            if (pop <= kSelListMax) {
#pragma unroll
                for (int e = 0; e < VPT; ++e)
                    if (kk[e] >= lo && kk[e] <= hi) s_slist[atomicAdd(&s_cn, 1u)] = kk[e];
                __syncthreads();
                for (uint32_t i = tid; i < pop; i += nt) {
                    const uint64_t v = s_slist[i];
                    uint32_t r = 0;
                    for (uint32_t j2 = 0; j2 < pop; ++j2) r += s_slist[j2] < v ? 1u : 0u;   // (keys are unique)
                    if (r + 1 == rk) s_T = v;
                }
                __syncthreads();
                T = s_T;
                break;
            }
            // a crowded bin (tie-heavy distances) is the new range
            vmin = lo;
            vmax = hi;
            rank = rk;
            __syncthreads();   // everyone has read the bin's count and rank
            clear();
            __syncthreads();
        }
    }

    auto decode = [&](uint64_t key, uint32_t i) {   // select_rerank_kernel's, without cand_dist
        const uint32_t vpos = (uint32_t)key;
        uint32_t lo = 0, hi = a.P;
        uint32_t csr;
        if (staged) {
            while (hi - lo > 1) {
                uint32_t mid = (lo + hi) >> 1;
                if (s_dvb[mid] <= vpos) lo = mid; else hi = mid;
            }
            csr = s_drow[lo] + (vpos - s_dvb[lo]);
        } else {
            while (hi - lo > 1) {
                uint32_t mid = (lo + hi) >> 1;
                if (vb[mid] <= vpos) lo = mid; else hi = mid;
            }
            csr = ix.leaf_off[a.tokens[(size_t)q * a.P + lo]] + (vpos - vb[lo]);
        }
        const uint32_t idx = ix.leaf_ids ? ix.leaf_ids[csr] : csr;
        a.cand_row[(size_t)q * m + i] = ix.rows_csr ? csr : idx;
        a.cand_key[(size_t)q * m + i] = key;
        a.cand_idx[(size_t)q * m + i] = idx;
    };
    // keep key <= T, in LIST order: the survivors' order follows the scan's, and the int8 bracket pass behind this
    // kernel gathers its rows in candidate order -- it takes 1.7 % longer behind slots handed out wave by wave.  The
    // kept keys of every 64-key run (e, wave) are counted by ballot, one wave scans the counts, no atomics
    constexpr uint32_t runs = (uint32_t)VPT * (nt / 64), per = (runs + 63u) / 64u;
    {
#pragma unroll
        for (int e = 0; e < VPT; ++e) {
            const unsigned long long kept = __ballot((uint32_t)e * nt + tid < cnt && kk[e] <= T);
            if (lane == 0) s_pre[(uint32_t)e * (nt / 64) + wave] = (uint32_t)__popcll(kept);
        }
        __syncthreads();
        if (wave == 0) {   // exclusive prefix over the runs, `per` consecutive runs a lane
            uint32_t c[per], mine = 0;
#pragma unroll
            for (uint32_t j = 0; j < per; ++j) {
                c[j] = lane * per + j < runs ? s_pre[lane * per + j] : 0u;
                mine += c[j];
            }
            uint32_t incl = mine;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
                if ((int)lane >= o) incl += up;
            }
            uint32_t excl = incl - mine;
#pragma unroll
            for (uint32_t j = 0; j < per; ++j) {
                if (lane * per + j < runs) s_pre[lane * per + j] = excl;
                excl += c[j];
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int e = 0; e < VPT; ++e) {
        const bool keep = (uint32_t)e * nt + tid < cnt && kk[e] <= T;
        uint32_t etot;
        const uint32_t slot = s_pre[(uint32_t)e * (nt / 64) + wave] + wave_prefix_count(keep, &etot);
        if (keep && slot < m) decode(kk[e], slot);   // (exactly min(m, cnt) are kept: the row has m slots)
    }
    if (tid == 0) a.cand_count[q] = min(m, cnt);
}

// =====================================================================================
// K8: exact re-rank.  tree_x_hybrid/mod.rs:350-358 -> squared_l2_avx2
// (simd/x86.rs:139-165): 8 lanes per candidate are the 8 AVX2 FMA lane chains (chunk
// order), combined by the fixed hsum tree (x86.rs:31-44) with DPP shuffles, plus the
// non-fused scalar tail.  32 candidates per 256-thread block, grid over (candidates,
// queries): the random row gathers are spread over the whole chip.
// =====================================================================================
// Exact distance of one (query, row) pair by a group of 8 lanes (lane8 = the AVX2 lane chain), with the
// measure of the re-ordering (utils/reordering.rs:35-44): squared_l2_avx2 / dot_product_avx2 /
// l1_distance_avx2 (simd/x86.rs) or the cosine of one_to_one.rs:559-612.  The result is valid in the
// group's lane 0 (act must be uniform over the group).
template <int U = 8>   // independent loads in flight per lane (U * 8 dims per memory round trip)
__device__ __forceinline__ float exact_pair_8lanes(const TxhIndexDev &ix, const float *s_q, const float *row, bool act,
                                                  uint32_t lane8) {
    const uint32_t dim = ix.dim, chunks = dim >> 3;
    float accv = 0.0f, aav = 0.0f, bbv = 0.0f;   // (aa / bb: Cosine's two extra lane chains)
    for (uint32_t i0 = 0; i0 < chunks; i0 += U) {
        float xv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) xv[u] = (act && i0 + u < chunks) ? row[8 * (i0 + u) + lane8] : 0.0f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (i0 + u < chunks) {
                const float qv = s_q[8 * (i0 + u) + lane8];
                if (ix.measure == SCANN_HIP_DOT_PRODUCT) {   // dot_product_avx2, x86.rs:72-96
                    accv = fmaf(qv, xv[u], accv);
                } else if (ix.measure == SCANN_HIP_L1) {     // l1_distance_avx2, x86.rs:103-132
                    accv = accv + fabsf(qv - xv[u]);
                } else if (ix.measure == SCANN_HIP_COSINE) { // cosine_similarity_f32_simd: add(mul), not fused
                    accv = accv + qv * xv[u];
                    aav = aav + qv * qv;
                    bbv = bbv + xv[u] * xv[u];
                } else {
                    const float diff = qv - xv[u];
                    accv = fmaf(diff, diff, accv);        // _mm256_fmadd_ps(diff, diff, sum)
                }
            }
        }
    }
    float r;
    float saa = 0.0f, sbb = 0.0f;
    if (ix.measure == SCANN_HIP_COSINE) {
        // wide 0.7 f32x8::reduce_add (non-AVX build): ((v0 + v1) + v2) + v3 per half, then lo + hi;
        // lane 0 of each half runs the chain with values shuffled in
        auto half_sum = [&](float v) {
            float h = v + __shfl_down(v, 1, 8);     // lanes 0, 4: v0 + v1
            h = h + __shfl_down(v, 2, 8);           // + v2
            h = h + __shfl_down(v, 3, 8);           // + v3
            return h + __shfl_down(h, 4, 8);        // lane 0: lo + hi
        };
        r = half_sum(accv);
        saa = half_sum(aav);
        sbb = half_sum(bbv);
    } else {
        // horizontal_sum_f32_avx2: (lo+hi) -> +movehdup -> +movehl
        const float s = accv + __shfl_down(accv, 4, 8);     // lanes 0..3: v[j] + v[j+4]
        const float t = s + __shfl_down(s, 1, 8);           // lane 0: s0+s1, lane 2: s2+s3
        r = t + __shfl_down(t, 2, 8);                       // lane 0: (s0+s1) + (s2+s3)
    }
    if (act && lane8 == 0) {
        for (uint32_t j = chunks * 8; j < dim; ++j) {   // scalar tail, not fused
            if (ix.measure == SCANN_HIP_DOT_PRODUCT) {
                r = r + s_q[j] * row[j];
            } else if (ix.measure == SCANN_HIP_L1) {
                r = r + fabsf(s_q[j] - row[j]);
            } else if (ix.measure == SCANN_HIP_COSINE) {
                r = r + s_q[j] * row[j];
                saa = saa + s_q[j] * s_q[j];
                sbb = sbb + row[j] * row[j];
            } else {
                const float diff = s_q[j] - row[j];
                r = r + diff * diff;
            }
        }
        // ReorderingHelper with the configured measure (utils/reordering.rs:35-44)
        if (ix.measure == SCANN_HIP_DOT_PRODUCT) r = -r;
        if (ix.measure == SCANN_HIP_L2) r = sqrtf(r);
        if (ix.measure == SCANN_HIP_COSINE) {
            const float na = sqrtf(saa), nb = sqrtf(sbb);
            r = 1.0f - ((na == 0.0f || nb == 0.0f) ? 0.0f : r / (na * nb));
        }
    }
    return r;
}

__global__ __launch_bounds__(256) void rerank_kernel(TxhIndexDev ix, const float *__restrict__ queries,
                                                     uint32_t q_stride, uint32_t m,
                                                     const uint32_t *__restrict__ cand_row,
                                                     const uint32_t *__restrict__ cand_count,
                                                     float *__restrict__ cand_exact) {
    extern __shared__ __attribute__((aligned(16))) float s_q[];   // [dim]
    const uint32_t q = blockIdx.y, tid = threadIdx.x;
    const uint32_t nsel = cand_count[q];
    const uint32_t c0 = blockIdx.x * 32u;
    if (c0 >= nsel) return;   // uniform
    const uint32_t dim = ix.dim;
    for (uint32_t j = tid; j < dim; j += blockDim.x) s_q[j] = queries[(size_t)q * q_stride + j];
    __syncthreads();
    const uint32_t lane8 = tid & 7u;
    const uint32_t c = c0 + (tid >> 3);
    const bool act = c < nsel;
    const float *row = ix.rows;
    if (act) row = ix.rows + (size_t)cand_row[(size_t)q * m + c] * ix.stride;
    const float r = exact_pair_8lanes(ix, s_q, row, act, lane8);
    if (act && lane8 == 0) {
        cand_exact[(size_t)q * m + c] = r;
    }
}

// K9: stable sort by exact distance (key = ordered(exact) << 32 | approx rank), first k.
// tree_x_hybrid/mod.rs:360-361.
__global__ __launch_bounds__(kSelectThreads) void final_sort_kernel(
    uint32_t m, uint32_t k, const uint32_t *__restrict__ cand_count,
    const uint32_t *__restrict__ cand_idx, const float *__restrict__ cand_exact,
    uint32_t *__restrict__ out_idx, float *__restrict__ out_dist, uint32_t *__restrict__ out_count) {
    extern __shared__ __attribute__((aligned(16))) uint64_t skeys[];
    const uint32_t q = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const uint32_t nsel = cand_count[q];
    uint32_t m2 = 1;
    while (m2 < nsel) m2 <<= 1;
    for (uint32_t i = tid; i < m2; i += nt)
        skeys[i] = (i < nsel) ? make_key(cand_exact[(size_t)q * m + i], i) : SCANN_KEY_MAX;
    __syncthreads();
    bitonic_sort_lds(skeys, m2);
    const uint32_t nout = min(k, nsel);   // truncate(k)
    for (uint32_t i = tid; i < k; i += nt) {
        uint32_t oi = kInvalid;
        float od = __builtin_inff();
        if (i < nout) {
            const uint64_t key = skeys[i];
            oi = cand_idx[(size_t)q * m + (uint32_t)key];
            od = ordered_to_f32((uint32_t)(key >> 32));
        }
        out_idx[(size_t)q * k + i] = oi;
        out_dist[(size_t)q * k + i] = od;
    }
    if (tid == 0) out_count[q] = nout;
}

// K9b: the same ordering without a sort, for small k and unsorted candidates: arg-min rounds
// over (ordered(exact), merge key) -- the merge key is monotone in the approximate rank, so
// this is exactly the stable sort's order.  Two levels without block-wide rounds: every wave
// extracts the k best of its share with wave shuffles only, then wave 0 extracts the k best
// of the (waves x k) finalists.
constexpr uint32_t kTopkMaxK = 64;

// One arg-min round over the per-lane best (b_eb, b_kk, b_sl) of a wave; returns the winner
// in every lane.  Exact-distance ties are rare: reduce the 32-bit distance first and fall
// back to the 96-bit reduction only when several lanes tie.
__device__ __forceinline__ void wave_argmin96(uint32_t &b_eb, uint64_t &b_kk, uint32_t &b_sl) {
    uint32_t mn = b_eb;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) mn = min(mn, (uint32_t)__shfl_xor((int)mn, d));
    const unsigned long long tie = __ballot(b_eb == mn);
    if (__popcll(tie) == 1) {
        const int src = __ffsll((long long)tie) - 1;
        b_eb = mn;
        b_sl = (uint32_t)__shfl((int)b_sl, src);
        const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)b_kk, src);
        const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(b_kk >> 32), src);
        b_kk = ((uint64_t)hi << 32) | lo;
        return;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o_eb = (uint32_t)__shfl_xor((int)b_eb, d), o_sl = (uint32_t)__shfl_xor((int)b_sl, d);
        const uint64_t o_kk = shfl_xor_t<uint64_t>(b_kk, d);
        if (o_eb < b_eb || (o_eb == b_eb && o_kk < b_kk)) {
            b_eb = o_eb;
            b_kk = o_kk;
            b_sl = o_sl;
        }
    }
}

template <int NT>
__global__ __launch_bounds__(NT) void final_topk_kernel(
    uint32_t m, uint32_t k, const uint32_t *__restrict__ cand_count,
    const uint32_t *__restrict__ cand_idx, const uint64_t *__restrict__ cand_key,
    const float *__restrict__ cand_exact, uint32_t *__restrict__ out_idx,
    float *__restrict__ out_dist, uint32_t *__restrict__ out_count) {
    constexpr int E = 8;                                  // candidates per thread: m <= 8 * NT
    constexpr int NWV = NT / 64;
    constexpr int E2 = NWV * kTopkMaxK / 64;              // finalists per lane of wave 0
    __shared__ uint32_t s_eb[NWV * kTopkMaxK];
    __shared__ uint64_t s_kk[NWV * kTopkMaxK];
    __shared__ uint32_t s_sl[NWV * kTopkMaxK];
    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nsel = cand_count[q];
    if (nsel & 0x80000000u) return;   // rerank_short_kernel already wrote this query's rows (block-uniform)
    const uint32_t nout = min(k, nsel);
    uint32_t eb[E];
    uint64_t kk[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const uint32_t slot = e * (uint32_t)NT + tid;
        const bool alive = slot < nsel;
        eb[e] = alive ? f32_to_ordered(cand_exact[(size_t)q * m + slot]) : 0xFFFFFFFFu;
        kk[e] = alive ? cand_key[(size_t)q * m + slot] : SCANN_KEY_MAX;
    }
    // level 1: the wave's nout best
    for (uint32_t r = 0; r < nout; ++r) {
        uint32_t b_eb = 0xFFFFFFFFu, b_sl = 0xFFFFFFFFu;
        uint64_t b_kk = SCANN_KEY_MAX;
#pragma unroll
        for (int e = 0; e < E; ++e)
            if ((uint32_t)e * (uint32_t)NT < nsel && (eb[e] < b_eb || (eb[e] == b_eb && kk[e] < b_kk))) {
                b_eb = eb[e];
                b_kk = kk[e];
                b_sl = e * (uint32_t)NT + tid;
            }
        wave_argmin96(b_eb, b_kk, b_sl);
        if (b_sl != 0xFFFFFFFFu && (b_sl & ((uint32_t)NT - 1)) == tid) {
            const uint32_t we = b_sl / (uint32_t)NT;
#pragma unroll
            for (int e = 0; e < E; ++e)
                if ((uint32_t)e == we) {
                    eb[e] = 0xFFFFFFFFu;
                    kk[e] = SCANN_KEY_MAX;
                }
        }
        if (lane == 0) {
            s_eb[wave * nout + r] = b_eb;
            s_kk[wave * nout + r] = b_kk;
            s_sl[wave * nout + r] = b_sl;
        }
    }
    __syncthreads();
    // level 2: wave 0 takes the nout best of the NWV * nout finalists
    if (wave == 0) {
        const uint32_t nfin = NWV * nout;
        uint32_t feb[E2], fsl[E2];
        uint64_t fkk[E2];
#pragma unroll
        for (int e = 0; e < E2; ++e) {
            const uint32_t i = e * 64 + lane;
            const bool alive = i < nfin;
            feb[e] = alive ? s_eb[i] : 0xFFFFFFFFu;
            fkk[e] = alive ? s_kk[i] : SCANN_KEY_MAX;
            fsl[e] = alive ? s_sl[i] : 0xFFFFFFFFu;
        }
        for (uint32_t r = 0; r < nout; ++r) {
            uint32_t b_eb = 0xFFFFFFFFu, b_sl = 0xFFFFFFFFu;
            uint64_t b_kk = SCANN_KEY_MAX;
#pragma unroll
            for (int e = 0; e < E2; ++e)
                if ((uint32_t)e * 64 < nfin && (feb[e] < b_eb || (feb[e] == b_eb && fkk[e] < b_kk))) {
                    b_eb = feb[e];
                    b_kk = fkk[e];
                    b_sl = fsl[e];
                }
            wave_argmin96(b_eb, b_kk, b_sl);
#pragma unroll
            for (int e = 0; e < E2; ++e)
                if (fsl[e] == b_sl) {   // slots are unique: exactly one lane/element matches
                    feb[e] = 0xFFFFFFFFu;
                    fkk[e] = SCANN_KEY_MAX;
                    fsl[e] = 0xFFFFFFFEu;
                }
            if (lane == 0) {
                out_idx[(size_t)q * k + r] = cand_idx[(size_t)q * m + b_sl];
                out_dist[(size_t)q * k + r] = ordered_to_f32(b_eb);
            }
        }
    }
    for (uint32_t i = nout + tid; i < k; i += blockDim.x) {
        out_idx[(size_t)q * k + i] = kInvalid;
        out_dist[(size_t)q * k + i] = __builtin_inff();
    }
    if (tid == 0) out_count[q] = nout;
}

// =====================================================================================
// K8b: exact re-rank behind an int8 row filter (low-precision row stores as
// shortlist filters; the reference's int8 rows: distance_measures/one_to_many_asymmetric.rs:25-377,
// brute_force/scalar_quantized.rs:168-260).
//
// reorder_results (tree_x_hybrid/mod.rs:342-364) scores ALL m candidates exactly and keeps k of
// them; at m = 5000 that is 2.6 GB of random 512-byte row gathers per 1024 queries, as long as the
// scan.  Here every row also exists as int8 (per-row scale s = max|x| / 127, q = round(x / s),
// x~ = s q) with its quantisation error E = ||x - x~|| stored beside it.  For a query q:
//     d~ = ||q - x~||^2,   | ||q - x||^2 - d~ |  <=  2 sqrt(d~) E + E^2
// so [L, U] = d~ -+ (2 sqrt(d~) E + E^2 + slack) brackets the reference's f32 distance (slack covers
// the f32 rounding of both sums).  With tau = the k-th smallest U, at least k candidates lie at or
// under tau, so a candidate with L > tau can neither enter the top k nor tie with it: only the
// shortlist {L <= tau} (tens of rows) is scored with the reference's arithmetic, and the result --
// indices, distances, tie order -- is the one the full re-rank gives.
//   rerank_i8_kernel     L, U of every candidate (128-byte int8 rows instead of 512-byte f32 rows)
//   rerank_short_kernel  block per query: tau, shortlist, exact distances (rerank_kernel's
//                        arithmetic), the k best by (exact, merge key), output rows
// =====================================================================================
// uni_scale > 0: every row with that one scale (the store of rerank_i8_kernel's UNIFORM form, see the launcher)
constexpr uint32_t kShortMaxFast = 1024;   // shortlists up to this size finish inside rerank_short_kernel

struct ShortArgs {
    uint32_t m, k;
    const float *queries;
    uint32_t q_stride;
    const uint32_t *lb, *ub;
    const uint32_t *cand_row, *cand_idx;
    const uint64_t *cand_key;
    uint32_t *cand_count;     // fallback: left as is; fast path: top bit set so that final_topk skips the query
    float *cand_exact;        // fallback: exact of the shortlist, +inf elsewhere
    uint32_t *out_idx;
    float *out_dist;
    uint32_t *out_count;
    // > 0: the LOCAL stage of a leaf-sharded search (lists sorted by merge key).  This rank's share of the global
    // candidates (the m smallest keys over all ranks) is a PREFIX of its list, and the final rows are the k best exact
    // distances within the union of those prefixes: a candidate past the first local_head entries whose lower bound
    // lies above tau = the k-th smallest upper bound among the first local_head entries has k candidates with smaller
    // keys AND smaller exact distances in every prefix that contains it, so it can never reach the final k.  Its exact
    // distance is not computed: it travels as +inf (it still counts as one of the m candidates in the merge).  The
    // first local_head entries always get their exact distance.  No final rows are written in this mode.
    uint32_t local_head;
};

constexpr uint32_t kShortVPT = kMaxPreReorderK / 256;   // upper bounds per thread (registers)
constexpr uint32_t kLocalHead = 256;                    // entries of a sharded rank's list that are always re-ranked exactly

__global__ __launch_bounds__(256) void rerank_short_kernel(TxhIndexDev ix, ShortArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_q[];   // [dim]
    __shared__ uint32_t s_mins[256], s_tlist[1024], s_hist[1024], s_slist[256], s_tcnt;
    __shared__ uint64_t s_red[48];
    __shared__ uint32_t s_pos[kShortMaxFast], s_eb[kShortMaxFast];
    __shared__ uint64_t s_kk[kShortMaxFast];
    __shared__ uint32_t s_ns;
    const uint32_t q = blockIdx.x, tid = threadIdx.x, nt = 256;
    const uint32_t m = a.m, k = a.k;
    const uint32_t nsel = a.cand_count[q];
    const uint32_t nout = min(k, nsel);
    for (uint32_t j = tid; j < ix.dim; j += nt) s_q[j] = a.queries[(size_t)q * a.q_stride + j];
    if (tid == 0) s_ns = 0;
    // tau = k-th smallest upper bound (everything is shortlisted when there are at most k candidates): a
    // tail rank, so the bounds stay in registers and only those under a pivot are ranked
    // (block_tail_select; an inexact result is the pivot, >= tau: a larger shortlist, still complete)
    uint32_t tau = 0xFFFFFFFFu;
    const uint32_t head = a.local_head;                        // (0: single-GPU final stage)
    const uint32_t ntau = head ? min(nsel, head) : nsel;       // entries whose upper bounds define tau
    if (ntau > k) {   // block-uniform
        uint32_t ubv[kShortVPT];   // (registers: 256 threads leave room, and the bounds are read once)
#pragma unroll
        for (int u = 0; u < (int)kShortVPT; ++u) {
            const uint32_t i = (uint32_t)u * nt + tid;
            ubv[u] = i < ntau ? a.ub[(size_t)q * m + i] : 0xFFFFFFFFu;
        }
        auto v = [&](int u) -> uint32_t { return ubv[u]; };
        bool exact;
        tau = block_tail_select<(int)kShortVPT>(v, k, s_mins, s_tlist, 1024, s_hist, s_slist, s_red, &s_tcnt, &exact);
    }
    __syncthreads();
    for (uint32_t b0 = 0; b0 < nsel; b0 += nt) {
        const uint32_t i = b0 + tid;
        const bool keep = i < nsel && (i < head || a.lb[(size_t)q * m + i] <= tau);
        uint32_t wtot;
        const uint32_t wpre = wave_prefix_count(keep, &wtot);
        uint32_t base = 0;
        if ((tid & 63u) == 0 && wtot) base = atomicAdd(&s_ns, wtot);
        base = (uint32_t)__shfl((int)base, 0);
        if (keep && base + wpre < kShortMaxFast) s_pos[base + wpre] = i;
        if (head && i < nsel && !keep) a.cand_exact[(size_t)q * m + i] = __builtin_inff();   // (local stage: see ShortArgs)
    }
    __syncthreads();
    const uint32_t ns = s_ns;
    // (a shortlist under nout rows means a bracket did not hold: the query is re-ranked without the filter, and the
    // fast path's nout arg-min rounds never run past s_pos[ns - 1])
    const bool unfiltered = ns < nout;
    const bool fast = ns <= kShortMaxFast && !unfiltered;
    // exact distances of the shortlist: rerank_kernel's arithmetic (8 FMA lane chains, fixed hsum tree,
    // unfused tail: simd/x86.rs:139-165, 31-44)
    const uint32_t chunks = ix.dim >> 3, lane8 = tid & 7u;
    const uint32_t total = fast ? ns : nsel;
    // (kShortR rows per 8-lane group and pass, their row gathers in flight together: one row per pass left every pass
    // waiting for a 512-byte gather from HBM -- 284 us at 10M x 128, m = 8192, where shortlists hold hundreds of rows)
    constexpr int kShortR = 4;
    for (uint32_t b0 = 0; b0 < total; b0 += (nt / 8) * kShortR) {
        uint32_t jx[kShortR], ci[kShortR];
        bool act[kShortR], listed[kShortR];
        const float *rowp[kShortR];
#pragma unroll
        for (int u = 0; u < kShortR; ++u) {
            jx[u] = b0 + (uint32_t)u * (nt / 8) + (tid >> 3);
            act[u] = jx[u] < total;
            ci[u] = 0;
            listed[u] = false;
            if (act[u]) {
                ci[u] = fast ? s_pos[jx[u]] : jx[u];
                listed[u] = fast || unfiltered || ci[u] < head || a.lb[(size_t)q * m + ci[u]] <= tau;
            }
            rowp[u] = ix.rows + (size_t)(listed[u] ? a.cand_row[(size_t)q * m + ci[u]] : 0u) * ix.stride;
        }
        float accv[kShortR];
#pragma unroll
        for (int u = 0; u < kShortR; ++u) accv[u] = 0.0f;
        for (uint32_t c = 0; c < chunks; ++c) {
#pragma unroll
            for (int u = 0; u < kShortR; ++u) {
                const float diff = s_q[8 * c + lane8] - rowp[u][8 * c + lane8];
                accv[u] = fmaf(diff, diff, accv[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < kShortR; ++u) {
            const float s1 = accv[u] + __shfl_down(accv[u], 4, 8);
            const float t1 = s1 + __shfl_down(s1, 1, 8);
            float r = t1 + __shfl_down(t1, 2, 8);
            if (lane8 == 0)
                for (uint32_t j = chunks * 8; j < ix.dim; ++j) {
                    const float diff = s_q[j] - rowp[u][j];
                    r = r + diff * diff;
                }
            if (!listed[u]) r = __builtin_inff();
            if (act[u] && lane8 == 0) {
                if (fast && !head) {
                    s_eb[jx[u]] = f32_to_ordered(r);
                    s_kk[jx[u]] = a.cand_key[(size_t)q * m + ci[u]];
                } else {
                    a.cand_exact[(size_t)q * m + ci[u]] = r;   // +inf outside the shortlist: final_topk orders the rest
                }
            }
        }
    }
    if (!fast || head) return;   // block-uniform: final_topk_kernel / the multi-GPU merge finish this query from cand_exact
    __syncthreads();
    // the k best of the shortlist by (exact, merge key) = the stable sort's first k: wave 0 runs k arg-min
    // rounds over its lanes' strided entries (ns <= 1024: <= 16 per lane)
    if (tid < 64) {
        constexpr int E = kShortMaxFast / 64;
        uint32_t eb[E];
        uint64_t kk[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const uint32_t j = (uint32_t)e * 64u + tid;
            eb[e] = j < ns ? s_eb[j] : 0xFFFFFFFFu;
            kk[e] = j < ns ? s_kk[j] : SCANN_KEY_MAX;
        }
        for (uint32_t r0 = 0; r0 < nout; ++r0) {
            uint32_t b_eb = 0xFFFFFFFFu, b_sl = 0xFFFFFFFFu;
            uint64_t b_kk = SCANN_KEY_MAX;
#pragma unroll
            for (int e = 0; e < E; ++e)
                if ((uint32_t)e * 64u < ns && (eb[e] < b_eb || (eb[e] == b_eb && kk[e] < b_kk))) {
                    b_eb = eb[e];
                    b_kk = kk[e];
                    b_sl = (uint32_t)e * 64u + tid;
                }
            wave_argmin96(b_eb, b_kk, b_sl);
            if (b_sl != 0xFFFFFFFFu && (b_sl & 63u) == tid) {
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if ((uint32_t)e == (b_sl >> 6)) {
                        eb[e] = 0xFFFFFFFFu;
                        kk[e] = SCANN_KEY_MAX;
                    }
            }
            if (tid == 0) {
                a.out_idx[(size_t)q * k + r0] = a.cand_idx[(size_t)q * m + s_pos[b_sl]];
                a.out_dist[(size_t)q * k + r0] = ordered_to_f32(b_eb);
            }
        }
    }
    for (uint32_t i = nout + tid; i < k; i += nt) {
        a.out_idx[(size_t)q * k + i] = kInvalid;
        a.out_dist[(size_t)q * k + i] = __builtin_inff();
    }
    if (tid == 0) {
        a.out_count[q] = nout;
        a.cand_count[q] = 0x80000000u;   // final_topk_kernel has nothing left to do for this query
    }
}

// =====================================================================================
// Small batches (nq <= 16, short candidate streams): the search as THREE launches -- or ONE.
//
// The batched pipeline above groups (query, leaf) pairs by leaf, samples a filter bound and scans
// through tile queues: ~12 dependent launches, each ~4 us of dispatch on its own -- ~115-150 us of
// device time for ONE query, of which the scan is 15-40.  For a handful of queries none of that
// machinery pays:
//   1. select_leaves_kernel with inline centroid scoring            TreePartitioner::partition
//   2. small_scan_kernel: one workgroup per (query, leaf, chunk of points) builds the pair's table
//      in LDS (lut_build_kernel's arithmetic) and writes EVERY point's merge key at its stream
//      position (dense list, no bound, no atomics)                  mod.rs:297-339
//   3. small_finish_kernel: block per query: the m smallest keys (rank select), decode, exact
//      distances (exact_pair_8lanes), the k best by (exact, merge key)   mod.rs:283-293, 342-364
// small_fused_kernel (below) runs the three stages in one launch for exact-scan indexes and flat
// hashers.  Same keys, same arithmetic, same order: rows identical to the batched pipeline's.
// (Tried for the finish stage's rank select of a handful of keys: a tournament of 64-bit wave minima,
// m rounds per wave and m over the finalists -- slower than block_select's histogram passes.)
// =====================================================================================
constexpr uint32_t kSmallChunk = 1024;      // points per workgroup of the scan
constexpr uint32_t kSmallMaxM = 1024;       // candidates the finish kernel keeps in LDS
constexpr uint32_t kFinGroups = 4096;       // sub-stream minima of the finish kernel's tail select

// exact_pair_thread (pair.h): the exact distance of one (query, row) pair by ONE thread.

struct SmallArgs {
    uint32_t nq, P, m, k, cap, q_stride;
    int exact_reorder;
    const float *queries;
    const uint32_t *tokens, *vbase;
    uint64_t *cand;           // [nq][cap] dense: key of stream position v at cand[q][v]
    uint32_t *counters;
    const uint64_t *allow;
    uint64_t allow_bits, allow_stride;
    uint32_t *out_idx;
    float *out_dist;
    uint32_t *out_count;
    uint32_t *done;           // pinned completion flags [nq] of a host call (or nullptr) and their value
    uint32_t seq;
    uint32_t chunk;           // points per workgroup of the scan (a multiple of 256)
};

__global__ __launch_bounds__(256) void small_scan_kernel(TxhIndexDev ix, SmallArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_lut[];   // [S][kp] then [dim] residual query
    const uint32_t pair = blockIdx.y, q = pair / a.P, r = pair - q * a.P, chunk = blockIdx.x, tid = threadIdx.x;
    if (pair == 0 && chunk == 0 && tid == 0) a.counters[CNT_STATUS] = 0;
    const uint32_t leaf = a.tokens[(size_t)q * a.P + r];
    const uint32_t lb = ix.leaf_off[leaf], size = ix.leaf_off[leaf + 1] - lb;
    const uint32_t c0 = chunk * a.chunk;
    if (c0 >= size) return;   // block-uniform
    const uint32_t S = ix.S, K = ix.K, dsub = ix.dsub, kp = ix.kp, dim = ix.dim;
    if (ix.exact_scan) {
        // SearchMode::Partitioned (scann.rs:213-252) and brute force: every row scored exactly; the dense
        // key list is then the whole result stream and the finish kernel takes its k smallest keys
        float *s_qe = s_lut;
        for (uint32_t j = tid; j < dim; j += 256) s_qe[j] = a.queries[(size_t)q * a.q_stride + j];
        __syncthreads();
        const uint32_t vbe = a.vbase[(size_t)q * (a.P + 1) + r];
        uint64_t *oute = a.cand + (size_t)q * a.cap;
        for (uint32_t j = c0 + tid; j < min(size, c0 + a.chunk); j += 256) {
            const uint32_t csr = lb + j;
            const float *row = ix.rows + (size_t)(ix.rows_csr ? csr : ix.leaf_ids[csr]) * ix.stride;
            const float dist = exact_pair_thread(ix.measure, dim, s_qe, row);
            const uint32_t vpos = vbe + j;
            if (vpos < a.cap) oute[vpos] = row_allowed(ix, a.allow, a.allow_stride, q, a.allow_bits, csr) ? make_key(dist, vpos) : SCANN_KEY_MAX;
        }
        return;
    }
    float *s_qr = s_lut + S * kp;
    for (uint32_t j = tid; j < dim; j += 256) {   // residual q - centroid (mod.rs:309-316)
        float v = a.queries[(size_t)q * a.q_stride + j];
        if (ix.use_residuals) v = v - ix.centers[(size_t)leaf * dim + j];
        s_qr[j] = v;
    }
    __syncthreads();
    for (uint32_t e = tid; e < S * kp; e += 256) {   // LookupTable::from_query (lut.rs:47-70, codebook.rs:98-115)
        const uint32_t sub = e / kp, c = e - sub * kp;
        float acc = 0.0f;
        if (c < K) {
            const float *cb = ix.codebook + ((size_t)sub * K + c) * dsub;
            for (uint32_t j = 0; j < dsub; ++j) {
                const float d = s_qr[sub * dsub + j] - cb[j];
                acc = acc + d * d;
            }
        }
        s_lut[e] = acc;
    }
    __syncthreads();
    const uint32_t vb = a.vbase[(size_t)q * (a.P + 1) + r];
    const uint32_t bits = ix.code_bits, per = 32u / bits, mask = (1u << bits) - 1u, nw = ix.nw;
    uint64_t *out = a.cand + (size_t)q * a.cap;
    for (uint32_t j = c0 + tid; j < min(size, c0 + a.chunk); j += 256) {
        const uint32_t *w = ix.codes + (size_t)(lb + j) * nw;
        float acc = 0.0f;   // LookupTable::compute_distance (lut.rs:74-82): 0.0 + lut[0][c0] + lut[1][c1] ...
        for (uint32_t sub = 0; sub < S; ++sub) {
            const uint32_t code = (w[sub / per] >> (bits * (sub % per))) & mask;
            const float tv = s_lut[sub * kp + code];
            acc = sub == 0 ? tv : acc + tv;
        }
        const uint32_t vpos = vb + j;
        if (vpos < a.cap)
            out[vpos] = row_allowed(ix, a.allow, a.allow_stride, q, a.allow_bits, lb + j) ? make_key(acc, vpos) : SCANN_KEY_MAX;
    }
}

// The finish stage: body of small_finish_kernel and last stage of small_fused_kernel (there vbq / tokq are
// the workgroup's LDS copies of the query's key bases and tokens).
// AGENT: the key list was written by other workgroups of the SAME launch (agent-scope write-through stores):
// read it with agent-scope loads (the per-XCD L2s are not coherent with each other inside a kernel).
template <bool AGENT>
__device__ __forceinline__ uint64_t list_key(const uint64_t *p) {
    if constexpr (AGENT) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}

template <bool AGENT>
__device__ __forceinline__ void small_finish_body(const TxhIndexDev &ix, const SmallArgs &a, uint32_t q, float *s_q,
                                                  const uint32_t *vbq, const uint32_t *tokq) {
    __shared__ uint64_t s_keys[kSmallMaxM], s_slist[kSelListMax], s_red[48], s_fin[kFinGroups];
    __shared__ uint32_t s_hist[kSelBinsMax], s_eb[kSmallMaxM], s_idx[kSmallMaxM], s_n;
    const uint32_t tid = threadIdx.x, nt = kSelectThreads;
    const uint32_t P = a.P, m = a.m, k = a.k;
    // result rows: plain stores, or -- when the host polls a completion flag in the same pinned buffer --
    // system-scope write-through stores (visible to the host once they have completed)
    const bool polled = a.done != nullptr;
    auto out_store = [&](auto *p, auto v) {
        if (polled) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        else *p = v;
    };
    const uint32_t cnt = min(vbq[P], a.cap);
    const uint64_t *list = a.cand + (size_t)q * a.cap;
    for (uint32_t j = tid; j < ix.dim; j += nt) s_q[j] = a.queries[(size_t)q * a.q_stride + j];
    if (tid == 0) s_n = 0;
    __syncthreads();
    // the m smallest keys (keys are unique; SCANN_KEY_MAX = a point the restrict filter rejected).  m is
    // far down the stream's tail (1000 of 100 k), so: minima of kFinGroups interleaved sub-streams -> the
    // m-th smallest minimum is a pivot just above the m-th smallest key (the m smallest minima are m
    // distinct keys) -> only the keys under the pivot are ranked.  Two passes over the list instead of
    // the histogram select's five; the histogram select remains for m close to cnt.
    uint64_t T = SCANN_KEY_MAX - 1;
    uint32_t from_fin = 0;   // > 0: the candidates are among s_fin[0 .. from_fin)
    if (cnt > m) {
        bool done = false;
        if (cnt <= kFinGroups) {   // a short stream: one load of the list into LDS, everything else there
            for (uint32_t i = tid; i < cnt; i += nt) s_fin[i] = list_key<AGENT>(list + i);
            __syncthreads();
            const uint64_t t = block_select<uint64_t>(s_fin, cnt, m, sel_cfg(cnt), s_hist, s_slist, s_red);
            if (t != SCANN_KEY_MAX) T = t;
            done = true;
            from_fin = cnt;
            __syncthreads();
        } else if ((uint64_t)m * 4 <= kFinGroups) {
            // Both passes read the list as 16-byte pairs, four loads in flight per thread (one workgroup
            // streams 800 KB at 100 k points: the passes are bound by its load round trips).  `head` = one
            // leading key when the list starts on an odd 8-byte slot; a last odd key is `tail`.
            constexpr int G = kFinGroups / kSelectThreads;   // minima per thread (any partition of the list works)
            const uint32_t head = (reinterpret_cast<uintptr_t>(list) & 8u) ? 1u : 0u;
            const uint32_t npairs = (cnt - head) >> 1;
            const bool tail = ((cnt - head) & 1u) != 0;
            const ulonglong2 *pairs = reinterpret_cast<const ulonglong2 *>(list + head);
            uint64_t mn[G];
#pragma unroll
            for (int g = 0; g < G; ++g) mn[g] = SCANN_KEY_MAX;
            for (uint32_t p0 = 0; p0 < npairs; p0 += nt * G) {
                ulonglong2 v[G];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const uint32_t pi = p0 + (uint32_t)g * nt + tid;
                    v[g] = make_ulonglong2(SCANN_KEY_MAX, SCANN_KEY_MAX);
                    if (pi < npairs) {
                        if constexpr (AGENT) {
                            v[g].x = list_key<true>(list + head + 2 * (size_t)pi);
                            v[g].y = list_key<true>(list + head + 2 * (size_t)pi + 1);
                        } else {
                            v[g] = pairs[pi];
                        }
                    }
                }
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const uint64_t lo2 = v[g].x < v[g].y ? v[g].x : v[g].y;
                    mn[g] = lo2 < mn[g] ? lo2 : mn[g];
                }
            }
            if (tid == 0 && head) { const uint64_t k0 = list_key<AGENT>(list); mn[0] = k0 < mn[0] ? k0 : mn[0]; }
            if (tid == 1 && tail) { const uint64_t k1 = list_key<AGENT>(list + cnt - 1); mn[0] = k1 < mn[0] ? k1 : mn[0]; }
#pragma unroll
            for (int g = 0; g < G; ++g) s_fin[(uint32_t)g * nt + tid] = mn[g];
            __syncthreads();
            const SelCfg gcfg = sel_cfg(kFinGroups);
            const uint64_t pivot = block_select<uint64_t>(s_fin, kFinGroups, m, gcfg, s_hist, s_slist, s_red);
            __syncthreads();
            if (pivot != SCANN_KEY_MAX) {
                if (tid == 0) s_n = 0;
                __syncthreads();
                // keys under the pivot -> s_fin (reused): ~1 % of the list, one LDS atomic each
                auto take = [&](uint64_t key) {
                    if (key <= pivot) {
                        const uint32_t pos = atomicAdd(&s_n, 1u);
                        if (pos < kFinGroups) s_fin[pos] = key;
                    }
                };
                for (uint32_t p0 = 0; p0 < npairs; p0 += nt * G) {
                    ulonglong2 v[G];
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        const uint32_t pi = p0 + (uint32_t)g * nt + tid;
                        v[g] = make_ulonglong2(SCANN_KEY_MAX, SCANN_KEY_MAX);
                    if (pi < npairs) {
                        if constexpr (AGENT) {
                            v[g].x = list_key<true>(list + head + 2 * (size_t)pi);
                            v[g].y = list_key<true>(list + head + 2 * (size_t)pi + 1);
                        } else {
                            v[g] = pairs[pi];
                        }
                    }
                    }
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        take(v[g].x);
                        take(v[g].y);
                    }
                }
                if (tid == 0 && head) take(list_key<AGENT>(list));
                if (tid == 1 && tail) take(list_key<AGENT>(list + cnt - 1));
                __syncthreads();
                const uint32_t c2 = s_n;
                __syncthreads();
                if (c2 <= kFinGroups) {   // (>= m by construction)
                    const uint64_t t = block_select<uint64_t>(s_fin, c2, m, sel_cfg(c2), s_hist, s_slist, s_red);
                    if (t != SCANN_KEY_MAX) T = t;
                    done = true;
                    from_fin = c2;       // the m smallest keys are all among these: no third pass over the list
                    __syncthreads();
                }
                if (tid == 0) s_n = 0;
                __syncthreads();
            }
        }
        if (!done) {
            const SelCfg cfg = sel_cfg(cnt);
            const uint64_t t = block_select<uint64_t, AGENT>(list, cnt, m, cfg, s_hist, s_slist, s_red);
            if (t != SCANN_KEY_MAX) T = t;   // fewer than m allowed points: keep them all
            __syncthreads();
        }
    }

    const uint64_t *src = from_fin ? s_fin : list;
    const uint32_t nsrc = from_fin ? from_fin : cnt;
    for (uint32_t b0 = 0; b0 < nsrc; b0 += nt) {
        const uint32_t i = b0 + tid;
        uint64_t key = SCANN_KEY_MAX;
        if (i < nsrc) key = from_fin ? src[i] : list_key<AGENT>(src + i);
        const bool keep = key <= T;
        uint32_t wtot;
        const uint32_t wpre = wave_prefix_count(keep, &wtot);
        uint32_t base = 0;
        if ((tid & 63u) == 0 && wtot) base = atomicAdd(&s_n, wtot);
        base = (uint32_t)__shfl((int)base, 0);
        if (keep && base + wpre < kSmallMaxM) s_keys[base + wpre] = key;
    }
    __syncthreads();
    const uint32_t nsel = min(s_n, min(m, kSmallMaxM));

    // decode tables of this query (key base and first CSR row of each selected leaf) in LDS: the
    // per-candidate chain vbase -> token -> leaf_off is otherwise three dependent global loads per pass
    uint32_t *s_dvb = reinterpret_cast<uint32_t *>(s_fin), *s_drow = s_dvb + kDecodeStage;   // (s_fin is free now)
    const bool staged = P <= kDecodeStage;
    if (staged)
        for (uint32_t r = tid; r < P; r += nt) {
            s_dvb[r] = vbq[r];
            s_drow[r] = ix.leaf_off[tokq[r]];
        }
    __syncthreads();
    // decode + exact distance: 8 lanes per candidate.  The passes' row ids first (their leaf_ids loads
    // travel together), then one memory round trip per candidate row of up to 128 dims.
    const uint32_t lane8 = tid & 7u;
    constexpr uint32_t kPasses = kSmallMaxM / (kSelectThreads / 8);
    uint32_t idxs[kPasses], rowis[kPasses];
#pragma unroll
    for (uint32_t ps = 0; ps < kPasses; ++ps) {
        const uint32_t c = ps * (nt / 8) + (tid >> 3);
        uint32_t idx = 0, rowi = 0;
        if (c < nsel) {
            const uint32_t vpos = (uint32_t)s_keys[c];
            uint32_t lo = 0, hi = P;
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if ((staged ? s_dvb[mid] : vbq[mid]) <= vpos) lo = mid; else hi = mid;
            }
            const uint32_t csr = staged ? s_drow[lo] + (vpos - s_dvb[lo])
                                        : ix.leaf_off[tokq[lo]] + (vpos - vbq[lo]);
            idx = ix.leaf_ids ? ix.leaf_ids[csr] : csr;
            rowi = ix.rows_csr ? csr : idx;
        }
        idxs[ps] = idx;
        rowis[ps] = rowi;
    }
#pragma unroll
    for (uint32_t ps = 0; ps < kPasses; ++ps) {
        const uint32_t c = ps * (nt / 8) + (tid >> 3);
        if (ps * (nt / 8) >= nsel) break;   // block-uniform
        const bool act = c < nsel;
        float r = 0.0f;
        if (a.exact_reorder) r = exact_pair_8lanes<16>(ix, s_q, ix.rows + (size_t)rowis[ps] * ix.stride, act, lane8);
        if (act && lane8 == 0) {
            s_idx[c] = idxs[ps];
            // without re-ordering the k best by approximate distance are wanted: order by the key itself
            s_eb[c] = a.exact_reorder ? f32_to_ordered(r) : (uint32_t)(s_keys[c] >> 32);
        }
    }
    __syncthreads();

    const uint32_t nout = min(k, nsel);
    if (nsel <= 64u) {
        // few candidates (m = k: exact scans, hashers without re-ordering): one per lane of wave 0, each lane
        // counts the candidates ahead of it in the (exact, merge key) order and writes its row at that rank
        if (tid < 64) {
            const uint32_t eb = tid < nsel ? s_eb[tid] : 0xFFFFFFFFu;
            const uint64_t kk = tid < nsel ? s_keys[tid] : SCANN_KEY_MAX;
            uint32_t rank = 0;
            for (uint32_t j = 0; j < nsel; ++j) {
                const uint32_t oe = (uint32_t)__shfl((int)eb, (int)j);
                const uint64_t ok = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(kk >> 32), (int)j) << 32) |
                                    (uint32_t)__shfl((int)(uint32_t)kk, (int)j);
                rank += (oe < eb || (oe == eb && ok < kk)) ? 1u : 0u;
            }
            if (tid < nsel && rank < nout) {
                out_store(&a.out_idx[(size_t)q * k + rank], s_idx[tid]);
                out_store(&a.out_dist[(size_t)q * k + rank], ordered_to_f32(eb));
            }
        }
    } else {
        // the k best by (exact, merge key), two levels: every wave extracts the k best of ITS 64 candidates (one
        // per lane: a round is one wave arg-min), then wave 0 the k best of the waves' finalists
        // (s_hist / s_slist are free by now: [0, 1024) ordered exact, [1024, 2048) candidate slot; merge keys)
        const uint32_t wave = tid >> 6, lane = tid & 63u;
        const uint32_t nwv = (nsel + 63u) >> 6;           // waves that hold candidates
        uint32_t *f_eb = s_hist, *f_sl = s_hist + kSmallMaxM;
        uint64_t *f_kk = s_slist;
        {
            uint32_t eb = tid < nsel ? s_eb[tid] : 0xFFFFFFFFu;
            uint64_t kk = tid < nsel ? s_keys[tid] : SCANN_KEY_MAX;
            if (wave < nwv) {
                for (uint32_t r0 = 0; r0 < nout; ++r0) {
                    uint32_t b_eb = eb, b_sl = kk == SCANN_KEY_MAX ? 0xFFFFFFFFu : tid;
                    uint64_t b_kk = kk;
                    wave_argmin96(b_eb, b_kk, b_sl);
                    if (b_sl == tid) {   // the winner leaves the pool
                        eb = 0xFFFFFFFFu;
                        kk = SCANN_KEY_MAX;
                    }
                    if (lane == 0) {
                        f_eb[wave * nout + r0] = b_eb;
                        f_kk[wave * nout + r0] = b_kk;
                        f_sl[wave * nout + r0] = b_sl;
                    }
                }
            }
        }
        __syncthreads();
        if (tid < 64) {
            constexpr int E = kSmallMaxM / 64;
            const uint32_t nfin = nwv * nout;             // <= 16 * 64
            uint32_t eb[E], sl[E];
            uint64_t kk[E];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const uint32_t j = (uint32_t)e * 64u + tid;
                const bool ok = j < nfin && f_sl[j] != 0xFFFFFFFFu;
                eb[e] = ok ? f_eb[j] : 0xFFFFFFFFu;
                kk[e] = ok ? f_kk[j] : SCANN_KEY_MAX;
                sl[e] = ok ? f_sl[j] : 0xFFFFFFFFu;
            }
            for (uint32_t r0 = 0; r0 < nout; ++r0) {
                uint32_t b_eb = 0xFFFFFFFFu, b_sl = 0xFFFFFFFFu;
                uint64_t b_kk = SCANN_KEY_MAX;
                int b_e = -1;
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if ((uint32_t)e * 64u < nfin && sl[e] != 0xFFFFFFFFu &&
                        (eb[e] < b_eb || (eb[e] == b_eb && kk[e] < b_kk))) {
                        b_eb = eb[e];
                        b_kk = kk[e];
                        b_sl = sl[e];
                        b_e = e;
                    }
                const uint32_t mine = b_sl;
                wave_argmin96(b_eb, b_kk, b_sl);
                if (b_sl != 0xFFFFFFFFu && mine == b_sl) {   // (candidate slots are unique: exactly one lane)
#pragma unroll
                    for (int e = 0; e < E; ++e)
                        if (e == b_e) {
                            eb[e] = 0xFFFFFFFFu;
                            kk[e] = SCANN_KEY_MAX;
                            sl[e] = 0xFFFFFFFFu;
                        }
                }
                if (tid == 0) {
                    out_store(&a.out_idx[(size_t)q * k + r0], s_idx[b_sl]);
                    out_store(&a.out_dist[(size_t)q * k + r0], ordered_to_f32(b_eb));
                }
            }
        }
    }
    for (uint32_t i = nout + tid; i < k; i += nt) {
        out_store(&a.out_idx[(size_t)q * k + i], kInvalid);
        out_store(&a.out_dist[(size_t)q * k + i], __builtin_inff());
    }
    if (tid == 0) out_store(&a.out_count[q], nout);

    if (a.done) {   // host call polling for completion: the flag after this block's result rows
        // (rows and flag live in pinned host memory and are written with system-scope write-through stores,
        // so waiting for their completion orders them; a system-scope release FENCE would write back the
        // whole L2 -- tens of microseconds)
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
        if (tid == 0) __hip_atomic_store(&a.done[q], a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ __launch_bounds__(kSelectThreads) void small_finish_kernel(TxhIndexDev ix, SmallArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_qf[];   // [dim]
    const uint32_t q = blockIdx.x;
    small_finish_body<false>(ix, a, q, s_qf, a.vbase + (size_t)q * (a.P + 1), a.tokens + (size_t)q * a.P);
}

// =====================================================================================
// Multi-GPU merge of gathered (key, idx, exact) triples [world][nq][m].  Every rank's
// list is sorted by key and keys are unique per query, so an element's position in the
// merged order is the number of smaller keys over all lists (binary searches); no sort
// of world*m keys is needed.  Then the same stable exact sort as above.
// =====================================================================================
__global__ __launch_bounds__(kSelectThreads) void merge_kernel(
    uint32_t world, uint32_t nq, uint32_t m_local, uint32_t m, uint32_t k, uint32_t m2max,
    size_t rank_stride, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ idx,
    const float *__restrict__ exact, const uint32_t *__restrict__ count,
    uint32_t *__restrict__ out_idx, float *__restrict__ out_dist,
    uint32_t *__restrict__ out_count, uint32_t *__restrict__ status, const uint32_t *__restrict__ qoff) {
    // rank g's arrays start rank_stride BYTES after rank g-1's (a packed all_gather buffer);
    // rank_stride == 0 means dense [world][nq][m_local] arrays.  qoff != nullptr: COMPACT lists (comm.hip): the
    // entries of (rank g, query q) start at element qoff[g * nq + q] of rank g's arrays instead of q * m_local.
    extern __shared__ __attribute__((aligned(16))) uint64_t skeys[];   // [m2max] (sort path)
    uint32_t *s_src = reinterpret_cast<uint32_t *>(skeys + m2max);     // [m2max] packed (g, slot)
    uint64_t *s_mth = reinterpret_cast<uint64_t *>(s_src + m2max);     // [1] key at rank nsel-1
    uint64_t *s_red = s_mth + 1;                                       // [kSelectThreads/64]
    const uint32_t q = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    auto at = [&](const void *base, uint32_t g, size_t dense_elems, size_t esz) -> const char * {
        return reinterpret_cast<const char *>(base) +
               (rank_stride ? (size_t)g * rank_stride : (size_t)g * dense_elems * esz);
    };
    auto first = [&](uint32_t g) { return qoff ? (size_t)qoff[(size_t)g * nq + q] : (size_t)q * m_local; };
    auto keys_of = [&](uint32_t g) {
        return reinterpret_cast<const uint64_t *>(at(keys, g, (size_t)nq * m_local, 8)) + first(g);
    };
    auto idx_of = [&](uint32_t g) {
        return reinterpret_cast<const uint32_t *>(at(idx, g, (size_t)nq * m_local, 4)) + first(g);
    };
    auto exact_of = [&](uint32_t g) {
        return reinterpret_cast<const float *>(at(exact, g, (size_t)nq * m_local, 4)) + first(g);
    };
    auto count_of = [&](uint32_t g) {
        return reinterpret_cast<const uint32_t *>(at(count, g, (size_t)nq, 4))[q];
    };
    uint32_t tot = 0;
    for (uint32_t g = 0; g < world; ++g) tot += count_of(g);
    const uint32_t nsel = min(m, tot);
    if (tid == 0) *s_mth = SCANN_KEY_MAX;
    __syncthreads();
    for (uint32_t g = 0; g < world; ++g) {
        const uint32_t cg = count_of(g);
        const uint64_t *kl = keys_of(g);
        for (uint32_t i = tid; i < cg; i += nt) {
            const uint64_t key = kl[i];
            uint32_t rank = i;                      // smaller keys in its own list
            for (uint32_t g2 = 0; g2 < world; ++g2) {
                if (g2 == g) continue;
                const uint64_t *k2 = keys_of(g2);
                uint32_t lo = 0, hi = count_of(g2);
                while (lo < hi) {
                    uint32_t mid = (lo + hi) >> 1;
                    if (k2[mid] < key) lo = mid + 1; else hi = mid;
                }
                rank += lo;
            }
            if (rank < nsel) s_src[rank] = (g << 24) | i;     // world <= 64, m_local <= 8192
            if (rank + 1 == nsel) *s_mth = key;
        }
    }
    __syncthreads();
    // Ranks may send fewer than m candidates (m_local < m, sized for a random shard's share
    // of the global top-m).  A truncated list whose last key is still below the global m-th
    // key could have held more members: report it, the caller re-runs with m_local = m.
    if (status && m_local < m && tid < world) {
        const uint32_t cg = count_of(tid);
        if (cg == m_local && cg > 0) {
            const uint64_t last = keys_of(tid)[cg - 1];
            if (tot < m || last < *s_mth) atomicMax(status, (uint32_t)SCANN_HIP_ABORTED);
        }
    }
    const uint32_t nout = min(k, nsel);
    if (k <= kTopkMaxK) {
        // stable sort by exact == order by (exact, merged approx rank): k block-wide arg-mins
        constexpr int E = kMaxPreReorderK / kSelectThreads;
        uint64_t key2[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const uint32_t r = e * kSelectThreads + tid;
            key2[e] = SCANN_KEY_MAX;
            if (r < nsel) {
                const uint32_t src = s_src[r];
                key2[e] = make_key(exact_of(src >> 24)[src & 0xFFFFFFu], r);
            }
        }
        for (uint32_t r = 0; r < nout; ++r) {
            uint64_t b = key2[0];
#pragma unroll
            for (int e = 1; e < E; ++e) b = min(b, key2[e]);
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) b = min(b, (uint64_t)__shfl_xor((unsigned long long)b, d, 64));
            if ((tid & 63u) == 0) s_red[tid >> 6] = b;
            __syncthreads();
            uint64_t gmin = s_red[0];
#pragma unroll
            for (int w2 = 1; w2 < (int)(kSelectThreads / 64); ++w2) gmin = min(gmin, s_red[w2]);
            const uint32_t rk = (uint32_t)gmin;
            if ((rk & (kSelectThreads - 1)) == tid) {
                const uint32_t we = rk / kSelectThreads;
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if ((uint32_t)e == we) key2[e] = SCANN_KEY_MAX;
                const uint32_t src = s_src[rk];
                out_idx[(size_t)q * k + r] = idx_of(src >> 24)[src & 0xFFFFFFu];
                out_dist[(size_t)q * k + r] = ordered_to_f32((uint32_t)(gmin >> 32));
            }
            __syncthreads();
        }
        for (uint32_t i = nout + tid; i < k; i += nt) {
            out_idx[(size_t)q * k + i] = kInvalid;
            out_dist[(size_t)q * k + i] = __builtin_inff();
        }
        if (tid == 0) out_count[q] = nout;
        return;
    }
    uint32_t m2 = 1;
    while (m2 < nsel) m2 <<= 1;
    for (uint32_t i = tid; i < m2; i += nt) {
        uint64_t kv = SCANN_KEY_MAX;
        if (i < nsel) {
            const uint32_t src = s_src[i];
            kv = make_key(exact_of(src >> 24)[src & 0xFFFFFFu], i);
        }
        skeys[i] = kv;
    }
    __syncthreads();
    bitonic_sort_lds(skeys, m2);
    for (uint32_t i = tid; i < k; i += nt) {
        uint32_t oi = kInvalid;
        float od = __builtin_inff();
        if (i < nout) {
            const uint64_t key = skeys[i];
            const uint32_t src = s_src[(uint32_t)key];
            oi = idx_of(src >> 24)[src & 0xFFFFFFu];
            od = ordered_to_f32((uint32_t)(key >> 32));
        }
        out_idx[(size_t)q * k + i] = oi;
        out_dist[(size_t)q * k + i] = od;
    }
    if (tid == 0) out_count[q] = nout;
}

// =====================================================================================
// launchers
// =====================================================================================
static int launch_partition_stage(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st) {
    if (ix.ah_mode) {
        return launch_ah_tokens(ix, w, st);
    }
    SCANN_TRY(launch_centroid_scores(ix, w, st));
    const uint32_t n2 = next_pow2_u32(ix.L);
    // select path when P is small against L: rank-select the P-th key, sort P keys instead of L
    uint32_t p2 = (w.P * 4u <= n2) ? next_pow2_u32(std::max(1u, w.P)) : 0u;
    const SelCfg lcfg = sel_cfg(ix.L);
    const auto lds_of = [&](uint32_t p_pow2) {
        return (size_t)(n2 + p_pow2) * sizeof(uint64_t) + (size_t)lcfg.bins * 4 + (size_t)lcfg.list * 8 + 48 * 8 + 64 * 4;
    };
    // ... and while its P extra keys fit: above 8192 leaves the 16384 keys and the large tables take 156 288 bytes, and
    // the survivors of more than 512 partitions would pass the CU's 160 KB -- those sort all the keys in place
    // (at 64 KB or below launch() checks nothing either)
    if (p2 && lds_of(p2) > 64 * 1024) {
        size_t static_bytes = 0;
        SCANN_TRY(static_lds_bytes(reinterpret_cast<const void *>(select_leaves_kernel), &static_bytes));
        if (lds_of(p2) + static_bytes > kMaxLdsBytes) p2 = 0;
    }
    const size_t lds2 = lds_of(p2);
    SCANN_TRY(launch(select_leaves_kernel, dim3(w.nq), dim3(p2 && ix.L <= 4096 ? 256u : kSelectThreads), lds2, st,
                     w.cdist, ix.L, n2, w.P, p2, ix.leaf_gsize, ix.leaf_off, w.st, w.tokens, w.token_dists,
                     w.vbase, w.sbase, (const float *)nullptr, (const float *)nullptr, 0u, 0u, 0u));
    return SCANN_HIP_OK;
}

int txh_launch_partition_only(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st) {
    return launch_partition_stage(ix, w, st);
}

static size_t threshold_select_lds(uint32_t scap) {
    const SelCfg tcfg = sel_cfg(scap);
    return ((size_t)((scap + 3u) & ~3u) + tcfg.bins + tcfg.list) * 4 + 48 * 8;
}

// K5a + K5b / K5c: the f32 sample of every query's stream and the filter bound from it
static int launch_gather_bound(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st) {
    if (!w.no_threshold) {
        SCANN_TRY(with_codec(ix, [&](auto codec) -> int {
            using C = decltype(codec);
            SampleArgs sa;
            sa.pair_off = w.pair_off; sa.stile_off = w.stile_off; sa.pair_q = w.pair_q;
            sa.pair_sbase = w.pair_sbase; sa.counters = w.counters; sa.lutq = w.lutq; sa.samp = w.samp;
            sa.scap = w.scap; sa.st = w.st; sa.qpt = w.sqpt; sa.allow = w.allow; sa.allow_bits = w.allow_bits;
            const size_t lds_smp = (size_t)2 * C::LUT4 * 16 + 16;
            if (w.allow && w.allow_stride) {   // one bitmap per query
                sa.allow_bits = pq_allow_bits(w.allow_bits, w.allow_stride);
                return launch(adc_sample_kernel<PqCodec<C>>, dim3((uint32_t)num_cus() * 8u), dim3(kScanThreads), lds_smp, st, ix, sa);
            }
            return launch(adc_sample_kernel<C>, dim3((uint32_t)num_cus() * 8u), dim3(kScanThreads), lds_smp, st, ix, sa);
        }));
    }
    const uint32_t nt = w.scap > 8192 ? kSelectThreads : 256u;
    // (without thr_ties the bound is on the distance alone: whole tie groups pass)
    if (w.thr_tail) {
        SCANN_TRY(launch(threshold_tail_kernel, dim3(w.nq), dim3(kThrTailThreads), 0, st, w.P, w.m, w.st, w.sbase,
                         w.samp, w.scap, w.slot_of, w.thr, w.pair_thr, w.thr_ties ? w.vbase : nullptr));
    } else {
        SCANN_TRY(launch(threshold_select_kernel, dim3(w.nq), dim3(nt), threshold_select_lds(w.scap), st, w.P, w.m, w.st,
                         (int)w.no_threshold, w.sbase, w.samp, w.scap, w.slot_of, w.thr, w.pair_thr,
                         w.thr_ties ? w.vbase : nullptr));
    }
    return SCANN_HIP_OK;
}

// thr = MAX for every query: select_rerank takes the k smallest of the whole stream
static int launch_open_bound(const TxhWork &w, hipStream_t st) {
    SCANN_TRY(launch(threshold_select_kernel, dim3(w.nq), dim3(256), threshold_select_lds(w.scap), st, w.P, w.m, w.st, 1,
                     w.sbase, w.samp, w.scap, w.slot_of, w.thr, w.pair_thr, w.vbase));
    return SCANN_HIP_OK;
}

// K6 / K6b: the f32 gather scan or its resident-table form
static int launch_gather_scan(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
    return with_codec(ix, [&](auto codec) -> int {
        using C = decltype(codec);
        const int cus = num_cus();
        ScanArgs a;
        a.pair_off = w.pair_off; a.tile_off = w.tile_off; a.pair_q = w.pair_q;
        a.pair_vbase = w.pair_vbase; a.counters = w.counters; a.lutq = w.lutq; a.pair_thr = w.pair_thr;
        a.cand_cnt = w.cand_cnt; a.cand = w.cand; a.cap = w.cap; a.qpt = w.qpt; a.allow = w.allow; a.allow_bits = w.allow_bits;
        if (ev0) SCANN_HIP_CHECK(hipEventRecord(ev0, st));
        const uint32_t wgs = (uint32_t)cus * 8u;
        a.res_cl = w.res_cl;
        const bool pq = w.allow && w.allow_stride;   // one bitmap per query: the _pq instantiations
        if constexpr (C::BITS == 4 && C::S <= 32) {
            if (w.scan == TxhScan::Resident) {
                if (pq) {
                    ScanArgs ap = a;
                    ap.allow_bits = pq_allow_bits(w.allow_bits, w.allow_stride);
                    SCANN_TRY(launch(adc_scan_res_kernel<PqCodec<C>>, dim3((uint32_t)cus * 4u), dim3(kResThreads),
                                     res_lds_bytes<C>(), st, ix, ap));
                } else {
                    SCANN_TRY(launch(adc_scan_res_kernel<C>, dim3((uint32_t)cus * 4u), dim3(kResThreads),
                                     res_lds_bytes<C>(), st, ix, a));
                }
                if (ev1) SCANN_HIP_CHECK(hipEventRecord(ev1, st));
                return SCANN_HIP_OK;
            }
        }
        if (pq)
            SCANN_TRY(launch(adc_scan_pq_kernel<C>, dim3(wgs), dim3(kScanThreads), scan_lds_bytes<C>(), st, ix, a, w.allow_stride));
        else
            SCANN_TRY(launch(adc_scan_kernel<C>, dim3(wgs), dim3(kScanThreads), scan_lds_bytes<C>(), st, ix, a));
        if (ev1) SCANN_HIP_CHECK(hipEventRecord(ev1, st));
        return SCANN_HIP_OK;
    });
}

// K5d + K5e: flat hasher in front of an MFMA prefilter: plain tables, integer sample, tail bound
static int launch_sample_mfma_bound(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st) {
    return with_codec(ix, [&](auto codec) -> int {
        using C = decltype(codec);
        if constexpr (C::BITS == 4) {
            Lut8Meta *meta = reinterpret_cast<Lut8Meta *>(w.lut8_meta);
            SCANN_TRY(launch_lut8_build(w, (uint32_t)C::S, -1, st));
            SampleMfmaArgs sm;
            sm.pair_off = w.pair_off; sm.pair_q = w.pair_q; sm.pair_sbase = w.pair_sbase; sm.lut8 = w.lut8;
            sm.samp16 = reinterpret_cast<uint16_t *>(w.samp); sm.scap = w.scap; sm.st = w.st;
            sm.allow = w.allow; sm.allow_bits = w.allow_bits;
            if (w.allow && w.allow_stride)   // one bitmap per query
                SCANN_TRY(launch(adc_sample_mfma_pq_kernel<C::S>, dim3((uint32_t)num_cus() * 4u), dim3(256), 0, st, ix, sm,
                                 w.allow_stride));
            else
                SCANN_TRY(launch(adc_sample_mfma_kernel<C::S>, dim3((uint32_t)num_cus() * 4u), dim3(256), 0, st, ix, sm));
            Tail16Args ta;
            ta.P = w.P; ta.m = w.m; ta.st = w.st; ta.scap = w.scap; ta.sbase = w.sbase; ta.slot_of = w.slot_of;
            ta.tokens = w.tokens; ta.vbase = w.vbase; ta.samp16 = sm.samp16; ta.lutq = w.lutq; ta.meta = meta;
            ta.thr = w.thr; ta.pair_thr = w.pair_thr;
            SCANN_TRY(launch(threshold_tail16_kernel<C::S>, dim3(w.nq), dim3(kThrTailThreads), 0, st, ix, ta));
        }
        return SCANN_HIP_OK;
    });
}

static size_t exact_scan_lds_bytes(uint32_t dim) {
    return (size_t)exact_quads_per_tile(dim) * 4 * ((dim + 3u) & ~3u) * sizeof(float);
}

// set_dyn_lds' own decision for launch_exact_scan: the dynamic request plus the kernel's static arrays, asked of the
// code object (a failed query counts as "does not fit": the batched launch then reports it)
bool txh_exact_scan_fits(const TxhIndexDev &ix) {
    size_t static_bytes = 0;
    const int s = with_measure(ix.measure, [&](auto m) {
        return static_lds_bytes(reinterpret_cast<const void *>(leaf_exact_scan_kernel<m()>), &static_bytes);
    });
    return s == SCANN_HIP_OK && exact_scan_lds_bytes(ix.dim) + static_bytes <= kMaxLdsBytes;
}

// SearchMode::Partitioned: dense key lists (no threshold), one exact-distance tile kernel.
static int launch_exact_scan(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st, hipEvent_t ev0,
                             hipEvent_t ev1) {
    const int cus = num_cus();
    SCANN_TRY(launch_open_bound(w, st));
    SCANN_TRY(launch(stream_counts_kernel, dim3(ceil_div_u32(w.nq, 256)), dim3(256), 0, st, w.nq, w.P, w.vbase,
                     w.cand_cnt));
    ExactScanArgs a;
    a.pair_off = w.pair_off; a.tile_off = w.tile_off; a.pair_q = w.pair_q; a.pair_vbase = w.pair_vbase;
    a.counters = w.counters; a.queries = w.queries; a.q_stride = w.q_stride; a.cand = w.cand; a.cap = w.cap;
    a.qpt = exact_quads_per_tile(ix.dim);
    const size_t lds = exact_scan_lds_bytes(ix.dim);
    if (ev0) SCANN_HIP_CHECK(hipEventRecord(ev0, st));
    const dim3 grid((uint32_t)cus * 8u), block(256);
    SCANN_TRY(with_measure(ix.measure, [&](auto m) {
        return launch(leaf_exact_scan_kernel<m()>, grid, block, lds, st, ix, a);
    }));
    if (ev1) SCANN_HIP_CHECK(hipEventRecord(ev1, st));
    return SCANN_HIP_OK;
}

// the candidates may leave the select in any order: the final stage orders them by 96-bit keys (K9b)
static bool select_unsorted(const TxhWork &w, bool local_only) {
    return w.exact_reorder && !local_only && !w.need_sorted_cands && w.k <= kTopkMaxK;
}

static int launch_select(const TxhIndexDev &ix, const TxhWork &w, bool local_only, hipStream_t st) {
    SelectArgs s;
    s.P = w.P; s.m = w.m; s.k = w.k; s.cap = w.cap;
    s.exact_reorder = w.exact_reorder; s.local_only = local_only ? 1 : 0;
    const bool unsorted = select_unsorted(w, local_only);
    s.unsorted = unsorted ? 1 : 0;
    s.queries = w.queries; s.q_stride = w.q_stride; s.tokens = w.tokens; s.vbase = w.vbase;
    s.thr = w.thr; s.cand_row = w.cand_row;
    s.cand_cnt = w.cand_cnt; s.cand = w.cand; s.counters = w.counters; s.cand_key = w.cand_key;
    s.cand_idx = w.cand_idx; s.cand_dist = w.cand_dist; s.cand_exact = w.cand_exact;
    s.cand_count = w.cand_count; s.out_idx = w.out_idx; s.out_dist = w.out_dist;
    s.out_count = w.out_count;
    // LDS key array: the candidate capacity rounded up to a power of two (bitonic path), at
    // most kSortCap; small lists run with 256-thread blocks so several fit a CU
    // (sorted path: room for the m keys that are kept -- a longer list is rank-selected straight from global
    // memory first, so the bitonic sort runs over pow2(m) keys, not pow2(capacity): half the stages' work at
    // capacity ~1.4 m)
    uint32_t lds_keys = std::min(kSortCap, next_pow2_u32(std::max(unsorted ? w.cap : std::min(w.cap, w.m), 64u)));
    // unsorted selection of a long list: straight from the global list, 512-thread workgroups with ~30 KB of
    // LDS (without select_direct: stage the keys as before)
    const bool direct = unsorted && w.select_direct && lds_keys > 4096u;
    s.direct = direct ? 1u : 0u;
    s.sel_n = w.cap;
    if (direct && w.select_regs) {
        // the list in registers (K7r): the instantiations cover plan_txh_search's capacities, (J + 8 sqrt(J) + 16) st
        // + 256 -- 12 770 at 1M points and m = 5000, ~17 500 at m = 8192; a longer list takes the kernel below
        void (*regs)(TxhIndexDev, SelectArgs) =
            w.cap <= kSelRegCaps[0]   ? select_regs_kernel<kSelRegCaps[0] / kSelRegThreads>
            : w.cap <= kSelRegCaps[1] ? select_regs_kernel<kSelRegCaps[1] / kSelRegThreads>
            : w.cap <= kSelRegCaps[2] ? select_regs_kernel<kSelRegCaps[2] / kSelRegThreads>
                                      : nullptr;
        if (regs) {
            s.lds_keys = 0;
            SCANN_TRY(launch(regs, dim3(w.nq), dim3(kSelRegThreads), 0, st, ix, s));
            return SCANN_HIP_OK;
        }
    }
    if (direct) lds_keys = 64;
    s.lds_keys = lds_keys;
    const SelCfg scfg = sel_cfg(direct ? w.cap : lds_keys);
    const size_t lds_sel = (size_t)lds_keys * 8 + (size_t)(kSelectThreads / 64 + 4) * 4 +
                           (size_t)scfg.bins * 4 + (size_t)scfg.list * 8 + 48 * 8 + 2 * kDecodeStage * 4;
    const uint32_t sel_threads = direct ? 512u : (lds_keys <= 4096 ? 256u : kSelectThreads);
    SCANN_TRY(launch(select_rerank_kernel, dim3(w.nq), dim3(sel_threads), lds_sel, st, ix, s));
    return SCANN_HIP_OK;
}

static int launch_rerank(const TxhIndexDev &ix, const TxhWork &w, bool local_only, hipStream_t st) {
    // rows stored quantized: every candidate scored from its stored row (txh_rows.hip K8q); the final kernels finish
    if (ix.qfmt) return launch_rerank_quant(ix, w, st);
    const bool unsorted = select_unsorted(w, local_only);
    // The re-rank's own view of the index: the rows' dimensionality and stride, and the queries of that space.  The same
    // as ix / w.queries on every handle but a projected one (txh.h: row_dim, rr_queries), which has no 8-bit store.
    TxhIndexDev rx = ix;
    if (ix.row_dim) {
        rx.dim = ix.row_dim;
        rx.stride = ix.row_stride;
    }
    const float *rr_q = w.rr_queries ? w.rr_queries : w.queries;
    const uint32_t rr_qs = w.rr_queries ? w.rr_q_stride : w.q_stride;
    const size_t lds_rr = (size_t)rx.dim * 4;
    // int8 row filter in front of the exact re-rank (K8b): single-GPU final stage, squared L2, lists long
    // enough for the two extra kernels to pay
    // (the local stage of a leaf-sharded search takes the same two kernels in their prefix form: ShortArgs::local_head;
    // without local_prune: every local candidate re-ranked exactly, as before)
    const bool i8_local = local_only && w.local_prune && w.exact_reorder && !w.need_sorted_cands && w.k <= kTopkMaxK &&
                          w.m > 2 * kLocalHead;
    const bool i8 = (unsorted || i8_local) && w.use_i8 && ix.rows8 && ix.measure == SCANN_HIP_SQUARED_L2 && (ix.dim & 15u) == 0 &&
                    !w.rr_queries;
    if (i8) {
        SCANN_TRY(launch_rerank_i8(ix, w, st));
        ShortArgs sa;
        sa.m = w.m; sa.k = w.k; sa.queries = w.queries; sa.q_stride = w.q_stride; sa.lb = w.rr_lb; sa.ub = w.rr_ub;
        sa.cand_row = w.cand_row; sa.cand_idx = w.cand_idx; sa.cand_key = w.cand_key; sa.cand_count = w.cand_count;
        sa.cand_exact = w.cand_exact; sa.out_idx = w.out_idx; sa.out_dist = w.out_dist; sa.out_count = w.out_count;
        sa.local_head = local_only ? kLocalHead : 0u;
        const size_t lds_sh = (size_t)ix.dim * 4;
        SCANN_TRY(launch(rerank_short_kernel, dim3(w.nq), dim3(256), lds_sh, st, ix, sa));
    } else {
        SCANN_TRY(launch(rerank_kernel, dim3(ceil_div_u32(w.m, 32), w.nq), dim3(256), lds_rr, st, rx,
                         rr_q, rr_qs, w.m, w.cand_row, w.cand_count, w.cand_exact));
    }
    return SCANN_HIP_OK;
}

static int launch_final(const TxhWork &w, hipStream_t st) {
    if (select_unsorted(w, false)) {
        return with_value<256, 1024>(w.m <= 2048 ? 256 : 1024, [&](auto nt) {
            return launch(final_topk_kernel<nt()>, dim3(w.nq), dim3(nt()), 0, st, w.m, w.k, w.cand_count, w.cand_idx,
                          w.cand_key, w.cand_exact, w.out_idx, w.out_dist, w.out_count);
        });
    }
    const size_t lds_fs = (size_t)next_pow2_u32(std::max(1u, w.m)) * 8;
    SCANN_TRY(launch(final_sort_kernel, dim3(w.nq), dim3(kSelectThreads), lds_fs, st, w.m, w.k,
                     w.cand_count, w.cand_idx, w.cand_exact, w.out_idx, w.out_dist, w.out_count));
    return SCANN_HIP_OK;
}

// ---- the small-batch pipeline as ONE launch ----------------------------------------------------------
// A kernel that follows another in a stream starts ~8-10 us after it (dispatch latency), which for a handful
// of queries is most of the job.  Here every workgroup (query q, 1024 stream positions) first repeats the
// query's leaf selection (select_leaves_body: the tables come from L2, the repetition costs no time), then
// scores its positions into the dense key list, and the LAST workgroup of the query to finish (a ticket
// counter behind a __threadfence) runs the finish stage.  No workgroup ever waits for another.

// Wide pipeline: stream positions per group minimum for a stream of cnt keys and m wanted candidates: the smallest
// power of two that leaves at most kWideGroups groups (wide_filter_kernel holds them in registers, 16 per thread) --
// the pivot, the m-th smallest group minimum, lets about -G ln(1 - m / G) keys pass when the candidates are spread
// evenly over G groups (1.2 m at G = 3 m), more when they sit in a few leaves -- but never fewer than 1.5 m groups.
// Chosen on the device from the query's OWN stream: leaves differ in size by an order of magnitude and the host only
// knows the longest stream.
constexpr uint32_t kWideGroups = 16384;
__host__ __device__ static inline uint32_t wide_group(uint32_t cnt, uint32_t m) {
    uint32_t g = 1;
    while (g < 64 && (cnt + g - 1) / g > kWideGroups) g <<= 1;
    while (g > 1 && (uint64_t)cnt / g < ((uint64_t)m * 3) / 2) g >>= 1;
    return g;
}

struct FusedArgs {
    uint32_t L, n_pow2, p_pow2, st;
    float *cdist, *token_dists;
    uint32_t *tokens, *vbase, *sbase;   // (written by workgroup 0 of each query)
    uint32_t *tickets;                  // [nq], zero between launches
};

__global__ __launch_bounds__(kSelectThreads) void small_fused_kernel(TxhIndexDev ix, SmallArgs a, FusedArgs f) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];   // selection | scan tables | query
    __shared__ uint32_t s_tok[kDecodeStage], s_vb[kDecodeStage + 1], s_lrow[kDecodeStage], s_last;
    const uint32_t q = blockIdx.y, b = blockIdx.x, tid = threadIdx.x, nt = kSelectThreads;
    const uint32_t P = a.P, dim = ix.dim;
    if (q == 0 && b == 0 && tid == 0) a.counters[CNT_STATUS] = 0;
    // ---- stage 1: the P nearest leaves and their key bases (every workgroup of the query)
    if (ix.ah_mode) {
        if (tid == 0) {
            s_tok[0] = 0;
            s_vb[0] = 0;
            s_vb[1] = ix.leaf_gsize[0];
            if (b == 0) {   // (ah_tokens_kernel)
                const uint32_t sz = ix.leaf_off[1] - ix.leaf_off[0];
                f.tokens[q] = 0;
                f.token_dists[q] = 0.0f;
                f.vbase[2 * q] = 0;
                f.vbase[2 * q + 1] = ix.leaf_gsize[0];
                f.sbase[3 * q] = 0;
                f.sbase[3 * q + 1] = (sz + f.st - 1) / f.st;
                f.sbase[3 * q + 2] = sz;
            }
        }
    } else {
        select_leaves_body(reinterpret_cast<uint64_t *>(s_dyn), q, b == 0, s_tok, s_vb, f.cdist, f.L, f.n_pow2, P,
                           f.p_pow2, ix.leaf_gsize, ix.leaf_off, f.st, f.tokens, f.token_dists, f.vbase, f.sbase,
                           ix.centers_t, a.queries, a.q_stride, dim, ix.centers_pitch);
    }
    __syncthreads();
    for (uint32_t r = tid; r < P; r += nt) s_lrow[r] = ix.leaf_off[s_tok[r]];
    const uint32_t cnt = min(s_vb[P], a.cap);
    const uint32_t chunk = a.chunk;   // stream positions per workgroup (<= the workgroup's threads)
    const uint32_t v0 = b * chunk;
    if (v0 >= cnt && b != 0) return;   // an idle workgroup (block-uniform; workgroup 0 always takes part)
    __syncthreads();
    // ---- stage 2: keys of the stream positions [v0, v0 + kFusedChunk)
    const uint32_t v = v0 + tid;
    const bool have = tid < chunk && v < cnt;
    uint32_t r = 0;
    if (have) {
        uint32_t lo = 0, hi = P;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_vb[mid] <= v) lo = mid; else hi = mid;
        }
        r = lo;
    }
    const uint32_t j = have ? v - s_vb[r] : 0u;
    const uint32_t csr = have ? s_lrow[r] + j : 0u;
    uint64_t *out = a.cand + (size_t)q * a.cap;
    if (ix.exact_scan) {
        float *s_qe = reinterpret_cast<float *>(s_dyn);
        for (uint32_t d = tid; d < dim; d += nt) s_qe[d] = a.queries[(size_t)q * a.q_stride + d];
        __syncthreads();
        if (have) {
            const float *row = ix.rows + (size_t)(ix.rows_csr ? csr : ix.leaf_ids[csr]) * ix.stride;
            const uint64_t key =
                row_allowed(ix, a.allow, a.allow_stride, q, a.allow_bits, csr) ? make_key(exact_pair_thread(ix.measure, dim, s_qe, row), v) : SCANN_KEY_MAX;
            __hip_atomic_store(&out[v], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else if (cnt) {
        const uint32_t S = ix.S, K = ix.K, dsub = ix.dsub, kp = ix.kp;
        float *s_lut = reinterpret_cast<float *>(s_dyn), *s_qr = s_lut + S * kp;
        // the leaves this workgroup's positions fall into (uniform: from the first and last position)
        uint32_t r_first = 0, r_last = 0;
        {
            const uint32_t va = v0, vz = min(v0 + chunk, cnt) - 1u;
            uint32_t lo = 0, hi = P;
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (s_vb[mid] <= va) lo = mid; else hi = mid;
            }
            r_first = lo;
            lo = 0; hi = P;
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (s_vb[mid] <= vz) lo = mid; else hi = mid;
            }
            r_last = lo;
        }
        const uint32_t bits = ix.code_bits, per = 32u / bits, mask = (1u << bits) - 1u, nw = ix.nw;
        for (uint32_t rr = r_first; rr <= r_last; ++rr) {
            if (s_vb[rr + 1] == s_vb[rr]) continue;   // an empty leaf (uniform)
            const uint32_t leaf = s_tok[rr];
            for (uint32_t d = tid; d < dim; d += nt) {   // residual q - centroid (mod.rs:309-316)
                float x = a.queries[(size_t)q * a.q_stride + d];
                if (ix.use_residuals) x = x - ix.centers[(size_t)leaf * dim + d];
                s_qr[d] = x;
            }
            __syncthreads();
            for (uint32_t e = tid; e < S * kp; e += nt) {   // LookupTable::from_query (lut.rs:47-70, codebook.rs:98-115)
                const uint32_t sub = e / kp, c = e - sub * kp;
                float acc = 0.0f;
                if (c < K) {
                    const float *cb = ix.codebook + ((size_t)sub * K + c) * dsub;
                    for (uint32_t d = 0; d < dsub; ++d) {
                        const float t = s_qr[sub * dsub + d] - cb[d];
                        acc = acc + t * t;
                    }
                }
                s_lut[e] = acc;
            }
            __syncthreads();
            if (have && r == rr) {
                const uint32_t *w = ix.codes + (size_t)csr * nw;
                float acc = 0.0f;   // LookupTable::compute_distance (lut.rs:74-82)
                for (uint32_t sub = 0; sub < S; ++sub) {
                    const uint32_t code = (w[sub / per] >> (bits * (sub % per))) & mask;
                    const float tv = s_lut[sub * kp + code];
                    acc = sub == 0 ? tv : acc + tv;
                }
                __hip_atomic_store(&out[v], row_allowed(ix, a.allow, a.allow_stride, q, a.allow_bits, csr) ? make_key(acc, v) : SCANN_KEY_MAX,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __syncthreads();   // (the tables are rebuilt for the next leaf)
        }
    }
    // ---- stage 3: the last workgroup of the query to get here finishes it.  The keys were stored with
    // agent scope (write-through: the XCDs' L2s are not coherent with each other inside a kernel, and an
    // agent-scope FENCE would write back the whole L2 -- tens of microseconds); every thread waits for its own
    // store, the barrier orders the workgroup, the ticket is an agent-scope atomic, and the finish stage reads
    // the list with agent-scope loads ONLY (block_select<.., AGENT> included).  This is not a release / acquire pair
    // of the memory model but the hand-off MI355X_MICROARCH.md lists as valid on gfx950 in its place ("Valid forms":
    // every byte stored sc1, every storing wave drained with s_waitcnt vmcnt(0) ahead of the barrier, ONE lane of
    // each storing workgroup adding to ONE unsharded agent-scope counter, the workgroup whose add returned last reading
    // with sc1 loads behind a workgroup barrier; 8-byte stores and loads): a hardware property, measured, not an
    // architectural guarantee -- test_small_batch_pipeline_matches_staged_pipeline runs it for every searcher kind,
    // with a restrictive allow-bitmap (the fallback select) and under uneven load.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (inline asm: the compiler may drop a builtin wait it thinks is covered)
    __syncthreads();
    if (tid == 0) {
        const uint32_t target = max(1u, (cnt + chunk - 1u) / chunk);
        const uint32_t t = __hip_atomic_fetch_add(&f.tickets[q], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (t + 1u == target) ? 1u : 0u;
        if (s_last) __hip_atomic_store(&f.tickets[q], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
    }
    __syncthreads();
    if (!s_last) return;
    small_finish_body<true>(ix, a, q, reinterpret_cast<float *>(s_dyn), s_vb, s_tok);
}

// =====================================================================================
// Few queries, long streams: the wide pipeline (TxhWork::small == 2).
//
// The small-batch pipeline above finishes a query in ONE workgroup: two passes over the dense key list, then m
// row gathers -- 0.1 ms for 100 k keys and m = 1000, and pre_reorder_k is capped by the workgroup's LDS.  One
// query over the flat 1M hasher at m = 5000 (the reference's ann_benchmark operating point,
// bin/ann_benchmark.rs:172-178) fell back to the batched pipeline's twelve launches.  Here every stage is
// spread over the chip, in three launches:
//   1. wide_scan_kernel: leaf selection + scan as in small_fused_kernel; every group of g stream positions
//      (wide_group: from the query's own stream length) also leaves its minimum approximate distance.
//   2. wide_filter_kernel: up to 256 workgroups per query.  Each derives the same pivot -- an upper bound of the
//      m-th smallest group minimum (the upper edge of its bin in a 4096-bin histogram of the minima), which is
//      >= the m-th smallest key's distance (the m smallest minima belong to m distinct points) and lets
//      1.2-1.6 m keys pass -- filters its share of the key list (64-key chunks interleaved between the workgroups),
//      decodes the passing keys, scores their rows exactly (exact_pair_8lanes) and appends (key, exact, index) to
//      the query's compact arrays (one global atomic per batch of candidates).
//   3. wide_final_kernel: a workgroup per query, the entries in registers: the m-th smallest key among them (the
//      candidates of mod.rs:283-293: everything above it drops out), then the k best of those by (exact, merge
//      key) (mod.rs:342-364): a histogram shortlist ranked by one wave, or the two-level tournament of
//      small_finish_body when ties crowd the shortlist -- exact under any number of ties.
// Measured (one query, MI355X): flat 1M x 128 hasher at m = 5000: 16 + 16 + 16 us of kernels, 0.061 ms per call
// (the batched pipeline's twelve launches: 0.175); Tree-X-Hybrid 1M x 128, 1000 leaves, P = 10, m = 1000: 35 (of
// which the leaf selection 27) + 12 + 16 us, 0.074 ms per call (three-launch small pipeline: 0.124).
// Same keys, same arithmetic, same tie order as the other pipelines: rows are identical.  If the compact arrays
// overflow (thousands of points tied at the pivot's distance: a dataset of few distinct code rows) the status word
// says RESOURCE_EXHAUSTED and a host call's count row 0xFFFFFFFF; the host entry repeats the call on the batched
// pipeline.
// =====================================================================================
constexpr uint32_t kWideList = 2048;        // passing keys a workgroup of the filter collects per batch

struct WideArgs {
    uint32_t ng_stride, cap2, wgs;
    const uint32_t *mins;
    uint64_t *ckey;
    uint32_t *ceb, *cidx, *ccnt;
};

// Launch 1: leaf selection (every workgroup repeats it, as in small_fused_kernel) and the scan of
// [v0, v0 + chunk) stream positions per workgroup -- for ADC scans up to kWideRep positions per thread, so that a
// workgroup's table build (and its four dependent round trips) is shared by 4096 points and one wave of workgroups
// covers a 1M stream -- plus the group minima.

__global__ __launch_bounds__(kSelectThreads) void wide_scan_kernel(TxhIndexDev ix, SmallArgs a, FusedArgs f, WideArgs wa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];   // selection | scan tables | query
    __shared__ uint32_t s_tok[kDecodeStage], s_vb[kDecodeStage + 1], s_lrow[kDecodeStage];
    const uint32_t q = blockIdx.y, b = blockIdx.x, tid = threadIdx.x, nt = kSelectThreads;
    const uint32_t P = a.P, dim = ix.dim;
#ifdef SCANN_WIDE_TIMING
    uint64_t ts[6];
    ts[0] = wall_clock64();
#endif
    if (q == 0 && b == 0 && tid == 0) a.counters[CNT_STATUS] = 0;
    if (b == 0 && tid == 0) wa.ccnt[q] = 0;
    if (ix.ah_mode) {
        if (tid == 0) {
            s_tok[0] = 0;
            s_vb[0] = 0;
            s_vb[1] = ix.leaf_gsize[0];
            if (b == 0) {   // (ah_tokens_kernel)
                const uint32_t sz = ix.leaf_off[1] - ix.leaf_off[0];
                f.tokens[q] = 0;
                f.token_dists[q] = 0.0f;
                f.vbase[2 * q] = 0;
                f.vbase[2 * q + 1] = ix.leaf_gsize[0];
                f.sbase[3 * q] = 0;
                f.sbase[3 * q + 1] = (sz + f.st - 1) / f.st;
                f.sbase[3 * q + 2] = sz;
            }
        }
    } else {
        select_leaves_body(reinterpret_cast<uint64_t *>(s_dyn), q, b == 0, s_tok, s_vb, f.cdist, f.L, f.n_pow2, P,
                           f.p_pow2, ix.leaf_gsize, ix.leaf_off, f.st, f.tokens, f.token_dists, f.vbase, f.sbase,
                           ix.centers_t, a.queries, a.q_stride, dim, ix.centers_pitch);
    }
    __syncthreads();
    for (uint32_t r = tid; r < P; r += nt) s_lrow[r] = ix.leaf_off[s_tok[r]];
    const uint32_t cnt = min(s_vb[P], a.cap);
    const uint32_t chunk = a.chunk;   // stream positions per workgroup: nt * rep
    const uint32_t v0 = b * chunk;
    if (v0 >= cnt) return;            // an idle workgroup (block-uniform)
    __syncthreads();
#ifdef SCANN_WIDE_TIMING
    ts[1] = wall_clock64();
#endif
    const uint32_t g = wide_group(cnt, a.m);
    uint32_t *mins = const_cast<uint32_t *>(wa.mins) + (size_t)q * wa.ng_stride;
    uint64_t *out = a.cand + (size_t)q * a.cap;
    auto leaf_of = [&](uint32_t v) {
        uint32_t lo = 0, hi = P;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_vb[mid] <= v) lo = mid; else hi = mid;
        }
        return lo;
    };
    // minimum of every group of g positions (a group lies inside one wave) -> mins[v / g]
    auto group_min = [&](uint32_t d32, uint32_t v, bool slot) {
        for (uint32_t o = 1; o < g; o <<= 1) {
            const uint32_t other = (uint32_t)__shfl_xor((int)d32, (int)o);
            d32 = other < d32 ? other : d32;
        }
        if (slot && (tid & (g - 1u)) == 0 && v < cnt) mins[v / g] = d32;
    };
    const uint32_t S = ix.S, K = ix.K, dsub = ix.dsub, kp = ix.kp;
    float *s_lut = reinterpret_cast<float *>(s_dyn), *s_qr = s_lut + S * kp;
    const uint32_t vz = min(v0 + chunk, cnt);                      // end of this workgroup's positions
    const uint32_t r_first = leaf_of(v0), r_last = leaf_of(vz - 1u);
    const uint32_t bits = ix.code_bits, per = 32u / bits, mask = (1u << bits) - 1u, nw = ix.nw;
    const bool fast4 = bits == 4 && nw <= 4 && S == nw * 8u;       // whole words of eight 4-bit codes
    uint32_t d32[kWideRep];
#pragma unroll
    for (int it = 0; it < kWideRep; ++it) d32[it] = 0xFFFFFFFFu;   // (no position / rejected by the restrict filter: absent)
    for (uint32_t rr = r_first; rr <= r_last; ++rr) {
        if (s_vb[rr + 1] == s_vb[rr]) continue;   // an empty leaf (uniform)
        const uint32_t leaf = s_tok[rr];
        for (uint32_t d = tid; d < dim; d += nt) {   // residual q - centroid (mod.rs:309-316)
            float x = a.queries[(size_t)q * a.q_stride + d];
            if (ix.use_residuals) x = x - ix.centers[(size_t)leaf * dim + d];
            s_qr[d] = x;
        }
        // this leaf's share of the positions: their code words travel while the tables are built
        const uint32_t la = max(v0, s_vb[rr]), lz = min(vz, s_vb[rr + 1]);
        uint32_t cw[kWideRep][4];
        bool in[kWideRep];
#pragma unroll
        for (int it = 0; it < kWideRep; ++it) {
            const uint32_t v = v0 + (uint32_t)it * nt + tid;
            in[it] = v >= la && v < lz;
#pragma unroll
            for (int wi = 0; wi < 4; ++wi) cw[it][wi] = 0;
            if (fast4 && in[it]) {
                const uint32_t *w = ix.codes + (size_t)(s_lrow[rr] + (v - s_vb[rr])) * nw;
#pragma unroll
                for (int wi = 0; wi < 4; ++wi)
                    if ((uint32_t)wi < nw) cw[it][wi] = w[wi];
            }
        }
        __syncthreads();
        for (uint32_t e = tid; e < S * kp; e += nt) {   // LookupTable::from_query (lut.rs:47-70, codebook.rs:98-115)
            const uint32_t sub = e / kp, c = e - sub * kp;
            float acc = 0.0f;
            if (c < K) {
                const float *cb = ix.codebook + ((size_t)sub * K + c) * dsub;
                for (uint32_t d = 0; d < dsub; ++d) {
                    const float t = s_qr[sub * dsub + d] - cb[d];
                    acc = acc + t * t;
                }
            }
            s_lut[e] = acc;
        }
        __syncthreads();
#ifdef SCANN_WIDE_TIMING
        ts[2] = wall_clock64();
#endif
#pragma unroll
        for (int it = 0; it < kWideRep; ++it) {
            if (!in[it]) continue;
            const uint32_t v = v0 + (uint32_t)it * nt + tid;
            const uint32_t csr = s_lrow[rr] + (v - s_vb[rr]);
            float acc = 0.0f;   // LookupTable::compute_distance (lut.rs:74-82): 0.0 + lut[0][c0] + lut[1][c1] ...
            if (fast4) {
#pragma unroll
                for (int wi = 0; wi < 4; ++wi) {
                    if ((uint32_t)wi >= nw) break;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float tv = s_lut[((uint32_t)wi * 8u + (uint32_t)j) * kp + ((cw[it][wi] >> (4 * j)) & 15u)];
                        acc = (wi == 0 && j == 0) ? tv : acc + tv;
                    }
                }
            } else {
                const uint32_t *w = ix.codes + (size_t)csr * nw;
                for (uint32_t sub = 0; sub < S; ++sub) {
                    const uint32_t code = (w[sub / per] >> (bits * (sub % per))) & mask;
                    const float tv = s_lut[sub * kp + code];
                    acc = sub == 0 ? tv : acc + tv;
                }
            }
            const uint64_t key = row_allowed(ix, a.allow, a.allow_stride, q, a.allow_bits, csr) ? make_key(acc, v) : SCANN_KEY_MAX;
            out[v] = key;
            d32[it] = (uint32_t)(key >> 32);
        }
        __syncthreads();   // (the tables are rebuilt for the next leaf)
    }
#ifdef SCANN_WIDE_TIMING
    ts[3] = wall_clock64();
#endif
#pragma unroll
    for (int it = 0; it < kWideRep; ++it) {
        if ((uint32_t)it * nt >= chunk) break;   // (uniform)
        group_min(d32[it], v0 + (uint32_t)it * nt + tid, true);
    }
#ifdef SCANN_WIDE_TIMING
    ts[4] = wall_clock64();
    if (tid == 0 && b == 0) printf("scan: leaves %.2f tables %.2f points %.2f minima %.2f us\n", (ts[1] - ts[0]) * 0.01, (ts[2] - ts[1]) * 0.01, (ts[3] - ts[2]) * 0.01, (ts[4] - ts[3]) * 0.01);
#endif
}

__global__ __launch_bounds__(kSelectThreads) void wide_filter_kernel(TxhIndexDev ix, SmallArgs a, WideArgs wa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_wdyn[];   // [dim] query
    __shared__ uint64_t s_pass[kWideList], s_slist[kSelListMax], s_red[48];
    __shared__ uint32_t s_hist[kSelBinsMax], s_eb[kWideList], s_ix[kWideList], s_dvb[kDecodeStage + 1], s_drow[kDecodeStage];
    __shared__ uint32_t s_n, s_base;
    const uint32_t q = blockIdx.y, b = blockIdx.x, tid = threadIdx.x, nt = kSelectThreads;
    const uint32_t P = a.P, m = a.m;
    const uint32_t *vbq = a.vbase + (size_t)q * (P + 1), *tokq = a.tokens + (size_t)q * P;
#ifdef SCANN_WIDE_TIMING
    uint64_t tf[6];
    tf[0] = wall_clock64();
#endif
    const uint32_t cnt = min(vbq[P], a.cap);
    if ((uint64_t)b * 64u >= cnt) return;   // no key chunk for this workgroup (block-uniform)
    float *s_q = reinterpret_cast<float *>(s_wdyn);
    for (uint32_t j = tid; j < ix.dim; j += nt) s_q[j] = a.queries[(size_t)q * a.q_stride + j];
    for (uint32_t r = tid; r <= P; r += nt) {
        s_dvb[r] = vbq[r];
        if (r < P) s_drow[r] = ix.leaf_off[tokq[r]];
    }
    if (tid == 0) s_n = 0;
    // Key positions of this workgroup: 64-key chunks c = (j * 16 + wave) * wgs + b, j = 0, 1, ... -- interleaved at
    // wave granularity, so that the near leaves' dense runs of passing keys (most of a tree query's candidates lie in
    // its first one or two leaves) are shared by all workgroups.  The first KP rounds travel while the pivot is computed.
    const uint64_t *list = a.cand + (size_t)q * a.cap;
    const uint32_t kwave = tid >> 6, klane = tid & 63u;
    auto key_pos = [&](uint32_t j) { return ((uint64_t)(j * (nt >> 6) + kwave) * wa.wgs + b) * 64u + klane; };
    constexpr int KP = 4;
    uint64_t kpre[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        const uint64_t i = key_pos((uint32_t)j);
        kpre[j] = i < cnt ? list[i] : SCANN_KEY_MAX;
    }
#ifdef SCANN_WIDE_TIMING
    tf[1] = wall_clock64();
#endif
    // ---- the pivot (every workgroup of the query computes the same one): an upper bound of the m-th smallest group
    // minimum -- the upper edge of its bin in a 4096-bin histogram over [min, max] of the minima.  One read of the
    // minima (16 per thread, in registers), four barriers; the exact m-th minimum (block_select: a dozen barriers
    // of 1024 threads, 9 us) would let a few dozen keys fewer pass.
    uint32_t pivot = 0xFFFFFFFEu;
    const uint32_t g = wide_group(cnt, m), ng = (cnt + g - 1u) / g;
    if (cnt > m && ng >= m) {
        const uint32_t *mins = wa.mins + (size_t)q * wa.ng_stride;
        constexpr int RV = 16;
        if (ng <= (uint32_t)RV * nt) {
            uint32_t *s_w = reinterpret_cast<uint32_t *>(s_red);   // [0..15] min, [16..31] max, [32..47] present / scan, [48] bin
            uint32_t mv[RV];
            uint32_t vmin = 0xFFFFFFFFu, vmax = 0, present = 0;
#pragma unroll
            for (int e = 0; e < RV; ++e) {
                const uint32_t i = (uint32_t)e * nt + tid;
                mv[e] = ((uint32_t)e * nt < ng && i < ng) ? mins[i] : 0xFFFFFFFFu;
            }
#pragma unroll
            for (int e = 0; e < RV; ++e)
                if (mv[e] != 0xFFFFFFFFu) {
                    vmin = min(vmin, mv[e]);
                    vmax = max(vmax, mv[e]);
                    ++present;
                }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                vmin = min(vmin, (uint32_t)__shfl_xor((int)vmin, o));
                vmax = max(vmax, (uint32_t)__shfl_xor((int)vmax, o));
                present += (uint32_t)__shfl_xor((int)present, o);
            }
            const uint32_t wave = tid >> 6, lane = tid & 63u;
            if (lane == 0) {
                s_w[wave] = vmin;
                s_w[16 + wave] = vmax;
                s_w[32 + wave] = present;
            }
            for (uint32_t i = tid; i < kSelBinsMax; i += nt) s_hist[i] = 0;
            __syncthreads();
            present = 0;
            for (uint32_t w2 = 0; w2 < (nt >> 6); ++w2) {
                vmin = min(vmin, s_w[w2]);
                vmax = max(vmax, s_w[16 + w2]);
                present += s_w[32 + w2];
            }
            __syncthreads();   // (s_w[32..] is reused by the scan)
            if (present >= m) {   // block-uniform (else: fewer than m groups hold an allowed point, everything passes)
                const uint32_t range = vmax - vmin;
                uint32_t sh = 0;
                while ((range >> sh) >= kSelBinsMax) ++sh;
#pragma unroll
                for (int e = 0; e < RV; ++e)
                    if (mv[e] != 0xFFFFFFFFu) atomicAdd(&s_hist[(mv[e] - vmin) >> sh], 1u);
                __syncthreads();
                const uint32_t bin = block_hist_rank_bin(s_hist, s_w, m);
                const uint64_t hi = (uint64_t)vmin + (((uint64_t)bin + 1u) << sh) - 1u;
                pivot = hi > vmax ? vmax : (uint32_t)hi;
                if (pivot == 0xFFFFFFFFu) pivot = 0xFFFFFFFEu;
            }
        } else {   // very long streams: the exact select, from L2
            __syncthreads();
            const uint32_t pv = block_select<uint32_t>(mins, ng, m, sel_cfg(ng), s_hist, reinterpret_cast<uint32_t *>(s_slist), s_red);
            if (pv != 0xFFFFFFFFu) pivot = pv;   // (fewer than m groups hold an allowed point: everything passes)
        }
    }
    __syncthreads();
#ifdef SCANN_WIDE_TIMING
    tf[2] = wall_clock64();
#endif
    // a batch of collected keys: decode, exact distance (8 lanes per candidate), append to the compact arrays
    auto flush = [&]() {
        const uint32_t n = min(s_n, kWideList);
        for (uint32_t c0 = 0; c0 < n; c0 += nt / 8) {
            const uint32_t c = c0 + (tid >> 3), lane8 = tid & 7u;
            const bool act = c < n;
            uint32_t idx = 0, rowi = 0;
            uint64_t key = 0;
            if (act) {
                key = s_pass[c];
                const uint32_t vpos = (uint32_t)key;
                uint32_t lo = 0, hi = P;
                while (hi - lo > 1) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (s_dvb[mid] <= vpos) lo = mid; else hi = mid;
                }
                const uint32_t csr = s_drow[lo] + (vpos - s_dvb[lo]);
                idx = ix.leaf_ids ? ix.leaf_ids[csr] : csr;
                rowi = ix.rows_csr ? csr : idx;
            }
            float r = 0.0f;
            if (a.exact_reorder) r = exact_pair_8lanes<16>(ix, s_q, ix.rows + (size_t)rowi * ix.stride, act, lane8);
            if (act && lane8 == 0) {
                s_ix[c] = idx;
                s_eb[c] = a.exact_reorder ? f32_to_ordered(r) : (uint32_t)(key >> 32);
            }
        }
        if (tid == 0) s_base = atomicAdd(&wa.ccnt[q], n);
        __syncthreads();
        const uint32_t base = s_base;
        if (tid == 0 && base + n > wa.cap2) atomicExch(&a.counters[CNT_STATUS], (uint32_t)SCANN_HIP_RESOURCE_EXHAUSTED);
        for (uint32_t i = tid; i < n; i += nt)
            if (base + i < wa.cap2) {
                const size_t e = (size_t)q * wa.cap2 + base + i;
                wa.ckey[e] = s_pass[i];
                wa.ceb[e] = s_eb[i];
                wa.cidx[e] = s_ix[i];
            }
        __syncthreads();
        if (tid == 0) s_n = 0;
        __syncthreads();
    };
    // ---- rounds of 16 chunks (one per wave)
    for (uint32_t jb = 0; (uint64_t)jb * (nt >> 6) * wa.wgs * 64u < cnt; ++jb) {
        const uint64_t i = key_pos(jb);
        uint64_t key = SCANN_KEY_MAX;
        if (jb < (uint32_t)KP) {
#pragma unroll
            for (int j = 0; j < KP; ++j)
                if (jb == (uint32_t)j) key = kpre[j];
        } else if (i < cnt) {
            key = list[i];
        }
        const bool keep = key != SCANN_KEY_MAX && (uint32_t)(key >> 32) <= pivot;
        uint32_t wtot;
        const uint32_t wpre = wave_prefix_count(keep, &wtot);
        uint32_t base = 0;
        if ((tid & 63u) == 0 && wtot) base = atomicAdd(&s_n, wtot);
        base = (uint32_t)__shfl((int)base, 0);
        if (keep) s_pass[base + wpre] = key;   // (s_n <= kWideList - nt before the block: never past the end)
        __syncthreads();
        const uint32_t collected = s_n;
        __syncthreads();                       // (everyone has read it before the next block adds to it)
        if (collected > kWideList - nt) flush();
    }
    __syncthreads();
#ifdef SCANN_WIDE_TIMING
    tf[3] = wall_clock64();
    const uint32_t npass = s_n;
#endif
    if (s_n) flush();
#ifdef SCANN_WIDE_TIMING
    tf[4] = wall_clock64();
    if (tid == 0 && b == 0) printf("filter: cnt %u pass %u setup %.2f pivot %.2f filter %.2f flush %.2f us\n", cnt, npass, (tf[1] - tf[0]) * 0.01, (tf[2] - tf[1]) * 0.01, (tf[3] - tf[2]) * 0.01, (tf[4] - tf[3]) * 0.01);
#endif
}

__global__ __launch_bounds__(kSelectThreads) void wide_final_kernel(SmallArgs a, WideArgs wa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_fdyn[];   // u64[cap2]
    __shared__ uint64_t s_slist[kSelListMax], s_red[48];
    __shared__ uint32_t s_hist[kSelBinsMax], s_ce[64], s_cs[64], s_cn;
    __shared__ uint64_t s_ck[64];
    const uint32_t q = blockIdx.x, tid = threadIdx.x, nt = kSelectThreads, wave = tid >> 6, lane = tid & 63u;
    const uint32_t m = a.m, k = a.k;
    uint64_t *s_v = reinterpret_cast<uint64_t *>(s_fdyn);
    const bool polled = a.done != nullptr;
    auto out_store = [&](auto *p, auto v) {
        if (polled) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        else *p = v;
    };
#ifdef SCANN_WIDE_TIMING
    uint64_t tq[8];
    int tqi = 0;
#define WIDE_T() do { __syncthreads(); tq[tqi++] = wall_clock64(); } while (0)
#else
#define WIDE_T() do { } while (0)
#endif
    WIDE_T();
    const uint32_t appended = wa.ccnt[q];
    const bool overflow = appended > wa.cap2;
    const uint32_t c2 = min(appended, wa.cap2);
    const uint64_t *ckey = wa.ckey + (size_t)q * wa.cap2;
    const uint32_t *ceb = wa.ceb + (size_t)q * wa.cap2, *cidx = wa.cidx + (size_t)q * wa.cap2;
    const uint32_t nsel = min(c2, m), nout = overflow ? 0u : min(k, nsel);
    if (nout) {
        // entry e * nt + tid of the compact arrays lives in this lane's registers (cap2 <= 16 * nt)
        constexpr int E0 = 16;
        uint64_t kk[E0];
        uint32_t eb[E0];
#pragma unroll
        for (int e = 0; e < E0; ++e) {
            const uint32_t i = (uint32_t)e * nt + tid;
            kk[e] = SCANN_KEY_MAX;
            eb[e] = 0xFFFFFFFFu;
            if ((uint32_t)e * nt < c2 && i < c2) {
                kk[e] = ckey[i];
                eb[e] = ceb[i];
            }
        }
        WIDE_T();
        // the candidates: the m smallest keys (mod.rs:283-293); everything above T drops out
        uint64_t T = SCANN_KEY_MAX - 1;
        if (c2 > m) {
            // block_select's scheme on the register copy (six barriers instead of a dozen): histogram of the keys over
            // [min, max], the bin of rank m, its members ranked exactly by counting
            uint32_t *s_w = reinterpret_cast<uint32_t *>(s_red);
            uint64_t kmin = SCANN_KEY_MAX, kmax = 0;
#pragma unroll
            for (int e = 0; e < E0; ++e)
                if ((uint32_t)e * nt < c2 && kk[e] != SCANN_KEY_MAX) {
                    kmin = kk[e] < kmin ? kk[e] : kmin;
                    kmax = kk[e] > kmax ? kk[e] : kmax;
                }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const uint64_t x = shfl_xor_t<uint64_t>(kmin, o), y = shfl_xor_t<uint64_t>(kmax, o);
                kmin = x < kmin ? x : kmin;
                kmax = y > kmax ? y : kmax;
            }
            if (lane == 0) {
                s_red[wave] = kmin;
                s_red[16 + wave] = kmax;
            }
            for (uint32_t i = tid; i < kSelBinsMax; i += nt) s_hist[i] = 0;
            if (tid == 0) s_cn = 0;
            __syncthreads();
            for (uint32_t w2 = 0; w2 < (nt >> 6); ++w2) {
                kmin = s_red[w2] < kmin ? s_red[w2] : kmin;
                kmax = s_red[16 + w2] > kmax ? s_red[16 + w2] : kmax;
            }
            uint32_t ksh = 0;
            while (((kmax - kmin) >> ksh) >= (uint64_t)kSelBinsMax) ++ksh;
#pragma unroll
            for (int e = 0; e < E0; ++e)
                if ((uint32_t)e * nt < c2 && kk[e] != SCANN_KEY_MAX) atomicAdd(&s_hist[(uint32_t)((kk[e] - kmin) >> ksh)], 1u);
            __syncthreads();   // (everyone has read the wave minima / maxima: the scan reuses their words)
            const uint32_t kbin = block_hist_rank_bin(s_hist, s_w, m);
            const uint32_t krk = s_w[49], kpop = s_hist[kbin];
            const uint64_t klo = kmin + ((uint64_t)kbin << ksh);
            uint64_t khi = klo + (((uint64_t)1 << ksh) - 1);
            if (khi > kmax || khi < klo) khi = kmax;
            if (ksh == 0) {
                T = klo;
            } else if (kpop <= kSelListMax) {
#pragma unroll
                for (int e = 0; e < E0; ++e)
                    if ((uint32_t)e * nt < c2 && kk[e] >= klo && kk[e] <= khi) s_slist[atomicAdd(&s_cn, 1u)] = kk[e];
                __syncthreads();
                for (uint32_t i = tid; i < kpop; i += nt) {
                    const uint64_t v = s_slist[i];
                    uint32_t r = 0;
                    for (uint32_t j2 = 0; j2 < kpop; ++j2) r += s_slist[j2] < v ? 1u : 0u;   // (keys are unique)
                    if (r + 1 == krk) s_red[40] = v;
                }
                __syncthreads();
                T = s_red[40];
            } else {   // a crowded bin: the general select on an LDS copy
#pragma unroll
                for (int e = 0; e < E0; ++e)
                    if ((uint32_t)e * nt < c2 && (uint32_t)e * nt + tid < c2) s_v[(uint32_t)e * nt + tid] = kk[e];
                __syncthreads();
                T = block_select<uint64_t>(s_v, c2, m, sel_cfg(c2), s_hist, s_slist, s_red);
            }
            __syncthreads();
        }
        WIDE_T();
#pragma unroll
        for (int e = 0; e < E0; ++e)
            if (kk[e] > T) {
                kk[e] = SCANN_KEY_MAX;
                eb[e] = 0xFFFFFFFFu;
            }
        // the nout best by (exact, merge key) (mod.rs:342-364).  The entries are in registers: a 4096-bin histogram of
        // the candidates' exact distances over [min, max] gives the bin of rank nout; the entries up to that bin's
        // upper edge (nout and a few more: the low tail is sparse) go to a short list, which one wave ranks by
        // counting.  More than 64 of them (heavy ties): the two-level tournament of small_finish_body instead.
        uint32_t *s_w = reinterpret_cast<uint32_t *>(s_red);
        uint32_t emin = 0xFFFFFFFFu, emax = 0;
#pragma unroll
        for (int e = 0; e < E0; ++e)
            if ((uint32_t)e * nt < c2 && kk[e] != SCANN_KEY_MAX) {
                emin = min(emin, eb[e]);
                emax = max(emax, eb[e]);
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            emin = min(emin, (uint32_t)__shfl_xor((int)emin, o));
            emax = max(emax, (uint32_t)__shfl_xor((int)emax, o));
        }
        if (lane == 0) {
            s_w[wave] = emin;
            s_w[16 + wave] = emax;
        }
        for (uint32_t i = tid; i < kSelBinsMax; i += nt) s_hist[i] = 0;
        if (tid == 0) s_cn = 0;
        __syncthreads();
        for (uint32_t w2 = 0; w2 < (nt >> 6); ++w2) {
            emin = min(emin, s_w[w2]);
            emax = max(emax, s_w[16 + w2]);
        }
        uint32_t esh = 0;
        while (((emax - emin) >> esh) >= kSelBinsMax) ++esh;
#pragma unroll
        for (int e = 0; e < E0; ++e)
            if ((uint32_t)e * nt < c2 && kk[e] != SCANN_KEY_MAX) atomicAdd(&s_hist[(eb[e] - emin) >> esh], 1u);
        __syncthreads();
        const uint32_t ebin = block_hist_rank_bin(s_hist, s_w, nout);
        const uint64_t ehi64 = (uint64_t)emin + (((uint64_t)ebin + 1u) << esh) - 1u;
        const uint32_t ehi = ehi64 > emax ? emax : (uint32_t)ehi64;
#pragma unroll
        for (int e = 0; e < E0; ++e)
            if ((uint32_t)e * nt < c2 && kk[e] != SCANN_KEY_MAX && eb[e] <= ehi) {
                const uint32_t pos = atomicAdd(&s_cn, 1u);
                if (pos < 64u) {
                    s_ce[pos] = eb[e];
                    s_ck[pos] = kk[e];
                    s_cs[pos] = (uint32_t)e * nt + tid;
                }
            }
        __syncthreads();
        const uint32_t cn = s_cn;   // >= nout
        WIDE_T();
        if (cn <= 64u) {
            if (tid < 64) {
                const bool have = tid < cn;
                const uint32_t ce = have ? s_ce[tid] : 0xFFFFFFFFu;
                const uint64_t ck = have ? s_ck[tid] : SCANN_KEY_MAX;
                uint32_t rank = 0;
                for (uint32_t j = 0; j < cn; ++j) {
                    const uint32_t oe = (uint32_t)__shfl((int)ce, (int)j);
                    const uint64_t ok = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(ck >> 32), (int)j) << 32) |
                                        (uint32_t)__shfl((int)(uint32_t)ck, (int)j);
                    rank += (oe < ce || (oe == ce && ok < ck)) ? 1u : 0u;
                }
                if (have && rank < nout) {
                    out_store(&a.out_idx[(size_t)q * k + rank], cidx[s_cs[tid]]);
                    out_store(&a.out_dist[(size_t)q * k + rank], ordered_to_f32(ce));
                }
            }
        } else {
        __syncthreads();   // (the histogram and the select's list are reused below)
        uint32_t *f_eb = s_hist, *f_sl = s_hist + kSelectThreads;
        uint64_t *f_kk = s_slist;
        for (uint32_t r0 = 0; r0 < nout; ++r0) {
            uint32_t b_eb = 0xFFFFFFFFu, b_sl = 0xFFFFFFFFu;
            uint64_t b_kk = SCANN_KEY_MAX;
#pragma unroll
            for (int e = 0; e < E0; ++e)
                if ((uint32_t)e * nt < c2 && kk[e] != SCANN_KEY_MAX && (eb[e] < b_eb || (eb[e] == b_eb && kk[e] < b_kk))) {
                    b_eb = eb[e];
                    b_kk = kk[e];
                    b_sl = (uint32_t)e * nt + tid;
                }
            wave_argmin96(b_eb, b_kk, b_sl);
            if (b_kk == SCANN_KEY_MAX) b_sl = 0xFFFFFFFFu;   // (the wave's pool is empty)
#pragma unroll
            for (int e = 0; e < E0; ++e)
                if ((uint32_t)e * nt < c2 && (uint32_t)e * nt + tid == b_sl) {
                    kk[e] = SCANN_KEY_MAX;
                    eb[e] = 0xFFFFFFFFu;
                }
            if (lane == 0) {
                f_eb[wave * nout + r0] = b_eb;
                f_kk[wave * nout + r0] = b_kk;
                f_sl[wave * nout + r0] = b_sl;
            }
        }
        __syncthreads();
        if (tid < 64) {
            constexpr int E = kSelectThreads / 64;
            const uint32_t nfin = (nt >> 6) * nout;           // <= 16 * 64
            uint32_t feb[E], fsl[E];
            uint64_t fkk[E];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const uint32_t j = (uint32_t)e * 64u + tid;
                const bool ok = j < nfin && f_sl[j] != 0xFFFFFFFFu;
                feb[e] = ok ? f_eb[j] : 0xFFFFFFFFu;
                fkk[e] = ok ? f_kk[j] : SCANN_KEY_MAX;
                fsl[e] = ok ? f_sl[j] : 0xFFFFFFFFu;
            }
            uint32_t my_eb = 0xFFFFFFFFu, my_sl = 0xFFFFFFFFu;   // lane r0 keeps round r0's winner
            for (uint32_t r0 = 0; r0 < nout; ++r0) {
                uint32_t b_eb = 0xFFFFFFFFu, b_sl = 0xFFFFFFFFu;
                uint64_t b_kk = SCANN_KEY_MAX;
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if ((uint32_t)e * 64u < nfin && fsl[e] != 0xFFFFFFFFu &&
                        (feb[e] < b_eb || (feb[e] == b_eb && fkk[e] < b_kk))) {
                        b_eb = feb[e];
                        b_kk = fkk[e];
                        b_sl = fsl[e];
                    }
                wave_argmin96(b_eb, b_kk, b_sl);
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if ((uint32_t)e * 64u < nfin && fsl[e] == b_sl) {   // (entry slots are unique: exactly one lane, one entry)
                        feb[e] = 0xFFFFFFFFu;
                        fkk[e] = SCANN_KEY_MAX;
                        fsl[e] = 0xFFFFFFFFu;
                    }
                if (tid == r0) {
                    my_eb = b_eb;
                    my_sl = b_sl;
                }
            }
            if (tid < nout) {   // the winners' datapoint indices: one parallel round trip
                out_store(&a.out_idx[(size_t)q * k + tid], cidx[my_sl]);
                out_store(&a.out_dist[(size_t)q * k + tid], ordered_to_f32(my_eb));
            }
        }
        }
    }
    WIDE_T();
#ifdef SCANN_WIDE_TIMING
    if (tid == 0 && nout) printf("final: c2 %u load %.2f select %.2f shortlist %.2f rank %.2f us\n", c2, (tq[1] - tq[0]) * 0.01, (tq[2] - tq[1]) * 0.01, (tq[3] - tq[2]) * 0.01, (tq[4] - tq[3]) * 0.01);
#endif
    for (uint32_t i = nout + tid; i < k; i += nt) {
        out_store(&a.out_idx[(size_t)q * k + i], kInvalid);
        out_store(&a.out_dist[(size_t)q * k + i], __builtin_inff());
    }
    if (tid == 0) out_store(&a.out_count[q], overflow ? (polled ? 0xFFFFFFFFu : 0u) : nout);   // (host calls: repeat on the batched pipeline)
    if (a.done) {   // (see small_finish_body)
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
        if (tid == 0) __hip_atomic_store(&a.done[q], a.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// the three-launch pipeline for small batches (see "Small batches" above)
static int launch_search_small(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st, hipEvent_t ev0,
                               hipEvent_t ev1) {
    SmallArgs a;
    a.nq = w.nq; a.P = w.P; a.m = w.m; a.k = w.k; a.cap = w.cap; a.q_stride = w.q_stride;
    a.exact_reorder = w.exact_reorder; a.queries = w.queries; a.tokens = w.tokens; a.vbase = w.vbase;
    a.cand = w.cand; a.counters = w.counters; a.allow = w.allow; a.allow_bits = w.allow_bits; a.allow_stride = w.allow_stride;
    a.out_idx = w.out_idx; a.out_dist = w.out_dist; a.out_count = w.out_count;
    a.done = w.small_done; a.seq = w.small_seq; a.chunk = w.chunk;
    // the one-launch forms: every workgroup repeats the leaf selection
    FusedArgs f;
    f.L = ix.L; f.n_pow2 = next_pow2_u32(ix.L);
    f.p_pow2 = (w.P * 4u <= f.n_pow2) ? next_pow2_u32(std::max(1u, w.P)) : 0u;
    f.st = w.st; f.cdist = w.cdist; f.token_dists = w.token_dists; f.tokens = w.tokens; f.vbase = w.vbase;
    f.sbase = w.sbase; f.tickets = w.pipeline == TxhPipeline::Wide ? nullptr : w.small_tickets;
    const SelCfg lcfg = sel_cfg(ix.L);
    const size_t lds_sel = ix.ah_mode ? 0 : (size_t)(f.n_pow2 + f.p_pow2) * sizeof(uint64_t) + (size_t)lcfg.bins * 4 +
                                            (size_t)lcfg.list * 8 + 48 * 8 + 64 * 4 + (size_t)ix.L * 8 +
                                            (size_t)((ix.dim + 3u) & ~3u) * 4 + 16;
    if (w.pipeline == TxhPipeline::Wide) {   // the wide few-query pipeline ("Few queries, long streams")
        WideArgs wa;
        wa.ng_stride = w.cap; wa.cap2 = w.wide_cap2;
        wa.wgs = std::min(256u, std::max(8u, ceil_div_u32(w.cap, 1024u)));
        wa.mins = w.wide_min; wa.ckey = w.wide_ckey; wa.ceb = w.wide_ceb; wa.cidx = w.wide_cidx; wa.ccnt = w.wide_cnt;
        const size_t lds_scan = ((size_t)ix.S * ix.kp + ix.dim) * sizeof(float);
        if (ev0) SCANN_HIP_CHECK(hipEventRecord(ev0, st));
        SCANN_TRY(launch(wide_scan_kernel, dim3(w.grid, w.nq), dim3(kSelectThreads), std::max(lds_sel, lds_scan), st, ix, a, f, wa));
        if (ev1) SCANN_HIP_CHECK(hipEventRecord(ev1, st));
        const size_t lds_f = (size_t)((ix.dim + 3u) & ~3u) * 4;
        SCANN_TRY(launch(wide_filter_kernel, dim3(wa.wgs, w.nq), dim3(kSelectThreads), lds_f, st, ix, a, wa));
        const size_t lds_l = (size_t)w.wide_cap2 * 8;
        SCANN_TRY(launch(wide_final_kernel, dim3(w.nq), dim3(kSelectThreads), lds_l, st, a, wa));
        return SCANN_HIP_OK;
    }
    if (w.fused) {   // one launch when the grid stays small
        const size_t lds_scan = ((size_t)(ix.exact_scan ? 0u : ix.S * ix.kp) + ix.dim) * sizeof(float);
        const size_t lds = std::max(lds_sel, lds_scan);
        // (the finish stage's static arrays are ~78 KB: from ~2200 leaves the selection's dynamic part passes 64 KB, and
        // launch() sets the attribute so that it leaves room for both)
        if (ev0) SCANN_HIP_CHECK(hipEventRecord(ev0, st));
        SCANN_TRY(launch(small_fused_kernel, dim3(w.grid, w.nq), dim3(kSelectThreads), lds, st, ix, a, f));
        if (ev1) SCANN_HIP_CHECK(hipEventRecord(ev1, st));
        return SCANN_HIP_OK;
    }
    if (ix.ah_mode) {
        SCANN_TRY(launch_ah_tokens(ix, w, st));
    } else {   // (lds_sel: + the leaf size tables and the query, the kernel's inline mode)
        SCANN_TRY(launch(select_leaves_kernel, dim3(w.nq), dim3(kSelectThreads), lds_sel, st, w.cdist, ix.L, f.n_pow2, w.P,
                         f.p_pow2, ix.leaf_gsize, ix.leaf_off, w.st, w.tokens, w.token_dists, w.vbase, w.sbase, ix.centers_t,
                         w.queries, w.q_stride, ix.dim, ix.centers_pitch));
    }
    // exact scans read a whole row per point (one row per thread keeps every load in flight at once); the
    // ADC scan amortises the table build of its workgroup over four points per thread
    a.chunk = ix.exact_scan ? 256u : kSmallChunk;
    const size_t lds_scan = ((size_t)(ix.exact_scan ? 0u : ix.S * ix.kp) + ix.dim) * sizeof(float);
    if (ev0) SCANN_HIP_CHECK(hipEventRecord(ev0, st));
    SCANN_TRY(launch(small_scan_kernel, dim3(ceil_div_u32(w.small_max_leaf, a.chunk), w.nq * w.P), dim3(256),
                     lds_scan, st, ix, a));
    if (ev1) SCANN_HIP_CHECK(hipEventRecord(ev1, st));
    const size_t lds_fin = (size_t)ix.dim * sizeof(float);
    SCANN_TRY(launch(small_finish_kernel, dim3(w.nq), dim3(kSelectThreads), lds_fin, st, ix, a));
    return SCANN_HIP_OK;
}

// The work lists follow the scan kernel's items.
static WorkTiling work_tiling(const TxhIndexDev &ix, const TxhWork &w) {
    switch (w.scan) {
        case TxhScan::Exact: return {kExactRows, exact_quads_per_tile(ix.dim), 1u};
        case TxhScan::Mfma16: return {kMfmaRange, 4u, 1u};
        case TxhScan::Mfma32: return {kMfmaRange, 8u, 1u};
        case TxhScan::Smfmac: return w.sp_pairs64 ? WorkTiling{kSpRange64, 16u, 1u} : WorkTiling{kMfmaRange, 8u, 1u};
        case TxhScan::Resident: return {kResThreads * kScanPPT, kResQuads, w.res_cl};
        default: return {scan_tile_points(ix), w.qpt, 1u};
    }
}

int txh_launch_search(const TxhIndexDev &ix, const TxhWork &w, bool local_only, hipStream_t st,
                      hipEvent_t ev0, hipEvent_t ev1) {
    if (w.nq == 0) return SCANN_HIP_OK;
    if (w.pipeline != TxhPipeline::Staged && !local_only && !w.need_sorted_cands) return launch_search_small(ix, w, st, ev0, ev1);
    // partition and work lists
    const WorkTiling tiling = work_tiling(ix, w);
    if (ix.ah_mode && ix.L == 1 && w.P == 1) {
        SCANN_TRY(launch_ah_setup(ix, w, tiling, st));
    } else {
        SCANN_TRY(launch_work_init(ix, w, st));
        SCANN_TRY(launch_partition_stage(ix, w, st));
        SCANN_TRY(launch_work_lists(ix, w, tiling, st));
    }
    if (w.scan == TxhScan::Exact) {
        SCANN_TRY(launch_exact_scan(ix, w, st, ev0, ev1));
    } else {
        // tables, bound, scan
        SCANN_TRY(launch_lut_build(ix, w, st));
        SCANN_TRY(with_codec(ix, [](auto) { return (int)SCANN_HIP_OK; }));   // an unsupported code layout ends the call here
        if (w.sample_mfma) SCANN_TRY(launch_sample_mfma_bound(ix, w, st));
        else SCANN_TRY(launch_gather_bound(ix, w, st));
        if (ix.code_bits == 4 && txh_scan_is_mfma(w.scan)) SCANN_TRY(launch_prefilter_refine(ix, w, st, ev0, ev1));
        else SCANN_TRY(launch_gather_scan(ix, w, st, ev0, ev1));
    }
    // select, re-rank, final
    SCANN_TRY(launch_select(ix, w, local_only, st));
    if (!w.exact_reorder) return SCANN_HIP_OK;
    SCANN_TRY(launch_rerank(ix, w, local_only, st));
    if (local_only) return SCANN_HIP_OK;
    return launch_final(w, st);
}

// Per-destination blocks for the all_to_all exchange: rank d merges the queries
// [d * nq/world, (d+1) * nq/world), so it needs exactly those rows of every rank's candidate
// arrays.  Block d = [keys u64 Qr*m | idx u32 Qr*m | exact f32 Qr*m | count u32 Qr], blocks
// block_bytes apart -- the layout txh_merge_device reads with rank_stride_bytes = block_bytes.
__global__ void pack_blocks_kernel(uint32_t world, uint32_t nq, uint32_t m,
                                   const uint64_t *__restrict__ keys, const uint32_t *__restrict__ idx,
                                   const float *__restrict__ exact, const uint32_t *__restrict__ count,
                                   unsigned char *__restrict__ out, size_t block_bytes) {
    const uint32_t qr = nq / world;
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < (uint64_t)nq * m) {
        const uint32_t q = (uint32_t)(e / m), i = (uint32_t)(e - (uint64_t)q * m);
        const uint32_t d = q / qr, ql = q - d * qr;
        unsigned char *blk = out + (size_t)d * block_bytes;
        const size_t slot = (size_t)ql * m + i, per = (size_t)qr * m;
        reinterpret_cast<uint64_t *>(blk)[slot] = keys[e];
        reinterpret_cast<uint32_t *>(blk + per * 8)[slot] = idx[e];
        reinterpret_cast<float *>(blk + per * 12)[slot] = exact[e];
    }
    if (e < nq) {
        const uint32_t q = (uint32_t)e, d = q / qr, ql = q - d * qr;
        reinterpret_cast<uint32_t *>(out + (size_t)d * block_bytes + (size_t)qr * m * 16)[ql] = count[q];
    }
}

int txh_launch_pack_blocks(uint32_t world, uint32_t nq, uint32_t m_local, const uint64_t *d_keys,
                           const uint32_t *d_idx, const float *d_exact, const uint32_t *d_count,
                           void *d_out, size_t block_bytes, hipStream_t st) {
    if (nq == 0) return SCANN_HIP_OK;
    if (world == 0 || nq % world != 0)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "the batch must divide evenly over the ranks");
    const size_t need = (size_t)(nq / world) * m_local * 16 + (size_t)(nq / world) * 4;
    if (block_bytes < need || (block_bytes & 7u))
        return fail(SCANN_HIP_INVALID_ARGUMENT, "block_bytes too small or not a multiple of 8");
    const uint64_t work = std::max<uint64_t>((uint64_t)nq * m_local, nq);
    SCANN_TRY(launch(pack_blocks_kernel, dim3((uint32_t)ceil_div_u64(work, 256)), dim3(256), 0, st, world, nq,
                     m_local, d_keys, d_idx, d_exact, d_count, static_cast<unsigned char *>(d_out),
                     block_bytes));
    return SCANN_HIP_OK;
}

int txh_launch_merge(uint32_t world, uint32_t nq, uint32_t m_local, uint32_t m, uint32_t k,
                     size_t rank_stride_bytes, const uint64_t *d_keys, const uint32_t *d_idx,
                     const float *d_exact, const uint32_t *d_count, uint32_t *d_out_idx,
                     float *d_out_dist, uint32_t *d_out_count, uint32_t *d_status, hipStream_t st,
                     const uint32_t *d_qoff) {
    if (nq == 0) return SCANN_HIP_OK;
    if (world == 0 || world > 64) return fail(SCANN_HIP_INVALID_ARGUMENT, "world must be 1..64");
    if (m_local == 0 || m_local > m) return fail(SCANN_HIP_INVALID_ARGUMENT, "need 0 < m_local <= m");
    if (m > kMaxPreReorderK)
        return fail(SCANN_HIP_UNIMPLEMENTED, "pre_reorder_k exceeds the LDS merge capacity");
    const uint32_t m2 = next_pow2_u32(std::max<uint32_t>(1u, m));
    const size_t lds = (size_t)m2 * 12 + 16 + (kSelectThreads / 64) * 8;
    SCANN_TRY(launch(merge_kernel, dim3(nq), dim3(kSelectThreads), lds, st, world, nq, m_local, m, k, m2,
                     rank_stride_bytes, d_keys, d_idx, d_exact, d_count, d_out_idx, d_out_dist,
                     d_out_count, d_status, d_qoff));
    return SCANN_HIP_OK;
}

}  // namespace scann

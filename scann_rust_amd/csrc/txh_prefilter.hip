// txh_prefilter.hip -- the integer-MFMA scans of the tree / flat-hasher search (see txh.hip for the pipeline): K6d / K6e,
// the dense and 2:4-sparse prefilters with their table and operand-plane builds, and the exact refine.
//
// Launch order of launch_prefilter_refine (one stream; the timing events enclose the scan alone):
//   lut8_build_kernel                          quantised tables (sparse prefilter: the pass bound folded in)
//   adc_mfma16 / adc_mfma / adc_smfmac[_wide][_pq]_kernel / adc_smfmac[_pq]_kernel64
//                                              survivors -> per-query lists (cand32, cand32_codes, cand32_cnt)
//   adc_refine_kernel                          lists -> exact keys, key <= T -> cand / cand_cnt
// and under TxhPlan::sp_bitmap (flat hashers, 64-pair items; SCANN_HIP_SP_BITMAP=0 keeps the order above):
//   lut8_build_kernel
//   adc_smfmac_bits_kernel64                   each item's survivor bitmap -> surv[query][range * 32 ..], no lists
//   adc_refine_bits_kernel                     walks the query's row of surv, allow test, exact keys -> cand / cand_cnt
#include "launch.h"
#include "txh_dev.h"
#include "txh_stages.h"

namespace scann {

// =====================================================================================
// K6d: ADC scan as an integer-MFMA prefilter + exact refine (4-bit codes, threshold known).
//
// The f32 scan above is bound by the LDS table gather (one ds_read_b128 per point, subspace and
// quad of queries).  The same sums over QUANTISED tables are a matrix product:
//     one-hot(codes) [points x (S*16)]  x  lut8 [(S*16) x pairs]   (u8 tables as i8 minus 128)
// which v_mfma_i32_32x32x32_i8 computes exactly (integer) at 1024 MAC/clk/SIMD: a 32-point x
// 32-pair tile costs S/2 MFMAs.  The integer sum BOUNDS the reference's f32 sum: with per-subspace
// offsets mn_s and one scale sc per pair, every table entry v satisfies |v - (mn_s + sc*q)| <=
// sc*(0.5 + 1e-9), so a point whose f32 sum passes the filter bound T has
//     sum_q <= (T*(1 + S*2^-23) - sum mn_s)/sc + S/2 + 1
// (the factor covers the rounding of the sequential f32 adds of non-negative terms).  Points under
// that integer bound -- the true survivors plus ~10 % -- are listed per query as stream positions,
// and adc_refine_kernel recomputes THEIR distances with the reference's arithmetic (f32 tables,
// subspace order: hashes/lut.rs:74-82), forms the merge keys and applies the exact filter.  The
// candidate lists handed to select_rerank_kernel are therefore identical to adc_scan_kernel's:
// the same shortlist-plus-proof pattern as the bf16 brute-force pass (bf.hip).
//
// Work decomposition: every WAVE pulls its own items (leaf, tile of 32 pair slots, range of
// kMfmaRange points) from the tile queues; the pair tile's tables are the wave's B fragments for
// the whole item (S/2 x 4 VGPRs), the A fragment of a (point, subspace pair) is one row of a
// 16 x 16-byte identity table in LDS (one conflict-free ds_read_b128 at offset code * 16), the
// 16 results of a lane belong to ONE pair (column) and are compared with that pair's bound.
// Survivors are staged per (wave, pair) in LDS and written at the end of the item as one
// contiguous segment per pair behind ONE returning atomic per pair.
// =====================================================================================
constexpr uint32_t kMfmaStage = 56;       // staged survivors per (wave, pair)
constexpr uint32_t kMfmaWaves = 4;        // waves per workgroup
#ifndef SCANN_MFMA_MINW
#define SCANN_MFMA_MINW 3
#endif
#ifndef SCANN_MFMA_DEPTH
#define SCANN_MFMA_DEPTH 3
#endif
constexpr int kMfmaDepth = SCANN_MFMA_DEPTH;   // one-hot LDS reads in flight per wave
constexpr uint32_t kRefineTablesMax = 40; // pair tables (2 KB each at S = 32) staged in LDS by the refine

// lutq [quad][s][16][4] f32 -> lut8 [slot][s][16] i8 (quantised value - 128) + meta[slot]
// Pass bound of a pair slot on the integer sums (see the derivation above), as thr + 1: a point passes iff
// acc - thr1 < 0.  Sums lie in [-128 S, 127 S]; the bound is clamped just outside that range (everything
// passes: no filter bound, or a table that is not quantised; nothing passes: padding slots).
__device__ __forceinline__ int mfma_pass_bound(uint32_t S, uint32_t pq, uint64_t T, double bias_sum, double scale) {
    const int lim = 128 * (int)S + 8;
    int thr = -lim;
    if (pq != kInvalid) {
        thr = lim;
        if (T != SCANN_KEY_MAX && scale > 0.0) {
            const double Tf = (double)ordered_to_f32((uint32_t)(T >> 32));
            const double qmax = floor((Tf * (1.0 + (double)S * 1.1920928955078125e-07) - bias_sum) / scale +
                                      0.5 * (double)S + 1.0) - 128.0 * (double)S;
            thr = qmax >= (double)lim ? lim : (qmax <= -(double)lim ? -lim : (int)qmax);
        }
    }
    return thr + 1;
}

// Three modes.  fold == 0 (dense prefilters): plain tables q - 128 and the pair's pass bound in thr1.  fold < 0 (K5d, ahead
// of any bound): the same plain tables and meta; pair_thr is not read and thr1 is not written.  fold > 0
// (adc_smfmac_kernel), the rest of this comment: the pass bound is folded INTO the tables, so that a point passes iff its integer sum
// is negative (the sparse MFMA accumulates in place: there is no free zero / bound operand, and the sign test is one
// vector instruction per result instead of two).  With qmax = the largest quantised sum a passing point can have (as
// in mfma_pass_bound), D = 128 S - 1 - qmax >= 0 is spread over the subspaces, d_s = D / S (+ 1 for the first D % S),
// and the entries are e = min(127, q - 128 + d_s): sum(q - 128 + d_s) = sum q - qmax - 1 < 0 <=> sum q <= qmax; the
// clamp at 127 only lowers sums (more points pass, never fewer) and d_s >= 0 means no entry is clamped from below.
// A bound with qmax > 128 S - 1 (more than half of the table range: a very loose filter) gets a coarser scale first,
// sc' = (T' - bias) / (127.5 S - 3): every entry still satisfies |v - (mn_s + sc' q)| <= sc' (0.5 + 1e-9), q <= 255.
// All-pass pairs (no bound, unquantisable table) store -128 everywhere, padding slots of a quad and bounds no point
// can meet store 127 (sums >= 0).
__global__ __launch_bounds__(256) void lut8_build_kernel(uint32_t S, const float *__restrict__ lutq,
                                                        const uint32_t *__restrict__ counters,
                                                        int8_t *__restrict__ lut8, Lut8Meta *__restrict__ meta,
                                                        const uint32_t *__restrict__ pair_q,
                                                        const uint64_t *__restrict__ pair_thr, int *__restrict__ thr1,
                                                        int fold) {
    __shared__ float s_min[4][64], s_rng[4][64];
    __shared__ double s_scale[4];
    __shared__ int s_bad[4], s_mode[4], s_dbase[4], s_drem[4];   // fold: 0 = quantise, 1 = all pass, 2 = none pass
    const uint32_t quad = blockIdx.x, tid = threadIdx.x;
    if (quad >= counters[CNT_TOTAL_QUADS]) return;
    const float4 *src = reinterpret_cast<const float4 *>(lutq) + (size_t)quad * S * 16;
    if (tid < 4) s_bad[tid] = 0;
    __syncthreads();
    const uint32_t p = tid & 3u, sub = tid >> 2;    // thread = (pair of the quad, subspace)
    float v[16];
    if (sub < S) {
        float mn = __builtin_inff(), mx = -__builtin_inff();
        bool bad = false;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const float4 e = src[sub * 16 + c];
            const float x = p == 0 ? e.x : p == 1 ? e.y : p == 2 ? e.z : e.w;
            v[c] = x;
            bad = bad || !(x >= 0.0f) || !(x < __builtin_inff());   // NaN, negative, infinite
            mn = fminf(mn, x);
            mx = fmaxf(mx, x);
        }
        s_min[p][sub] = mn;
        s_rng[p][sub] = mx - mn;
        if (bad) atomicOr(&s_bad[p], 1);
    }
    __syncthreads();
    if (tid < 4) {
        double bias = 0.0;
        float r = 0.0f;
        for (uint32_t j = 0; j < S; ++j) {
            bias += (double)s_min[tid][j];
            r = fmaxf(r, s_rng[tid][j]);
        }
        double sc = (s_bad[tid] || !(r > 0.0f)) ? 0.0 : (double)r / 255.0;
        const size_t slot = (size_t)quad * 4 + tid;
        if (fold > 0) {
            int mode = 1, dbase = 0, drem = 0;
            const uint64_t T = pair_thr[slot];
            if (pair_q[slot] == kInvalid) {
                mode = 2;
            } else if (T != SCANN_KEY_MAX && sc > 0.0) {
                const double Tf = (double)ordered_to_f32((uint32_t)(T >> 32));
                const double tq = Tf * (1.0 + (double)S * 1.1920928955078125e-07) - bias;
                const double lim = 128.0 * (double)S - 1.0;
                if (tq < 3.0e38) {   // (false for a NaN bound: everything passes)
                    double qmax = floor(tq / sc + 0.5 * (double)S + 1.0);
                    if (qmax > lim) {
                        const double sc2 = tq / (lim - 0.5 * (double)S - 2.0) * (1.0 + 1e-12);
                        sc = sc2 > sc ? sc2 : sc;
                        qmax = floor(tq / sc + 0.5 * (double)S + 1.0);
                    }
                    if (qmax < 0.0) {
                        mode = 2;
                    } else if (qmax <= lim) {
                        const int delta = (int)(lim - qmax);
                        mode = 0;
                        dbase = delta / (int)S;
                        drem = delta % (int)S;
                    }
                }
            }
            s_mode[tid] = mode;
            s_dbase[tid] = dbase;
            s_drem[tid] = drem;
            thr1[slot] = 0;
        } else if (fold == 0) {
            // (the pair's pass bound right away: the filter bounds are known by now -- one launch less)
            thr1[slot] = mfma_pass_bound(S, pair_q[slot], pair_thr[slot], bias, sc);
        }
        // (fold < 0: nothing here -- the plain tables ahead of any bound; pair_thr and thr1 are not touched)
        s_scale[tid] = sc;
        Lut8Meta m;
        m.bias_sum = bias;
        m.scale = sc;
        meta[slot] = m;
    }
    __syncthreads();
    if (sub < S) {
        const double sc = s_scale[p], mn = (double)s_min[p][sub];
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            int q = 0;
            if (sc > 0.0) {
                const double t = ((double)v[c] - mn) / sc;
                q = (int)floor(t + 0.5);
                q = q < 0 ? 0 : (q > 255 ? 255 : q);
            }
            int e = q - 128;
            if (fold > 0) {
                const int mode = s_mode[p];
                e += s_dbase[p] + ((int)sub < s_drem[p] ? 1 : 0);
                e = mode == 1 ? -128 : mode == 2 ? 127 : (e > 127 ? 127 : e);
            }
            w[c >> 2] |= (uint32_t)(e & 0xFF) << (8 * (c & 3));
        }
        *reinterpret_cast<uint4 *>(lut8 + (((size_t)quad * 4 + p) * S + sub) * 16) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

struct MfmaArgs {
    const int *thr1;          // [slots] pass bound + 1 (lut8_build_kernel)
    const uint32_t *pair_off, *tile_off, *pair_q, *pair_vbase;
    uint32_t *counters;
    const int8_t *lut8;
    const Lut8Meta *meta;
    const uint64_t *pair_thr;
    uint32_t *cand32_cnt;     // [nq]
    uint32_t *cand32;         // [nq][cap32] stream positions of the prefilter's survivors
    uint32_t *cand32_codes;   // [nq][cap32][S/8] their packed codes: the refine reads them in list order
    uint32_t cap32;
    const uint64_t *allow;    // the search's allow-bitmap (or nullptr): disallowed survivors never enter the lists,
    uint64_t allow_bits;      // so that the filter bounds them as it bounds the gather scan's (cap32 assumes it)
    uint32_t *surv;           // [nq rounded up to 64][surv_stride] survivor bitmaps (adc_smfmac_bits_kernel64), else unused
    uint32_t surv_stride;     // words per query: ranges of kSpRange64 points x 32
};

// The survivor mask `m` of a prefilter tile without its disallowed points: bit b of m stands for the point at leaf
// position pos_of(b) (CSR row lb + pos_of(b)).  Walks the set bits only (a few per tile); callers take this branch
// only when a bitmap is present, so an unfiltered scan runs none of it.  q: the query the mask belongs to (the lane's
// pair); its bitmap's address is formed once, here.
template <typename F>
__device__ __forceinline__ uint32_t mask_allowed(const TxhIndexDev &ix, const uint64_t *allow, uint64_t stride, uint32_t q,
                                                 uint64_t allow_bits, uint32_t lb, uint32_t m, F pos_of) {
    allow = query_allow(allow, stride, q);
    uint32_t keep = 0;
    while (m) {
        const uint32_t b = (uint32_t)__ffs((int)m) - 1u;
        m &= m - 1u;
        if (row_allowed(ix, allow, 0, 0, allow_bits, lb + pos_of(b))) keep |= 1u << b;
    }
    return keep;
}

// Appends one prefilter survivor to query q's list: slot `dst` takes the stream position `pos` and, where the list
// carries packed codes (cand32_codes: wave-uniform), the point's code words, read from its row `codes` of ix.codes.  A
// slot past cap32 is dropped: the query's count still passes cap32, and adc_refine_kernel reports the overflow.
template <int S>
__device__ __forceinline__ void append_survivor(uint32_t *cand32, uint32_t *cand32_codes, uint32_t cap32, uint32_t q,
                                                uint32_t dst, uint32_t pos, const uint32_t *codes) {
    constexpr int NW = Codec<S, 4>::NWORDS;
    if (dst < cap32) {
        const size_t o = (size_t)q * cap32 + dst;
        cand32[o] = pos;
        if (cand32_codes) {
            uint32_t cw[NW];
            Codec<S, 4>::load_words(codes, cw);
            Codec<S, 4>::store_words(cand32_codes + o * NW, cw);
        }
    }
}
// (The copy-outs of sp_flush_item_lanes / sp_flush_item_words write the same record from code words they loaded ahead,
// kSpU points at a time, in the plane form of ix.codes_sp; they keep their own lines: through a shared helper
// adc_smfmac_kernel<48, false> spilled two more VGPRs.)

template <int S_>
__device__ __forceinline__ void adc_mfma_body(TxhIndexDev ix, MfmaArgs a, const uint64_t allow_stride) {
    typedef int v4i __attribute__((ext_vector_type(4)));
    typedef int v16i __attribute__((ext_vector_type(16)));
    constexpr int S = S_, KS = S / 2, NW = S / 8;
    __shared__ __attribute__((aligned(16))) uint32_t s_ident[64];                 // 16 one-hot rows of 16 bytes
    __shared__ uint32_t s_stage[kMfmaWaves][32][kMfmaStage];
    __shared__ uint32_t s_cnt[kMfmaWaves][32];
    __shared__ uint32_t s_fpre[kMfmaWaves][32], s_fq[kMfmaWaves][32], s_fgb[kMfmaWaves][32], s_fvb[kMfmaWaves][32];   // flush: per pair
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t col = lane & 31u, h = lane >> 5;
    // row c (16 bytes = words 4c .. 4c+3): byte c set to 1  ->  word 4c + (c >> 2) holds 1 << 8*(c & 3)
    if (tid < 64) {
        const uint32_t c = tid >> 2, wsel = tid & 3u;
        s_ident[tid] = (wsel == (c >> 2)) ? (1u << (8 * (c & 3u))) : 0u;
    }
    __syncthreads();
    const uint32_t total_tiles = a.counters[CNT_TOTAL_TILES];
    const char *ident = reinterpret_cast<const char *>(s_ident);

    uint32_t tile = 0;
    if (lane == 0) tile = grab_tile(a.counters + CNT_XQ, total_tiles);
    tile = __builtin_amdgcn_readfirstlane(tile);
    while (tile != kInvalid) {
        // the next item's queue atomic travels while this item is computed
        uint32_t next_tile = 0;
        if (lane == 0) next_tile = grab_tile(a.counters + CNT_XQ, total_tiles);
        const WorkItem item = decode_item(ix, a.tile_off, a.pair_off, tile);
        const uint32_t lb = item.lb, size = item.size, local = item.local, slot0 = item.slot0, slot_end = item.slot_end;
        const uint32_t nranges = (size + kMfmaRange - 1) / kMfmaRange;
        const uint32_t range = local % nranges, pt = local / nranges;
        const uint32_t c0 = range * kMfmaRange;
        const uint32_t npts = min(kMfmaRange, size - c0);

        // this lane's pair (column): tables, bound, key base
        const uint32_t slot = slot0 + pt * 32u + col;
        const bool pair_ok = slot < slot_end;
        const uint32_t pq = pair_ok ? a.pair_q[slot] : kInvalid;
        const uint32_t vb = pair_ok ? a.pair_vbase[slot] : 0u;
        v4i b[KS];
        {
            const int8_t *bsrc = a.lut8 + ((size_t)(pair_ok ? slot : slot0) * S + h) * 16;   // padding columns: any table
#pragma unroll
            for (int t = 0; t < KS; ++t) b[t] = *reinterpret_cast<const v4i *>(bsrc + (size_t)t * 32);
        }
        const int thr1 = pair_ok ? a.thr1[slot] : -(128 * S + 7);   // a point passes iff acc - thr1 < 0
        if (lane < 32) s_cnt[wave][lane] = 0;
        // (s_cnt / s_stage are private to the wave: no workgroup barrier anywhere in this loop)

        const uint32_t ntile = (npts + 31u) >> 5;
        uint32_t wn[NW];
        {
            const uint32_t j = c0 + col;
            Codec<S, 4>::load_words(ix.codes + (size_t)(lb + (j < size ? j : 0u)) * NW, wn);
        }
        // Software pipeline over the item's tiles, two accumulators: step(t) issues the MFMA chain of tile
        // t and, between its MFMAs (their shadow hides ~6 vector instructions each), builds the survivor
        // mask of tile t - 1 from the other accumulator; then the (rare, branchy) survivor staging of
        // tile t - 1.  One extra step drains the last tile (its MFMAs run on stale codes and are dropped).
        // Staged survivors -> the queries' lists: ONE returning atomic per flushed pair (all of them in one
        // wave instruction), then one contiguous segment per pair.  all = false flushes only the pairs
        // whose stage could overflow in the next tile (a tile adds at most 32 per pair): dense pairs --
        // the nearest leaves of a query, where a large share of the points pass -- flush often, sparse
        // ones once per item.
        auto flush = [&](bool all) {
            uint32_t n = 0, gbase = 0;
            if (lane < 32) {
                n = min(s_cnt[wave][lane], kMfmaStage);
                if (!all && n + 32u <= kMfmaStage) n = 0;
                if (n) {
                    gbase = atomicAdd(&a.cand32_cnt[pq], n);
                    s_cnt[wave][lane] = 0;
                }
            }
            // all flushed pairs as ONE list spread over the 64 lanes: entry e belongs to the pair c with
            // pre[c] <= e < pre[c] + n[c]; its position and its packed codes (the tile's lines are still in
            // L2) go to slot gbase[c] + (e - pre[c]) of the query's list
            uint32_t incl = n;
#pragma unroll
            for (int o = 1; o < 32; o <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
                if ((int)lane >= o) incl += up;
            }
            const uint32_t total = (uint32_t)__shfl((int)incl, 31);
            if (total == 0) return;
            if (lane < 32) {
                s_fpre[wave][lane] = incl - n;
                s_fq[wave][lane] = pq == kInvalid ? 0u : pq;
                s_fgb[wave][lane] = gbase;
                s_fvb[wave][lane] = vb;
            }
            // (per-pair values through LDS, not shuffles: the loop's last pass runs with lanes switched off)
            for (uint32_t e = lane; e < total; e += 64u) {
                uint32_t c = 0;
#pragma unroll
                for (uint32_t stp = 16; stp; stp >>= 1)
                    if (s_fpre[wave][c + stp] <= e) c += stp;
                const uint32_t idx = e - s_fpre[wave][c];
                const uint32_t j = s_stage[wave][c][idx];
                const uint32_t dst = s_fgb[wave][c] + idx;
                append_survivor<S>(a.cand32, a.cand32_codes, a.cap32, s_fq[wave][c], dst, s_fvb[wave][c] + j, ix.codes + (size_t)(lb + j) * NW);
            }
        };
        auto step = [&](v16i &accN, const v16i &accO, uint32_t t) {
            // nibbles of this lane's subspace parity h, pre-shifted to byte offsets code * 16
            uint32_t rg[NW];
#pragma unroll
            for (int wi = 0; wi < NW; ++wi) rg[wi] = h ? (wn[wi] & 0xF0F0F0F0u) : ((wn[wi] & 0x0F0F0F0Fu) << 4);
            if (t + 1 < ntile) {
                const uint32_t j = c0 + (t + 1) * 32u + col;
                Codec<S, 4>::load_words(ix.codes + (size_t)(lb + (j < size ? j : 0u)) * NW, wn);
            }
            accN = v16i{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            // A fragments: kMfmaDepth one-hot rows in flight ahead of the MFMA that consumes them
            constexpr int D = kMfmaDepth < KS ? kMfmaDepth : KS;
            v4i av[D + 1];
            auto onehot = [&](int kt) {
                const uint32_t off = (rg[kt >> 2] >> (8 * (kt & 3))) & 0xFFu;   // code * 16 of subspace 2 kt + h
                return *reinterpret_cast<const v4i *>(ident + off);
            };
#pragma unroll
            for (int kt = 0; kt < D; ++kt) av[kt] = onehot(kt);
            // lane (col, h), register r: point row (r & 3) + 8 * (r >> 2) + 4 * h of the tile.  Survivor
            // bits of the lane's 16 results without a branch per result (a tile holds ~10 survivors among
            // 1024 results): v_sub + v_alignbit shift the sign of acc - thr1 into the mask, so result r
            // ends up at bit 15 - r.
            uint32_t m16 = 0;
            // the MFMA chain issues ahead of the other waves' staging / flush streams (s_setprio: -2 % kernel time)
            __builtin_amdgcn_s_setprio(2);
#pragma unroll
            for (int kt = 0; kt < KS; ++kt) {
                if (kt + D < KS) av[(kt + D) % (D + 1)] = onehot(kt + D);
                accN = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[kt % (D + 1)], b[kt], accN, 0, 0, 0);
#pragma unroll
                for (int r = kt * 16 / KS; r < (kt + 1) * 16 / KS; ++r)
                    m16 = __builtin_amdgcn_alignbit(m16, (uint32_t)(accO[r] - thr1), 31);
                __builtin_amdgcn_sched_barrier(0);
            }
            __builtin_amdgcn_s_setprio(0);
            if (t == 0) return;                // nothing before the first tile (wave-uniform)
            const uint32_t base = c0 + (t - 1) * 32u + 4u * h;
            if (t == ntile && (npts & 31u)) {  // partial last tile: rows past the leaf's end are padding
                uint32_t okm = 0;
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    okm |= (base + (uint32_t)((r & 3) + 8 * (r >> 2)) < size ? 1u : 0u) << (15 - r);
                m16 &= okm;
            }
            if (a.allow && m16)                // search_with_filter: disallowed points are not survivors
                m16 = mask_allowed(ix, a.allow, allow_stride, pq, a.allow_bits, lb, m16, [&](uint32_t b) {
                    const uint32_t r = 15u - b;
                    return base + (r & 3u) + ((r >> 2) << 3);
                });
            bool risk = false;                 // this lane's pair could overflow its stage in the next tile
            if (m16) {
                uint32_t sl = atomicAdd(&s_cnt[wave][col], (uint32_t)__popc(m16));   // one LDS atomic per lane
                do {
                    const uint32_t r = 15u - ((uint32_t)__ffs((int)m16) - 1u);
                    m16 &= m16 - 1u;
                    const uint32_t j = base + (r & 3u) + ((r >> 2) << 3);
                    if (sl < kMfmaStage) {
                        s_stage[wave][col][sl] = j;
                    } else {   // stage full: direct (slow) append
                        const uint32_t pos = atomicAdd(&a.cand32_cnt[pq], 1u);
                        append_survivor<S>(a.cand32, a.cand32_codes, a.cap32, pq, pos, vb + j, ix.codes + (size_t)(lb + j) * NW);
                    }
                    ++sl;
                } while (m16);
                risk = sl + 32u > kMfmaStage;   // (the lane that appended last to a pair saw its full count)
            }
            if (__any(risk)) flush(false);
        };
        // (tile 0 is peeled: inside the loop t >= 1 is known, so the compiler keeps the mask build between
        // the MFMAs in BOTH instances instead of sinking it below a `t == 0` branch)
        v16i accA = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, accB = accA;
        step(accA, accB, 0u);
        for (uint32_t tl = 1; tl <= ntile; tl += 2) {
            step(accB, accA, tl);
            if (tl + 1 <= ntile) step(accA, accB, tl + 1);
        }
        flush(true);
        tile = __builtin_amdgcn_readfirstlane(next_tile);
    }
}
// One bitmap for the batch, or none: the kernel every search without allow_bitmap_stride runs (its code is that of the
// body with the stride folded to 0).  _pq: one bitmap per query, allow_stride words apart.
template <int S_>
__global__ __launch_bounds__(kMfmaWaves * 64, (S_ <= 32 ? SCANN_MFMA_MINW : 2)) void adc_mfma_kernel(TxhIndexDev ix, MfmaArgs a) {
    adc_mfma_body<S_>(ix, a, 0);
}
template <int S_>
__global__ __launch_bounds__(kMfmaWaves * 64, (S_ <= 32 ? SCANN_MFMA_MINW : 2)) void adc_mfma_pq_kernel(TxhIndexDev ix, MfmaArgs a, uint64_t allow_stride) {
    adc_mfma_body<S_>(ix, a, allow_stride);
}

// =====================================================================================
// K6e: the 32-pair prefilter on the 2:4 STRUCTURED-SPARSE MFMA (v_smfmac_i32_32x32x64_i8).
//
// A one-hot row has one non-zero per 16 K-elements, so it satisfies 2:4 sparsity by construction: the
// sparse instruction multiplies a COMPRESSED A (two values per group of four K-elements + a 2-bit position
// each) with a dense 64-deep B in the time the dense instruction takes for K = 32 -- four subspaces per MFMA
// slot instead of two (tools/micro/smfmac_probe.hip: 21.5-26 ns against 19.4-25 ns per instruction per SIMD).
// Operand layout (probed on the hardware, same tool): A lane (m, ha) holds row m; its compressed byte b (value slot
// b & 1 of group (b >> 1) & 3 of half b >> 3) with position i multiplies B lane (n, hb = b >> 3), byte 16 ha + 4
// ((b >> 1) & 3) + i; the selection is a plain mux (equal or descending positions of a group's two values work).
// Sparse MFMA kt therefore covers subspaces s0 .. s0 + 3 (s0 = 4 + 4 kt): B lane (n, hb) = the 32 table bytes of
// subspaces s0 + 2 hb, s0 + 2 hb + 1 of pair n (contiguous in lut8), A lane (m, ha) = the codes ca = code[s0 + ha]
// (bytes 0..7) and cb = code[s0 + 2 + ha] (bytes 8..15) of point m: value 1 at byte 2 (ca >> 2) / 8 + 2 (cb >> 2),
// positions (ca & 3) / (cb & 3) replicated over the half's four groups (the other groups hold zeros).
//
// The sparse instruction accumulates in place (no C operand), so a tile starts with two DENSE MFMAs (subspaces 0..3,
// C = the inline constant 0: no accumulator clearing on the vector pipe) followed by (S - 4) / 4 sparse ones: 9 MFMA
// slots per 32 x 32 tile at S = 32 instead of 16.  Both A operands come from 16-row LDS tables (conflict-free
// ds_read_b128 / ds_read_b32: lanes with equal rows broadcast); their row numbers are precomputed per point at index
// creation as two nibble PLANES (codes_sp: V = (ca >> 2) | (cb >> 2) << 2 picks the value row, N = (ca & 3) |
// (cb & 3) << 2 the position word; the last nibble of each plane is the raw code of dense MFMA 0 / 1), so a tile
// costs 7 unpack instructions + 2 byte extractions per sparse MFMA.  The pass bound lives in the tables
// (lut8_build_kernel, fold): a point passes iff its sum is negative -- one v_alignbit per result.
// Items, survivor staging, flush and lists as in adc_mfma_kernel; candidate lists identical (the refine is exact).
// =====================================================================================
#ifndef SCANN_SP_STAGE
#define SCANN_SP_STAGE 512
#endif
constexpr uint32_t kSpStage = SCANN_SP_STAGE;   // adc_smfmac_kernel: list entries staged per flush round (per wave)
#ifndef SCANN_SP_U
#define SCANN_SP_U 8
#endif
constexpr uint32_t kSpU = SCANN_SP_U;         // ... and code rows in flight per lane in the copy phase
#ifndef SCANN_SP_STAGE64
#define SCANN_SP_STAGE64 1024   // (two workgroups per CU: 69 KB each; an item's ~800 entries at C3 in one round)
#endif

// Shape of a wave's item by its column tiles: CT = 1, 32 (query, leaf) pairs x kMfmaRange points; CT = 2, 64 pairs x
// kSpRange64 points -- the same MFMAs per item, and with half the points the same 32 bitmap words per lane.
template <int CT>
struct SpItem {
    static constexpr uint32_t RANGE = CT == 2 ? kSpRange64 : kMfmaRange;      // points
    static constexpr uint32_t STAGE = CT == 2 ? SCANN_SP_STAGE64 : kSpStage;   // list entries staged per flush round
    static constexpr int TTM = (int)(RANGE / 64);                              // tile pairs (bitmap words per lane and column tile)
};

template <int S_>
struct SpLayout {
    static constexpr int NS = (S_ - 4) / 4;      // sparse MFMAs per tile
    static constexpr int NIB = NS + 1;           // nibbles per plane (the last one: a dense MFMA's raw code)
    static constexpr int NWP = (NIB + 7) / 8;    // words per plane
    static constexpr int SPW = 4 * NWP;          // words per point: [ha][plane V, N][word]
};

__global__ __launch_bounds__(256) void codes_sp_build_kernel(const uint32_t *__restrict__ codes, uint64_t n, uint32_t S,
                                                            uint32_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t nw = S / 8, ns = (S - 4) / 4, nwp = (ns + 1 + 7) / 8;
    const uint32_t *w = codes + i * nw;
    auto code = [&](uint32_t sub) { return (w[sub >> 3] >> (4 * (sub & 7u))) & 15u; };
    uint32_t *o = out + i * 4 * nwp;
    for (uint32_t ha = 0; ha < 2; ++ha)
        for (uint32_t wi = 0; wi < nwp; ++wi) {
            uint32_t v = 0, nn = 0;
            for (uint32_t j = 8 * wi; j < 8 * wi + 8 && j <= ns; ++j) {
                uint32_t vn, nb;
                if (j < ns) {
                    const uint32_t ca = code(4 + 4 * j + ha), cb = code(4 + 4 * j + 2 + ha);
                    vn = (ca >> 2) | ((cb >> 2) << 2);
                    nb = (ca & 3u) | ((cb & 3u) << 2);
                } else {   // dense MFMA 0 scores subspace ha, dense MFMA 1 subspace 2 + ha
                    vn = code(ha);
                    nb = code(2 + ha);
                }
                v |= vn << (4 * (j & 7u));
                nn |= nb << (4 * (j & 7u));
            }
            o[(ha * 2 + 0) * nwp + wi] = v;
            o[(ha * 2 + 1) * nwp + wi] = nn;
        }
}

// inclusive prefix sum over the 64 lanes of a wave: DPP row shifts inside the 16-lane rows, then the row broadcasts
// (six v_add with a DPP operand; no LDS round trips)
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);   // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);   // row_bcast:15 into rows 1, 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);   // row_bcast:31 into rows 2, 3
    return v;
}

// search_with_filter in the sparse prefilter: lane (col, h) drops the disallowed points from its own words of the item's
// survivor bitmap (words[tt * 64], tt < ntt; see adc_smfmac_body: word [tt][h][col] = the masks of tiles 2 tt (low half)
// and 2 tt + 1, result r of a tile -- point row (r & 3) + 8 (r >> 2) + 4 h -- at bit 15 - r), before the flush counts
// them.  pq: the query of the lane's pair (padding pairs have no bits, so their query is never used).  Called at the top
// of the flushes, where the tile loop's registers are dead, and only when a bitmap is present.
__device__ __forceinline__ void sp_filter_words(const TxhIndexDev &ix, const uint64_t *allow, uint64_t stride, uint32_t pq,
                                                uint64_t allow_bits, uint32_t *words, uint32_t ntt, uint32_t c0, uint32_t lb, uint32_t h) {
    for (uint32_t tt = 0; tt < ntt; ++tt) {
        const uint32_t wd = words[tt * 64u];
        if (wd)
            words[tt * 64u] = mask_allowed(ix, allow, stride, pq, allow_bits, lb, wd, [&](uint32_t b) {
                const uint32_t r = 15u - (b & 15u);
                return c0 + (2u * tt + (b >> 4)) * 32u + 4u * h + (r & 3u) + ((r >> 2) << 3);
            });
    }
    __builtin_amdgcn_wave_barrier();   // (the word-parallel flush reads the other lanes' words)
}

#ifndef SCANN_SP_FLUSH_INLINE
#define SCANN_SP_FLUSH_INLINE __forceinline__
#endif
// The flush for FLAT hashers (one leaf, every pair sparse: ~0.4 survivors per bitmap word at C3): lane (col, h) keeps
// its own 32 words in registers and walks their bits itself, in rounds of kSpStage staged entries; the copy-out is the
// same as in sp_flush_item_words.  No per-pair round trip through LDS and the wave scan: 0.35 ms at C3 against
// 0.44 ms for the word-parallel form -- which wins wherever pairs are dense (tree indexes: 10M x 128, P = 25, m = 1000:
// scan 0.27 ms against 0.71 ms), because a lane walking its own survivors takes them one by one.
// CT = 2 (64 pairs): lane (col, h) owns pair col of both column tiles, words [ct][tt] of the bitmap; the pairs are
// numbered ct * 32 + col in the prefix, the stage entries and the s_fq / s_fvb / s_fgb rows, and lane (col, h) issues
// the atomic of pair h * 32 + col (one returning atomic per live pair, all 64 in one instruction).
template <int S, int CT>
__device__ SCANN_SP_FLUSH_INLINE void sp_flush_item_lanes(const uint32_t *__restrict__ codes_sp, const TxhIndexDev &ix,
                                                        const uint64_t *allow, uint64_t allow_bits, uint64_t allow_stride, uint32_t *__restrict__ cand32_cnt,
                                                        uint32_t *__restrict__ cand32, uint32_t *__restrict__ cand32_codes,
                                                        uint32_t cap32, uint32_t *bits, uint2 *stage, uint32_t *s_fq,
                                                        uint32_t *s_fvb, uint32_t *s_fgb, uint32_t ntile, uint32_t c0,
                                                        uint32_t lb, const uint32_t (&pq)[CT], const uint32_t (&vb)[CT]) {
    constexpr int SPW = SpLayout<S>::SPW;
    constexpr int TTM = SpItem<CT>::TTM;
    constexpr uint32_t STAGE = SpItem<CT>::STAGE;
    uint32_t lane = threadIdx.x & 63u;
    // (CT = 2, opaque per item: the optimiser otherwise forms the walk's 32 per-word entry bases once per kernel and
    // keeps them across the tile loop, whose two table sets leave no room -- they went to scratch memory)
    if constexpr (CT == 2) asm volatile("" : "+v"(lane));
    const uint32_t col = lane & 31u, h = lane >> 5;
    const uint32_t ntt = (ntile + 1u) >> 1;
    if (allow) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) sp_filter_words(ix, allow, allow_stride, pq[ct], allow_bits, bits + ct * TTM * 64, ntt, c0, lb, h);
    }
    // CT = 1: the lane's words stay in registers and are walked one after the other.  CT = 2: only a mask `nz` of its
    // non-empty words does, and the walk pops the words off it (below).
    constexpr bool MASKED = CT == 2;
    static_assert(!MASKED || CT * TTM <= 32, "one mask bit per bitmap word of the lane");
    uint32_t w[MASKED ? 1 : CT][MASKED ? 1 : TTM];
    uint32_t nz = 0;
    uint32_t cnt[CT], other[CT], n_pair[CT], incl[CT];
    uint32_t total = 0;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        cnt[ct] = 0;
#pragma unroll
        for (int tt = 0; tt < TTM; ++tt) {
            const uint32_t x = (uint32_t)tt < ntt ? bits[(ct * TTM + tt) * 64] : 0u;
            if constexpr (MASKED) nz |= x ? 1u << (ct * TTM + tt) : 0u;
            else w[ct][tt] = x;
            cnt[ct] += (uint32_t)__popc(x);
        }
        other[ct] = (uint32_t)__shfl_xor((int)cnt[ct], 32);
        n_pair[ct] = cnt[ct] + other[ct];
        incl[ct] = n_pair[ct];   // prefix over the pairs, computed alike in both halves of the wave
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl[ct], o, 32);
            if ((int)col >= o) incl[ct] += up;
        }
        incl[ct] += total;       // (the column tiles one after the other)
        total = (uint32_t)__shfl((int)incl[ct], 31, 32);
    }
    if (total == 0) return;
    // the pair this lane speaks for in the per-pair rows: col (lanes 0..31); CT = 2: pair lane
    const bool second = CT == 2 && h;
    const uint32_t my_n = second ? n_pair[CT - 1] : n_pair[0], my_q = second ? pq[CT - 1] : pq[0];
    const bool speaks = CT == 2 || h == 0;
    uint32_t gbase = 0;
    if (speaks && my_n) gbase = atomicAdd(&cand32_cnt[my_q], my_n);   // (padding pairs have no bits)
    if (speaks) {
        s_fq[lane] = my_q == kInvalid ? 0u : my_q;
        s_fvb[lane] = second ? vb[CT - 1] : vb[0];
    }
    uint32_t sq[CT], rel[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        sq[ct] = incl[ct] - n_pair[ct] + (h ? other[ct] : 0u);   // this lane's first entry in the wave's staging order
        rel[ct] = h ? other[ct] : 0u;                            // ... and its position in the pair's segment
    }
    // MASKED walk: (wcur, wi) = what is left of the word being walked and its number ct * TTM + tt, (sqc, relc) = the
    // entry counters of its column tile; all of them carry over from round to round.
    uint32_t wcur = 0, wi = 0, ctc = 0, sqc = sq[0], relc = rel[0];
    for (uint32_t base = 0; base < total; base += STAGE) {
        const uint32_t lim = base + STAGE;
        if constexpr (MASKED) {
            // One loop over the lane's set bits, whichever word they are in: a wave takes as many trips as its fullest
            // lane has survivors (~20 at 0.4 survivors per word), where the loop per word of the CT = 1 form takes as
            // many as the fullest lane of EVERY word (~2.5 x 32).  The words come back from LDS one at a time (a
            // lane's own column: conflict-free); a lane's entries of column tile 0 precede those of tile 1 in the
            // staging order as its words do in the mask, so a round ends for it at the first entry past the stage.
            for (;;) {
                if (wcur == 0) {
                    if (nz == 0) break;
                    wi = (uint32_t)__ffs((int)nz) - 1u;
                    nz &= nz - 1u;
                    wcur = bits[wi * 64u];
                    if (wi >= (uint32_t)TTM && ctc == 0) {   // the lane's first word of column tile 1
                        ctc = 1;
                        sqc = sq[CT - 1];
                        relc = rel[CT - 1];
                    }
                }
                if (sqc >= lim) break;
                const uint32_t bpos = (uint32_t)__ffs((int)wcur) - 1u;
                wcur &= wcur - 1u;
                const uint32_t r = 15u - (bpos & 15u);
                const uint32_t jrel = (2u * (wi - ctc * (uint32_t)TTM) + (bpos >> 4)) * 32u + 4u * h + (r & 3u) + ((r >> 2) << 3);
                stage[sqc - base] = make_uint2(relc, ((ctc * 32u + col) << 16) | jrel);
                ++sqc;
                ++relc;
            }
        } else {
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
                for (int tt = 0; tt < TTM; ++tt) {
                    while (w[ct][tt] && sq[ct] < lim) {
                        const uint32_t bpos = (uint32_t)__ffs((int)w[ct][tt]) - 1u;
                        w[ct][tt] &= w[ct][tt] - 1u;
                        const uint32_t r = 15u - (bpos & 15u);
                        const uint32_t jrel = (2u * (uint32_t)tt + (bpos >> 4)) * 32u + 4u * h + (r & 3u) + ((r >> 2) << 3);
                        stage[sq[ct] - base] = make_uint2(rel[ct], (((uint32_t)ct * 32u + col) << 16) | jrel);
                        ++sq[ct];
                        ++rel[ct];
                    }
                }
            }
        }
        if (base == 0 && speaks) s_fgb[lane] = gbase;   // (the atomics have travelled under the walk)
        __builtin_amdgcn_wave_barrier();
        const uint32_t n = min(STAGE, total - base);
        for (uint32_t e0 = 0; e0 < n; e0 += 64u * kSpU) {
            uint2 ent[kSpU];
            uint4 cw[kSpU][SPW / 4];
#pragma unroll
            for (int u = 0; u < (int)kSpU; ++u) {
                const uint32_t e = e0 + lane + 64u * (uint32_t)u;
                ent[u] = e < n ? stage[e] : make_uint2(0xFFFFFFFFu, 0u);
            }
            if (cand32_codes) {   // (wave-uniform)
#pragma unroll
                for (int u = 0; u < (int)kSpU; ++u)
#pragma unroll
                    for (int x = 0; x < SPW / 4; ++x)
                        cw[u][x] = reinterpret_cast<const uint4 *>(codes_sp + (size_t)(lb + c0 + (ent[u].y & 0xFFFFu)) * SPW)[x];
            } else {   // (defined on every path: a conditionally initialised array stays in scratch memory -- 16 scratch
                       // round trips per copy-out, 0.41 instead of 0.35 ms at C3)
#pragma unroll
                for (int u = 0; u < (int)kSpU; ++u)
#pragma unroll
                    for (int x = 0; x < SPW / 4; ++x) cw[u][x] = make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (int u = 0; u < (int)kSpU; ++u) {
                if (ent[u].x != 0xFFFFFFFFu) {
                    const uint32_t c = ent[u].y >> 16;
                    const uint32_t dst = s_fgb[c] + ent[u].x;
                    if (dst < cap32) {
                        const size_t o = (size_t)s_fq[c] * cap32 + dst;
                        cand32[o] = s_fvb[c] + c0 + (ent[u].y & 0xFFFFu);
                        if (cand32_codes) {
#pragma unroll
                            for (int x = 0; x < SPW / 4; ++x) reinterpret_cast<uint4 *>(cand32_codes + o * SPW)[x] = cw[u][x];
                        }
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// The flush of adc_smfmac_kernel: the item's survivor bitmap -> the queries' lists.  The tile loop left word
// [tt][h][col] = the masks of tiles 2 tt, 2 tt + 1 of lane (col, h).
//   1. every lane counts the bits of its own words; the two lanes of a pair share ONE returning atomic for the pair's
//      segment of the query's list (issued now, consumed in step 3);
//   2. pair by pair, the 64 lanes take the pair's 64 words ONE WORD EACH: a DPP prefix sum gives every word its offset
//      in the segment, and each lane stages (offset, pair, point) of its word's bits in LDS.  A pair whose every point
//      passes (a query's nearest leaf in a tree index) costs 32 rounds here, not the 2048 a lane walking its own
//      survivors one by one would need; a sparse pair (0.2 bits per word on a flat 1M index) costs two;
//   3. whenever the stage is full (kSpStage entries) or the pairs are done, the 64 lanes copy the staged entries to the
//      lists side by side, each with up to kSpU row loads in flight.  What travels with a position (flat hashers) is
//      the point's PLANE row (codes_sp: the lines the tile loop has just read, still in L2 -- the packed codes were
//      last touched at index creation); adc_refine_kernel decodes it (RefineArgs::planes).
template <int S>
__device__ SCANN_SP_FLUSH_INLINE void sp_flush_item_words(const uint32_t *__restrict__ codes_sp, const TxhIndexDev &ix,
                                                        const uint64_t *allow, uint64_t allow_bits, uint64_t allow_stride, uint32_t *__restrict__ cand32_cnt,
                                                        uint32_t *__restrict__ cand32, uint32_t *__restrict__ cand32_codes,
                                                        uint32_t cap32, uint32_t *bits_w, uint2 *stage, uint32_t *s_fq,
                                                        uint32_t *s_fvb, uint32_t *s_fgb, uint32_t ntile, uint32_t c0,
                                                        uint32_t lb, uint32_t pq, uint32_t vb) {
    constexpr int SPW = SpLayout<S>::SPW;
    constexpr int TTM = (int)(kMfmaRange / 64);
    static_assert(TTM == 32, "the flush maps the 64 words of a pair onto the 64 lanes");
    const uint32_t lane = threadIdx.x & 63u, h = lane >> 5;
    const uint32_t ntt = (ntile + 1u) >> 1;
    if (allow) sp_filter_words(ix, allow, allow_stride, pq, allow_bits, bits_w + lane, ntt, c0, lb, h);
    uint32_t cnt = 0;
#pragma unroll
    for (int tt = 0; tt < TTM; ++tt) cnt += (uint32_t)tt < ntt ? (uint32_t)__popc(bits_w[tt * 64 + lane]) : 0u;
    const uint32_t n_pair = cnt + (uint32_t)__shfl_xor((int)cnt, 32);   // (the same in both lanes of a pair)
    if (!__any(n_pair != 0)) return;
    uint32_t gbase = 0;
    if (h == 0 && n_pair) gbase = atomicAdd(&cand32_cnt[pq], n_pair);   // (padding pairs have no bits)
    if (lane < 32) {
        s_fq[lane] = pq == kInvalid ? 0u : pq;
        s_fvb[lane] = vb;
    }
    bool fgb_done = false;
    // step 3: stage[0 .. n) -> the lists
    auto copy_out = [&](uint32_t n) {
        if (!fgb_done) {   // (wave-uniform; the atomics have travelled under the first pairs' staging)
            if (lane < 32) s_fgb[lane] = gbase;
            fgb_done = true;
        }
        __builtin_amdgcn_wave_barrier();
        for (uint32_t e0 = 0; e0 < n; e0 += 64u * kSpU) {
            uint2 ent[kSpU];
            uint4 cw[kSpU][SPW / 4];
#pragma unroll
            for (int u = 0; u < (int)kSpU; ++u) {
                const uint32_t e = e0 + lane + 64u * (uint32_t)u;
                ent[u] = e < n ? stage[e] : make_uint2(0xFFFFFFFFu, 0u);
            }
            if (cand32_codes) {   // (wave-uniform)
#pragma unroll
                for (int u = 0; u < (int)kSpU; ++u)
#pragma unroll
                    for (int x = 0; x < SPW / 4; ++x)
                        cw[u][x] = reinterpret_cast<const uint4 *>(codes_sp + (size_t)(lb + c0 + (ent[u].y & 0xFFFFu)) * SPW)[x];
            } else {   // (defined on every path: a conditionally initialised array stays in scratch memory -- 16 scratch
                       // round trips per copy-out, 0.41 instead of 0.35 ms at C3)
#pragma unroll
                for (int u = 0; u < (int)kSpU; ++u)
#pragma unroll
                    for (int x = 0; x < SPW / 4; ++x) cw[u][x] = make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (int u = 0; u < (int)kSpU; ++u) {
                if (ent[u].x != 0xFFFFFFFFu) {
                    const uint32_t c = ent[u].y >> 16;
                    const uint32_t dst = s_fgb[c] + ent[u].x;
                    if (dst < cap32) {
                        const size_t o = (size_t)s_fq[c] * cap32 + dst;
                        cand32[o] = s_fvb[c] + c0 + (ent[u].y & 0xFFFFu);
                        if (cand32_codes) {
#pragma unroll
                            for (int x = 0; x < SPW / 4; ++x) reinterpret_cast<uint4 *>(cand32_codes + o * SPW)[x] = cw[u][x];
                        }
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    };
    // step 2: lane = word (tt, hh) of the current pair
    const uint32_t tt = lane & 31u, hh = lane >> 5;
    const uint32_t woff = tt * 64u + hh * 32u;
    const bool wok = tt < ntt;
    auto jrel_of = [&](uint32_t bpos) {
        const uint32_t r = 15u - (bpos & 15u);
        return (2u * tt + (bpos >> 4)) * 32u + 4u * hh + (r & 3u) + ((r >> 2) << 3);
    };
    // (one copy_out site: the stage is filled with as many pairs -- or as much of a dense pair -- as fit, then copied)
    uint32_t c = 0, r0 = 0;   // current pair; entries of it already copied out (a dense pair spans several rounds)
    for (;;) {
        uint32_t fill = 0;
        while (c < 32u) {
            const uint32_t n_c = (uint32_t)__builtin_amdgcn_readlane((int)n_pair, (int)c);
            if (n_c == 0) {   // (wave-uniform)
                ++c;
                continue;
            }
            const uint32_t rem = n_c - r0;
            if (fill && fill + min(rem, kSpStage) > kSpStage) break;   // no room: copy out first
            const uint32_t take = min(rem, kSpStage - fill);           // entries [r0, r0 + take) of the pair's segment
            const uint32_t w = wok ? bits_w[woff + c] : 0u;
            const uint32_t p = (uint32_t)__popc(w);
            uint32_t x = w, i = wave_incl_scan(p) - p;
            while (x) {
                const uint32_t bpos = (uint32_t)__ffs((int)x) - 1u;
                x &= x - 1u;
                if (i - r0 < take) stage[fill + i - r0] = make_uint2(i, (c << 16) | jrel_of(bpos));
                ++i;
            }
            fill += take;
            r0 += take;
            if (r0 < n_c) break;   // a dense pair: the rest after this copy-out
            ++c;
            r0 = 0;
        }
        if (!fill) break;
        copy_out(fill);
    }
}

#ifndef SCANN_SP_BITS_RUN_MAX
#define SCANN_SP_BITS_RUN_MAX 8
#endif
constexpr uint32_t kSpBitsRunMax = SCANN_SP_BITS_RUN_MAX;   // queue entries a wave of the BITMAP form takes at once, at most
// grab_tile (txh_dev.h) for `run` entries of one queue at once: the tiles first, first + 8, ... (*cnt of them; the run
// is cut at the queue's end).  kInvalid = no tiles left.
__device__ __forceinline__ uint32_t grab_run(uint32_t *queues, uint32_t total_tiles, uint32_t run, uint32_t *cnt) {
    const uint32_t xcd = blockIdx.x & 7u;
    for (uint32_t a2 = 0; a2 < 8u; ++a2) {
        const uint32_t x = (xcd + a2) & 7u;
        const uint32_t nx = (total_tiles + 7u - x) >> 3;   // tiles = x (mod 8)
        uint32_t *ctr = queues + x * CNT_XQ_STRIDE;
        if (a2 && __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= nx) continue;
        const uint32_t l = atomicAdd(ctr, run);
        if (l < nx) {
            *cnt = min(run, nx - l);
            return l * 8u + x;
        }
    }
    *cnt = 0;
    return kInvalid;
}

// The item's end in the BITMAP form of the 64-pair items (flat hashers): the wave copies the item's survivor bitmap
// from LDS to the queries' rows of `surv` as it stands -- query q's 32 words of this range, [tt][h] (128 contiguous
// bytes), at surv[q][range * 32 ..]: bit bpos of word [tt][h] is point
//     jrel = (2 tt + (bpos >> 4)) * 32 + 4 h + (r & 3) + ((r >> 2) << 3),  r = 15 - (bpos & 15)
// of the range.  Words past the item's last tile pair are written as zero (s_bits holds an earlier item's words there),
// padding pairs write nothing.  Every (query, range) belongs to exactly one item of a call, so the rows need no
// clearing and nothing of an earlier call is ever read.  Nothing here waits on memory: eight 16-byte stores per lane,
// eight neighbouring lanes to a query's line.  adc_refine_bits_kernel walks the rows.
__device__ __forceinline__ void sp_store_item_bits(uint32_t *__restrict__ surv, uint32_t stride, const uint32_t *bits_w,
                                                   uint32_t ntile, uint32_t range, const uint32_t (&pq)[2]) {
    constexpr uint32_t TTM = SpItem<2>::TTM;
    static_assert(TTM == 16, "a query's words of an item: 16 tile pairs x 2 halves = 128 bytes");
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t ntt = (ntile + 1u) >> 1;
    const uint32_t k = lane & 7u;           // the 16-byte part of a pair's 128 bytes: words [2k][0], [2k][1], [2k+1][0], [2k+1][1]
    __builtin_amdgcn_wave_barrier();        // (the words of the other lanes)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t p = (uint32_t)i * 8u + (lane >> 3);   // pair of the item: column tile i >> 2, column p & 31
        const uint32_t q = (uint32_t)__shfl((int)pq[i >> 2], (int)(p & 31u));
        const uint32_t *src = bits_w + ((uint32_t)(i >> 2) * TTM + 2u * k) * 64u + (p & 31u);
        // (the eight lanes of a pair read the same bank, 128 words apart: 8-way, ~500 LDS cycles an item against the
        // ~40 k cycles of its MFMAs; the stores stay whole lines)
        uint4 v;
        v.x = src[0]; v.y = src[32]; v.z = src[64]; v.w = src[96];
        if (2u * k >= ntt) v.x = v.y = 0u;
        if (2u * k + 1u >= ntt) v.z = v.w = 0u;
        if (q != kInvalid) *reinterpret_cast<uint4 *>(surv + (size_t)q * stride + range * 32u + 4u * k) = v;
    }
    __builtin_amdgcn_wave_barrier();        // (before the next item's tile loop writes the words again)
}

// WORDS: the word-parallel flush (tree indexes); else lanes walk their own words (flat).  CT: column tiles of 32 pairs
// scored against each point tile.  With CT = 2 the point side of a tile step -- the plane words, their unpacking, the
// byte extractions and every LDS operand read -- is paid once for two MFMA chains (18 MFMAs at S = 32), the wave holds
// both tiles' tables (128 registers at S = 32) and two accumulator pairs, and runs at two waves per SIMD.
// BITMAP (CT = 2 only): the item ends with sp_store_item_bits instead of a flush -- no lists, no allow-list, no stage.
template <int S_, bool WORDS, int CT, bool BITMAP = false>
__device__ __forceinline__ void adc_smfmac_body(const TxhIndexDev &ix, const MfmaArgs &a, const uint64_t allow_stride) {
    typedef int v4i __attribute__((ext_vector_type(4)));
    typedef int v8i __attribute__((ext_vector_type(8)));
    typedef int v16i __attribute__((ext_vector_type(16)));
    typedef SpLayout<S_> SP;
    static_assert(CT == 1 || (CT == 2 && !WORDS && S_ <= 32), "64-pair items: lane-walk flush, S <= 32");
    static_assert(!BITMAP || CT == 2, "the bitmap form is a form of the 64-pair items");
    constexpr int S = S_, NS = SP::NS, KT = NS + 2, NWP = SP::NWP, SPW = SP::SPW;
    // operands in flight ahead of the MFMA that consumes them (CT = 2: every operand feeds two MFMAs, so about the same
    // cover in MFMA slots from fewer registers)
    constexpr int DEPTH = (kMfmaDepth + CT - 1) / CT;
    constexpr int D = DEPTH < KT ? DEPTH : KT;
    constexpr uint32_t kRange = SpItem<CT>::RANGE;              // points per item
    constexpr uint32_t kTT = kRange / 64;                       // tile pairs per item
    __shared__ __attribute__((aligned(16))) uint32_t s_ident[64];   // dense A: 16 one-hot rows of 16 bytes
    __shared__ __attribute__((aligned(16))) uint32_t s_vtab[64];    // sparse A values: row V = (ga | gb << 2)
    __shared__ uint32_t s_ntab[16];                                 // sparse A positions: word N = (ia | ib << 2)
    // survivor bitmap of the wave's item: word [ct][tt][h][col] = the 16-bit masks of tiles 2 tt (low half) and 2 tt + 1
    // of lane (col, h) in column tile ct.  Written once per two tiles with one conflict-free ds_write_b32; no atomics, no
    // branches and no waits in the tile loop -- the item's flush turns it into list entries.
    __shared__ uint32_t s_bits[kMfmaWaves][CT * kTT][64];
    // (BITMAP: no flush.  Its one-element arrays are never referenced and take no LDS -- the kernel's 33 344 bytes are the
    // bitmap and the three operand tables; declaring them through a conditional type changed the instruction streams of
    // the list-form kernels, which this form leaves as they were.)
    constexpr uint32_t kStage = BITMAP ? 1u : SpItem<CT>::STAGE, kRows = BITMAP ? 1u : 32u * CT;
    __shared__ uint2 s_stage[kMfmaWaves][kStage];                                    // flush: staged list entries
    __shared__ uint32_t s_fq[kMfmaWaves][kRows], s_fvb[kMfmaWaves][kRows], s_fgb[kMfmaWaves][kRows];   // flush: per pair
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t col = lane & 31u, h = lane >> 5;
    if (tid < 64) {
        const uint32_t c = tid >> 2, wsel = tid & 3u;
        s_ident[tid] = (wsel == (c >> 2)) ? (1u << (8 * (c & 3u))) : 0u;
        // row V, word wsel: words 0, 1 = bytes 0..7 (group ga = V & 3: value 1 at byte 2 ga), words 2, 3 = bytes 8..15 (gb = V >> 2)
        const uint32_t g = wsel < 2 ? (c & 3u) : (c >> 2);
        s_vtab[tid] = ((g >> 1) == (wsel & 1u)) ? (1u << (16 * (g & 1u))) : 0u;
        if (tid < 16) s_ntab[tid] = (tid & 3u) * 0x1111u | (tid >> 2) * 0x11110000u;
    }
    __syncthreads();
    const uint32_t total_tiles = a.counters[CNT_TOTAL_TILES];
    const char *ident = reinterpret_cast<const char *>(s_ident);
    const char *vtab = reinterpret_cast<const char *>(s_vtab);
    const char *ntab = reinterpret_cast<const char *>(s_ntab);
    uint32_t *bits = &s_bits[wave][0][lane];

    struct Planes {   // one tile's operand planes as LDS byte offsets (see step)
        uint32_t ve[NWP], vo[NWP], ne[NWP], no[NWP], d1;
    };
    struct Ops {      // the first D operands of a tile, fetched during the previous tile's MFMA chain
        v4i av[D];
        int iv[D];
    };

    // BITMAP: a wave takes `run` entries of a queue at once -- tiles 8 apart, which on a flat hasher are ranges 8 apart
    // of the same pair tile -- and keeps its table fragments (32 KB of loads an item at S = 32) while the pair tile
    // stays the same.  run = the items a wave gets anyway (at most 8), so the queues still hand every wave its share.
    uint32_t run = 1, left = 0;   // left: tiles of the current run behind `tile`
    if constexpr (BITMAP) run = min(kSpBitsRunMax, max(1u, (total_tiles + gridDim.x * kMfmaWaves - 1u) / (gridDim.x * kMfmaWaves)));
    uint32_t have_slot0 = kInvalid, have_pt = kInvalid;   // BITMAP: the pair tile whose tables the wave holds
    uint32_t tile = 0;
    if constexpr (BITMAP) {
        uint32_t cnt = 0;
        if (lane == 0) tile = grab_run(a.counters + CNT_XQ, total_tiles, run, &cnt);
        left = (uint32_t)__builtin_amdgcn_readfirstlane(cnt);
        left = left ? left - 1u : 0u;
    } else {
        if (lane == 0) tile = grab_tile(a.counters + CNT_XQ, total_tiles);
    }
    tile = __builtin_amdgcn_readfirstlane(tile);
    // this lane's pair (column) of each column tile: tables (the pass bound is folded into them), key base
    uint32_t pq[CT], vb[CT];
    v4i bd[CT][2];
    v8i bs[CT][NS];
    while (tile != kInvalid) {
        uint32_t next_tile = 0, next_cnt = 0;
        if constexpr (BITMAP) {
            if (left == 0 && lane == 0) next_tile = grab_run(a.counters + CNT_XQ, total_tiles, run, &next_cnt);
        } else {
            if (lane == 0) next_tile = grab_tile(a.counters + CNT_XQ, total_tiles);
        }
        const WorkItem item = decode_item(ix, a.tile_off, a.pair_off, tile);
        const uint32_t lb = item.lb, size = item.size, local = item.local, slot0 = item.slot0, slot_end = item.slot_end;
        const uint32_t nranges = (size + kRange - 1) / kRange;
        const uint32_t range = local % nranges, pt = local / nranges;
        const uint32_t c0 = range * kRange;
        const uint32_t npts = min(kRange, size - c0);

        const bool reload = !BITMAP || slot0 != have_slot0 || pt != have_pt;   // (wave-uniform)
        have_slot0 = slot0;
        have_pt = pt;
        if (reload) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const uint32_t slot = slot0 + pt * (32u * CT) + (uint32_t)ct * 32u + col;
            const bool pair_ok = slot < slot_end;
            pq[ct] = pair_ok ? a.pair_q[slot] : kInvalid;
            vb[ct] = pair_ok ? a.pair_vbase[slot] : 0u;
            const int8_t *bsrc = a.lut8 + (size_t)(pair_ok ? slot : slot0) * S * 16;
#pragma unroll
            for (int d = 0; d < 2; ++d) bd[ct][d] = *reinterpret_cast<const v4i *>(bsrc + (size_t)(2 * d + h) * 16);
#pragma unroll
            for (int kt = 0; kt < NS; ++kt) {
                const v4i x0 = *reinterpret_cast<const v4i *>(bsrc + (size_t)(4 + 4 * kt + 2 * h) * 16);
                const v4i x1 = *reinterpret_cast<const v4i *>(bsrc + (size_t)(4 + 4 * kt + 2 * h) * 16 + 16);
                bs[ct][kt] = v8i{x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
            }
            if (!pair_ok) {   // padding columns: every entry 127, sums stay positive (nothing passes)
                const int k7 = 0x7F7F7F7F;
#pragma unroll
                for (int d = 0; d < 2; ++d) bd[ct][d] = v4i{k7, k7, k7, k7};
#pragma unroll
                for (int kt = 0; kt < NS; ++kt) bs[ct][kt] = v8i{k7, k7, k7, k7, k7, k7, k7, k7};
            }
        }
        }

        const uint32_t ntile = (npts + 31u) >> 5;
        static_assert(NWP == 1 || NWP == 2, "plane words");
        struct Raw {
            uint32_t wv[NWP], wn[NWP];
        };
        auto load_planes = [&](uint32_t t) {   // raw planes of tile t (rows past the leaf's end: any row, masked later)
            const uint32_t j = c0 + t * 32u + col;
            const uint32_t *src = ix.codes_sp + (size_t)(lb + (j < size ? j : 0u)) * SPW + h * 2u * NWP;
            Raw r;
            if constexpr (NWP == 1) {
                const uint2 v = *reinterpret_cast<const uint2 *>(src);
                r.wv[0] = v.x; r.wn[0] = v.y;
            } else {
                const uint4 v = *reinterpret_cast<const uint4 *>(src);
                r.wv[0] = v.x; r.wv[1] = v.y; r.wn[0] = v.z; r.wn[1] = v.w;
            }
            return r;
        };
        // planes -> LDS byte offsets: nibble j of the V plane times 16 (a 16-byte row), of the N plane times 4
        auto unpack = [&](const Raw &r) {
            Planes p;
#pragma unroll
            for (int wi = 0; wi < NWP; ++wi) {
                p.ve[wi] = r.wv[wi] & 0xF0F0F0F0u;
                p.vo[wi] = (r.wv[wi] << 4) & 0xF0F0F0F0u;
                p.ne[wi] = (r.wn[wi] >> 2) & 0x3C3C3C3Cu;
                p.no[wi] = (r.wn[wi] << 2) & 0x3C3C3C3Cu;
                // (opaque to the optimiser: it would otherwise re-derive every offset from the plane word with a
                // shift and a mask of its own -- two vector instructions per offset instead of one byte extraction)
                asm volatile("" : "+v"(p.ve[wi]), "+v"(p.vo[wi]), "+v"(p.ne[wi]), "+v"(p.no[wi]));
            }
            p.d1 = ((r.wn[NS >> 3] >> (4 * (NS & 7))) & 15u) << 4;   // dense MFMA 1: raw code, last nibble of the N plane
            return p;
        };
        auto voff = [&](const Planes &p, int j) { return (((j & 1) ? p.ve[j >> 3] : p.vo[j >> 3]) >> (8 * ((j & 7) >> 1))) & 0xFFu; };
        auto noff = [&](const Planes &p, int j) { return (((j & 1) ? p.ne[j >> 3] : p.no[j >> 3]) >> (8 * ((j & 7) >> 1))) & 0xFFu; };
        // operands of MFMA oi: 0, 1 dense (identity rows), 2 .. sparse (value row + position word)
        auto fetch = [&](const Planes &p, int oi, v4i &av, int &iv) {
            if (oi == 0) {
                av = *reinterpret_cast<const v4i *>(ident + voff(p, NS));
            } else if (oi == 1) {
                av = *reinterpret_cast<const v4i *>(ident + p.d1);
            } else {
                av = *reinterpret_cast<const v4i *>(vtab + voff(p, oi - 2));
                iv = *reinterpret_cast<const int *>(ntab + noff(p, oi - 2));
            }
        };
        // Software pipeline over the item's tiles.  step(t): the MFMA chain of tile t into accN; between its MFMAs
        // the survivor mask of tile t - 1 from accO (the sign of each result), the operand reads of the chain's
        // later MFMAs and -- in its last D slots -- of the FIRST D MFMAs of tile t + 1, so that no chain starts with
        // an exposed LDS round trip; the global load of tile t + 2's planes is issued at the top.  One extra step
        // drains the last tile (its MFMAs run on stale operands and are dropped).
        Raw rawn = load_planes(ntile > 1 ? 1u : 0u);
        Planes pl = unpack(load_planes(0u));
        Ops ops;
#pragma unroll
        for (int oi = 0; oi < D; ++oi) fetch(pl, oi, ops.av[oi], ops.iv[oi]);
        uint32_t mlo[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) mlo[ct] = 0;
        // (CT = 2: every operand is fetched once and issued to both column tiles' chains, ct = 0 then ct = 1, so that
        // consecutive MFMAs never depend on each other; both masks are built in the same shadow)
        auto step = [&](v16i (&accN)[CT], const v16i (&accO)[CT], uint32_t t, auto hi_half) {
            const Planes pn = unpack(rawn);                        // tile t + 1 (loaded during step t - 1)
            if (t + 2 < ntile) rawn = load_planes(t + 2);
            v4i av[KT];
            int iv[KT];
            Ops nops;
#pragma unroll
            for (int oi = 0; oi < D; ++oi) {
                av[oi] = ops.av[oi];
                iv[oi] = ops.iv[oi];
            }
            // lane (col, h), register r: point row (r & 3) + 8 * (r >> 2) + 4 * h of the tile; result r's sign
            // (negative = passes) ends up at bit 15 - r of the mask
            uint32_t m16[CT];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) m16[ct] = 0;
            __builtin_amdgcn_s_setprio(2);
#pragma unroll
            for (int oi = 0; oi < KT; ++oi) {
                if (oi + D < KT) fetch(pl, oi + D, av[oi + D], iv[oi + D]);
                else fetch(pn, oi + D - KT, nops.av[oi + D - KT], nops.iv[oi + D - KT]);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    if (oi == 0)
                        accN[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[0], bd[ct][0], v16i{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, 0, 0, 0);
                    else if (oi == 1)
                        accN[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[1], bd[ct][1], accN[ct], 0, 0, 0);
                    else
                        accN[ct] = __builtin_amdgcn_smfmac_i32_32x32x64_i8(av[oi], bs[ct][oi - 2], accN[ct], iv[oi], 0, 0);
                }
#pragma unroll
                for (int r = oi * 16 / KT; r < (oi + 1) * 16 / KT; ++r)
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) m16[ct] = __builtin_amdgcn_alignbit(m16[ct], (uint32_t)accO[ct][r], 31);
                __builtin_amdgcn_sched_barrier(0);
            }
            __builtin_amdgcn_s_setprio(0);
            ops = nops;
            pl = pn;
            if (t == 0) return;                // nothing before the first tile (wave-uniform)
            if (t == ntile && (npts & 31u)) {  // partial last tile: rows past the leaf's end are padding
                const uint32_t base = c0 + (t - 1) * 32u + 4u * h;
                uint32_t okm = 0;
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    okm |= (base + (uint32_t)((r & 3) + 8 * (r >> 2)) < size ? 1u : 0u) << (15 - r);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) m16[ct] &= okm;
            }
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                if constexpr (decltype(hi_half)::value) {
                    bits[((uint32_t)ct * kTT + ((t - 1) >> 1)) * 64u] = mlo[ct] | (m16[ct] << 16);
                } else {
                    mlo[ct] = m16[ct];
                }
            }
        };
        // (tile 0 is peeled: inside the loop t >= 1 is known, so the compiler keeps the mask build between
        // the MFMAs in BOTH instances instead of sinking it below a `t == 0` branch)
        v16i accA[CT], accB[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) accA[ct] = accB[ct] = v16i{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        step(accA, accB, 0u, std::false_type());
        for (uint32_t tl = 1; tl <= ntile; tl += 2) {
            step(accB, accA, tl, std::false_type());                          // mask of tile tl - 1 (even): low half
            if (tl + 1 <= ntile) step(accA, accB, tl + 1, std::true_type());  // mask of tile tl (odd): high half, write
        }
        if (ntile & 1u) {   // the last tile had an even number: its word has no high half
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) bits[((uint32_t)ct * kTT + (ntile >> 1)) * 64u] = mlo[ct];
        }
        // ---- flush: the item's bitmap -> the queries' lists (sp_flush_item: its own function, so that its registers
        // are allocated apart from the tile loop's -- inlined, the loop spilled its table fragments)
        if constexpr (BITMAP)
            sp_store_item_bits(a.surv, a.surv_stride, &s_bits[wave][0][0], ntile, range, pq);
        else if constexpr (WORDS)
            sp_flush_item_words<S>(ix.codes_sp, ix, a.allow, a.allow_bits, allow_stride, a.cand32_cnt, a.cand32, a.cand32_codes, a.cap32, &s_bits[wave][0][0],
                                   s_stage[wave], s_fq[wave], s_fvb[wave], s_fgb[wave], ntile, c0, lb, pq[0], vb[0]);
        else
            sp_flush_item_lanes<S, CT>(ix.codes_sp, ix, a.allow, a.allow_bits, allow_stride, a.cand32_cnt, a.cand32, a.cand32_codes, a.cap32, bits, s_stage[wave],
                                       s_fq[wave], s_fvb[wave], s_fgb[wave], ntile, c0, lb, pq, vb);
        if constexpr (BITMAP) {
            if (left) {
                tile += 8u;
                --left;
            } else {
                tile = __builtin_amdgcn_readfirstlane(next_tile);
                left = (uint32_t)__builtin_amdgcn_readfirstlane(next_cnt);
                left = left ? left - 1u : 0u;
            }
        } else {
            tile = __builtin_amdgcn_readfirstlane(next_tile);
        }
    }
}

// S <= 32: three waves per SIMD (the pair tile's table fragments alone are 64 registers); S = 48, 64: two.  (Capping the
// registers at 144 to leave room for a wave of another stream's kernel was tried: amdgpu_num_vgpr is ignored by this
// compiler, and two waves per SIMD (two workgroups per CU) cost the scan 10 % and gained the two-stream step nothing.)
#ifndef SCANN_SP_VGPRS
#define SCANN_SP_VGPRS 144
#endif
template <int S_, bool WORDS>
__global__ __launch_bounds__(kMfmaWaves * 64, SCANN_MFMA_MINW) __attribute__((amdgpu_num_vgpr(SCANN_SP_VGPRS)))
void adc_smfmac_kernel(TxhIndexDev ix, MfmaArgs a) {
    adc_smfmac_body<S_, WORDS, 1>(ix, a, 0);
}
template <int S_, bool WORDS>
__global__ __launch_bounds__(kMfmaWaves * 64, 2) void adc_smfmac_wide_kernel(TxhIndexDev ix, MfmaArgs a) {   // S = 48, 64
    adc_smfmac_body<S_, WORDS, 1>(ix, a, 0);
}
// (_pq: one bitmap per query, allow_stride words apart; see adc_mfma_pq_kernel)
template <int S_, bool WORDS>
__global__ __launch_bounds__(kMfmaWaves * 64, SCANN_MFMA_MINW) __attribute__((amdgpu_num_vgpr(SCANN_SP_VGPRS)))
void adc_smfmac_pq_kernel(TxhIndexDev ix, MfmaArgs a, uint64_t allow_stride) {
    adc_smfmac_body<S_, WORDS, 1>(ix, a, allow_stride);
}
template <int S_, bool WORDS>
__global__ __launch_bounds__(kMfmaWaves * 64, 2) void adc_smfmac_wide_pq_kernel(TxhIndexDev ix, MfmaArgs a, uint64_t allow_stride) {
    adc_smfmac_body<S_, WORDS, 1>(ix, a, allow_stride);
}
// The 64-pair form (CT = 2; S <= 32, lane-walk flush): two tiles' tables and two accumulator pairs, two waves per SIMD.
template <int S_>
__global__ __launch_bounds__(kMfmaWaves * 64, 2) void adc_smfmac_kernel64(TxhIndexDev ix, MfmaArgs a) {
    adc_smfmac_body<S_, false, 2>(ix, a, 0);
}
template <int S_>
__global__ __launch_bounds__(kMfmaWaves * 64, 2) void adc_smfmac_pq_kernel64(TxhIndexDev ix, MfmaArgs a, uint64_t allow_stride) {
    adc_smfmac_body<S_, false, 2>(ix, a, allow_stride);
}

// ... and its BITMAP form: the item's survivor bitmap goes to MfmaArgs::surv as it is (no lists, no allow-list: the
// refine tests it).  Its LDS is the bitmap alone (32 KB a workgroup); registers still hold it at two waves per SIMD.
template <int S_>
__global__ __launch_bounds__(kMfmaWaves * 64, 2) void adc_smfmac_bits_kernel64(TxhIndexDev ix, MfmaArgs a) {
    adc_smfmac_body<S_, false, 2, true>(ix, a, 0);
}

// The prefilter with 16-pair tiles on v_mfma_i32_16x16x64_i8, for leaves scanned by 8-24 queries of the batch
// (typical Tree-X-Hybrid batches: 1024 queries x 10 leaves over 1000 leaves): a 32-pair tile would be a
// third full there.  A tile = 32 points (two groups of 16) x 16 pairs = 2 x S/4 MFMAs of 4 subspaces each, two
// independent accumulator chains of 4 registers.  Lane (c16 = lane & 15, kb = lane >> 4): A row = point c16 of
// the group, K block kb = subspace 4 kt + kb (one-hot row from the LDS identity table); B column = pair c16;
// results D[row 4 kb + r][column c16], r = 0..3.  Items, bounds, staging, flush and lists as in adc_mfma_kernel
// (the worklist is built with 4 quads per tile).  Measured as a 32-pair kernel (two halves) this shape lost to
// adc_mfma_kernel (more vector work per tile); here it replaces the f32 LDS-gather scan.
template <int S_>
__device__ __forceinline__ void adc_mfma16_body(TxhIndexDev ix, MfmaArgs a, const uint64_t allow_stride) {
    typedef int v4i __attribute__((ext_vector_type(4)));
    constexpr int S = S_, KT = S / 4, NW = S / 8, NP = (NW + 1) / 2;
    __shared__ __attribute__((aligned(16))) uint32_t s_ident[64];                 // 16 one-hot rows of 16 bytes
    __shared__ uint32_t s_stage[kMfmaWaves][16][kMfmaStage];
    __shared__ uint32_t s_cnt[kMfmaWaves][16];
    __shared__ uint32_t s_fpre[kMfmaWaves][16], s_fq[kMfmaWaves][16], s_fgb[kMfmaWaves][16], s_fvb[kMfmaWaves][16];   // per pair
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t c16 = lane & 15u, kb = lane >> 4;
    if (tid < 64) {
        const uint32_t c = tid >> 2, wsel = tid & 3u;
        s_ident[tid] = (wsel == (c >> 2)) ? (1u << (8 * (c & 3u))) : 0u;
    }
    __syncthreads();
    const uint32_t total_tiles = a.counters[CNT_TOTAL_TILES];
    const char *ident = reinterpret_cast<const char *>(s_ident);

    uint32_t tile = 0;
    if (lane == 0) tile = grab_tile(a.counters + CNT_XQ, total_tiles);
    tile = __builtin_amdgcn_readfirstlane(tile);
    while (tile != kInvalid) {
        uint32_t next_tile = 0;
        if (lane == 0) next_tile = grab_tile(a.counters + CNT_XQ, total_tiles);
        const WorkItem item = decode_item(ix, a.tile_off, a.pair_off, tile);
        const uint32_t lb = item.lb, size = item.size, local = item.local, slot0 = item.slot0, slot_end = item.slot_end;
        const uint32_t nranges = (size + kMfmaRange - 1) / kMfmaRange;
        const uint32_t range = local % nranges, pt = local / nranges;
        const uint32_t c0 = range * kMfmaRange;
        const uint32_t npts = min(kMfmaRange, size - c0);

        // this lane's pair (column c16 of the tile): tables, bound; query and key base go to LDS for the flush
        const uint32_t slot = slot0 + pt * 16u + c16;
        const bool pair_ok = slot < slot_end;
        if (lane < 16) {
            s_cnt[wave][lane] = 0;
            s_fq[wave][lane] = pair_ok ? a.pair_q[slot] : kInvalid;
            s_fvb[wave][lane] = pair_ok ? a.pair_vbase[slot] : 0u;
        }
        v4i b[KT];
        {
            const int8_t *bsrc = a.lut8 + ((size_t)(pair_ok ? slot : slot0) * S + kb) * 16;   // padding columns: any table
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) b[kt] = *reinterpret_cast<const v4i *>(bsrc + (size_t)kt * 64);
        }
        const int thr1 = pair_ok ? a.thr1[slot] : -(128 * S + 7);   // a point passes iff acc - thr1 < 0

        const uint32_t ntile = (npts + 31u) >> 5;
        uint32_t wn[2][NW];
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const uint32_t j = c0 + 16u * g + c16;
            Codec<S, 4>::load_words(ix.codes + (size_t)(lb + (j < size ? j : 0u)) * NW, wn[g]);
        }
        auto flush = [&](bool all) {
            uint32_t n = 0, gbase = 0;
            if (lane < 16) {
                n = min(s_cnt[wave][lane], kMfmaStage);
                if (!all && n + 32u <= kMfmaStage) n = 0;
                if (n) {
                    gbase = atomicAdd(&a.cand32_cnt[s_fq[wave][lane]], n);
                    s_cnt[wave][lane] = 0;
                }
            }
            uint32_t incl = n;
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
                if ((int)lane >= o) incl += up;
            }
            const uint32_t total = (uint32_t)__shfl((int)incl, 15);
            if (total == 0) return;
            if (lane < 16) {
                s_fpre[wave][lane] = incl - n;
                s_fgb[wave][lane] = gbase;
            }
            for (uint32_t e = lane; e < total; e += 64u) {
                uint32_t c = 0;
#pragma unroll
                for (uint32_t stp = 8; stp; stp >>= 1)
                    if (s_fpre[wave][c + stp] <= e) c += stp;
                const uint32_t idx = e - s_fpre[wave][c];
                const uint32_t j = s_stage[wave][c][idx];
                const uint32_t dst = s_fgb[wave][c] + idx;
                append_survivor<S>(a.cand32, a.cand32_codes, a.cap32, s_fq[wave][c], dst, s_fvb[wave][c] + j, ix.codes + (size_t)(lb + j) * NW);
            }
        };
        // step(t): the MFMAs of tile t into accN, the survivor mask of tile t - 1 from accO between them, then
        // the staging of tile t - 1's survivors
        auto step = [&](v4i (&accN)[2], const v4i (&accO)[2], uint32_t t) {
            // byte kt' of pk[g][i] = code * 16 of subspace 4 kt + kb, kt = 4 i + {0, 2, 1, 3}[kt']
            uint32_t pk[2][NP];
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int i = 0; i < NP; ++i) {
                    const uint32_t y0 = (wn[g][2 * i] >> (4u * kb)) & 0x000F000Fu;
                    const uint32_t y1 = (2 * i + 1 < NW) ? ((wn[g][(2 * i + 1 < NW) ? 2 * i + 1 : 0] >> (4u * kb)) & 0x000F000Fu) : 0u;
                    pk[g][i] = (y0 | (y1 << 8)) << 4;
                }
            if (t + 1 < ntile) {
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    const uint32_t j = c0 + (t + 1) * 32u + 16u * g + c16;
                    Codec<S, 4>::load_words(ix.codes + (size_t)(lb + (j < size ? j : 0u)) * NW, wn[g]);
                }
            }
            accN[0] = v4i{0, 0, 0, 0};
            accN[1] = v4i{0, 0, 0, 0};
            constexpr int NA = 2 * KT;                        // MFMAs per tile, in order (kt, g)
            constexpr int D = kMfmaDepth < NA ? kMfmaDepth : NA;
            v4i av[D + 1];
            auto onehot = [&](int ai) {
                const int kt = ai >> 1, g = ai & 1;
                const int byte = ((kt & 1) << 1) | ((kt >> 1) & 1);   // kt & 3 -> {0, 2, 1, 3}
                const uint32_t off = (pk[g][kt >> 2] >> (8 * byte)) & 0xFFu;
                return *reinterpret_cast<const v4i *>(ident + off);
            };
#pragma unroll
            for (int ai = 0; ai < D; ++ai) av[ai] = onehot(ai);
            uint32_t m8 = 0;   // survivor bits: result (g, r) at bit 7 - (4 g + r)
            __builtin_amdgcn_s_setprio(2);
#pragma unroll
            for (int ai = 0; ai < NA; ++ai) {
                const int kt = ai >> 1, g = ai & 1;
                if (ai + D < NA) av[(ai + D) % (D + 1)] = onehot(ai + D);
                accN[g] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[ai % (D + 1)], b[kt], accN[g], 0, 0, 0);
#pragma unroll
                for (int ri = ai * 8 / NA; ri < (ai + 1) * 8 / NA; ++ri)
                    m8 = __builtin_amdgcn_alignbit(m8, (uint32_t)(accO[ri >> 2][ri & 3] - thr1), 31);
                __builtin_amdgcn_sched_barrier(0);
            }
            __builtin_amdgcn_s_setprio(0);
            if (t == 0) return;
            const uint32_t base = c0 + (t - 1) * 32u + 4u * kb;
            if (t == ntile && (npts & 31u)) {  // partial last tile: rows past the leaf's end are padding
                uint32_t okm = 0;
#pragma unroll
                for (int ri = 0; ri < 8; ++ri)
                    okm |= (base + 16u * (uint32_t)(ri >> 2) + (uint32_t)(ri & 3) < size ? 1u : 0u) << (7 - ri);
                m8 &= okm;
            }
            bool risk = false;
            m8 &= 0xFFu;
            if (a.allow && m8)                 // search_with_filter: disallowed points are not survivors
                m8 = mask_allowed(ix, a.allow, allow_stride, s_fq[wave][c16], a.allow_bits, lb, m8, [&](uint32_t b) {
                    const uint32_t qi = 7u - b;
                    return base + 16u * (qi >> 2) + (qi & 3u);
                });
            if (m8) {
                uint32_t sl = atomicAdd(&s_cnt[wave][c16], (uint32_t)__popc(m8));
                do {
                    const uint32_t qi = 7u - ((uint32_t)__ffs((int)m8) - 1u);
                    m8 &= m8 - 1u;
                    const uint32_t j = base + 16u * (qi >> 2) + (qi & 3u);
                    if (sl < kMfmaStage) {
                        s_stage[wave][c16][sl] = j;
                    } else {   // stage full: direct (slow) append
                        const uint32_t pqd = s_fq[wave][c16];
                        const uint32_t pos = atomicAdd(&a.cand32_cnt[pqd], 1u);
                        append_survivor<S>(a.cand32, a.cand32_codes, a.cap32, pqd, pos, s_fvb[wave][c16] + j, ix.codes + (size_t)(lb + j) * NW);
                    }
                    ++sl;
                } while (m8);
                risk = sl + 32u > kMfmaStage;
            }
            if (__any(risk)) flush(false);
        };
        v4i accA[2], accB[2];
        accA[0] = accA[1] = accB[0] = accB[1] = v4i{0, 0, 0, 0};
        step(accA, accB, 0u);
        for (uint32_t tl = 1; tl <= ntile; tl += 2) {
            step(accB, accA, tl);
            if (tl + 1 <= ntile) step(accA, accB, tl + 1);
        }
        flush(true);
        tile = __builtin_amdgcn_readfirstlane(next_tile);
    }
}
// One bitmap for the batch, or none: the kernel every search without allow_bitmap_stride runs (its code is that of the
// body with the stride folded to 0).  _pq: one bitmap per query, allow_stride words apart.
template <int S_>
__global__ __launch_bounds__(kMfmaWaves * 64, (S_ <= 32 ? 4 : 2)) void adc_mfma16_kernel(TxhIndexDev ix, MfmaArgs a) {
    adc_mfma16_body<S_>(ix, a, 0);
}
template <int S_>
__global__ __launch_bounds__(kMfmaWaves * 64, (S_ <= 32 ? 4 : 2)) void adc_mfma16_pq_kernel(TxhIndexDev ix, MfmaArgs a, uint64_t allow_stride) {
    adc_mfma16_body<S_>(ix, a, allow_stride);
}

// Exact refine of the prefilter's survivors: block per query.  Recomputes the reference's f32 sums
// (LookupTable::compute_distance, hashes/lut.rs:74-82: acc = lut[0][c0]; acc += lut[s][cs], s
// ascending), forms the merge keys and keeps key <= T -- exactly adc_scan_kernel's survivors.
struct RefineArgs {
    uint32_t P, cap, cap32;
    const uint32_t *tokens, *vbase, *slot_of;
    const float *lutq;
    const uint64_t *thr;
    const uint32_t *cand32_cnt, *cand32, *cand32_codes;
    uint32_t *cand_cnt;
    uint64_t *cand;
    uint32_t *counters;
    const uint64_t *allow;
    uint64_t allow_bits, allow_stride;
    int planes;   // cand32_codes holds codes_sp plane rows (adc_smfmac_kernel), not packed codes
    const uint32_t *surv;   // adc_refine_bits_kernel: [nq..][surv_stride] survivor bitmaps (adc_smfmac_bits_kernel64)
    uint32_t surv_stride;   // words per query (a multiple of 32)
};

// code of subspace s from a point's plane row (SpLayout: [ha][plane V, N][word]); ca / cb = the code nibbles of the
// first / second subspace each sparse MFMA takes from parity ha, rebuilt word-parallel by sp_row_decode
template <int S>
struct SpRow {
    static constexpr int NWP = SpLayout<S>::NWP, NS = SpLayout<S>::NS;
    uint32_t ca[2][NWP], cb[2][NWP], dv[2], dn[2];   // dv / dn: the dense MFMAs' raw codes (subspaces ha, 2 + ha)
    __device__ __forceinline__ void decode(const uint32_t *row) {
#pragma unroll
        for (int ha = 0; ha < 2; ++ha) {
#pragma unroll
            for (int wi = 0; wi < NWP; ++wi) {
                const uint32_t v = row[(ha * 2 + 0) * NWP + wi], n = row[(ha * 2 + 1) * NWP + wi];
                ca[ha][wi] = ((v & 0x33333333u) << 2) | (n & 0x33333333u);
                cb[ha][wi] = (v & 0xCCCCCCCCu) | ((n >> 2) & 0x33333333u);
            }
            dv[ha] = (row[(ha * 2 + 0) * NWP + (NS >> 3)] >> (4 * (NS & 7))) & 15u;
            dn[ha] = (row[(ha * 2 + 1) * NWP + (NS >> 3)] >> (4 * (NS & 7))) & 15u;
        }
    }
    __device__ __forceinline__ uint32_t code(int s) const {   // s: compile-time after unrolling
        if (s < 4) return (s >> 1) ? dn[s & 1] : dv[s & 1];
        const int kt = (s - 4) >> 2, q = (s - 4) & 3, ha = q & 1;
        const uint32_t src = (q >> 1) ? cb[ha][kt >> 3] : ca[ha][kt >> 3];
        return (src >> (4 * (kt & 7))) & 15u;
    }
};

#ifndef SCANN_REFINE_THREADS
#define SCANN_REFINE_THREADS 256
#endif
#ifndef SCANN_REFINE_U
#define SCANN_REFINE_U 4
#endif
constexpr uint32_t kRefineThreads = SCANN_REFINE_THREADS;

template <typename C>
__global__ __launch_bounds__(kRefineThreads) void adc_refine_kernel(TxhIndexDev ix, RefineArgs a) {
    constexpr int S = C::S, NW = C::NWORDS;
    // words per list entry: packed codes, or (4-bit codes behind the sparse-MFMA prefilter) the point's plane row
    constexpr int SPW = C::BITS == 4 ? (int)(4 * ((((S - 4) / 4 + 1) + 7) / 8)) : NW;
    constexpr int RW = SPW > NW ? SPW : NW;
    const bool planes = C::BITS == 4 && a.planes;   // (block-uniform)
    const uint32_t ew = planes ? (uint32_t)SPW : (uint32_t)NW;
    extern __shared__ __attribute__((aligned(16))) float s_tab[];       // [min(P, kRefineTablesMax)][S][16]
    __shared__ uint32_t s_dvb[kDecodeStage], s_drow[kDecodeStage], s_slot[kDecodeStage], s_out;
    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
    const uint32_t P = a.P;
    const uint32_t cnt = a.cand32_cnt[q];
    if (cnt > a.cap32) {   // list overflow: report, never a wrong row
        if (tid == 0) {
            atomicMax(&a.counters[CNT_STATUS], (uint32_t)SCANN_HIP_RESOURCE_EXHAUSTED);
            a.cand_cnt[q] = a.cap + 1u;
        }
        return;
    }
    const uint64_t T = a.thr[q];
    const bool staged = P <= kDecodeStage;
    const bool tabs = P <= kRefineTablesMax;
    const uint32_t *vbq = a.vbase + (size_t)q * (P + 1);
    if (staged)
        for (uint32_t r = tid; r < P; r += kRefineThreads) {
            s_dvb[r] = vbq[r];
            s_drow[r] = ix.leaf_off[a.tokens[(size_t)q * P + r]];
            s_slot[r] = a.slot_of[(size_t)q * P + r];
        }
    if (tid == 0) s_out = 0;
    __syncthreads();
    if (tabs) {   // this query's pair tables, de-interleaved: [r][s][16]
        for (uint32_t e = tid; e < P * S * 16; e += kRefineThreads) {
            const uint32_t r = e / (S * 16), sc = e - r * (S * 16);
            const uint32_t slot = staged ? s_slot[r] : a.slot_of[(size_t)q * P + r];
            s_tab[e] = slot == kInvalid ? 0.0f : a.lutq[((size_t)(slot >> 2) * S * 16 + sc) * 4 + (slot & 3u)];
        }
        __syncthreads();
    }
    uint64_t *out = a.cand + (size_t)q * a.cap;
    const uint32_t *list = a.cand32 + (size_t)q * a.cap32;
    const uint32_t *list_codes = a.cand32_codes ? a.cand32_codes + (size_t)q * a.cap32 * ew : nullptr;
    constexpr int U = SCANN_REFINE_U;   // entries per thread per pass: their dependent loads (position -> codes) overlap
    for (uint32_t b0 = 0; b0 < cnt; b0 += kRefineThreads * U) {
        uint32_t vpos[U], csr[U], lo_[U];
        uint32_t w[U][RW];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t e = b0 + tid + kRefineThreads * u;
            vpos[u] = e < cnt ? list[e] : 0xFFFFFFFFu;
            if (a.cand32_codes) {   // (written with the position)
                const uint32_t *src = list_codes + (size_t)(e < cnt ? e : 0u) * ew;
                if (planes) {
#pragma unroll
                    for (int x = 0; x < SPW / 4; ++x) {
                        const uint4 v = reinterpret_cast<const uint4 *>(src)[x];
                        w[u][4 * x] = v.x; w[u][4 * x + 1] = v.y; w[u][4 * x + 2] = v.z; w[u][4 * x + 3] = v.w;
                    }
                } else {
                    uint32_t t[NW];
                    C::load_words(src, t);
#pragma unroll
                    for (int x = 0; x < NW; ++x) w[u][x] = t[x];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            uint32_t lo = 0, hi = P;
            const uint32_t vp = vpos[u] == 0xFFFFFFFFu ? 0u : vpos[u];
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if ((staged ? s_dvb[mid] : vbq[mid]) <= vp) lo = mid; else hi = mid;
            }
            lo_[u] = lo;
            csr[u] = (staged ? s_drow[lo] : ix.leaf_off[a.tokens[(size_t)q * P + lo]]) + (vp - (staged ? s_dvb[lo] : vbq[lo]));
            if (!a.cand32_codes) {
                uint32_t t[NW];
                C::load_words(ix.codes + (size_t)(vpos[u] == 0xFFFFFFFFu ? 0u : csr[u]) * NW, t);
#pragma unroll
                for (int x = 0; x < NW; ++x) w[u][x] = t[x];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            bool keep = false;
            uint64_t key = 0;
            if (vpos[u] != 0xFFFFFFFFu) {
                float acc = 0.0f;
                bool done = false;
                if constexpr (C::BITS == 4) {
                    if (planes && tabs) {   // (the sparse prefilter runs with staged tables: P <= kRefineTablesMax or not, both forms)
                        SpRow<S> row;
                        row.decode(w[u]);
                        const float *tb = s_tab + lo_[u] * (S * 16);
#pragma unroll
                        for (int s2 = 0; s2 < S; ++s2) {
                            const float tv = tb[s2 * 16 + row.code(s2)];
                            acc = s2 == 0 ? tv : acc + tv;
                        }
                        done = true;
                    } else if (planes) {
                        SpRow<S> row;
                        row.decode(w[u]);
                        const uint32_t slot = staged ? s_slot[lo_[u]] : a.slot_of[(size_t)q * P + lo_[u]];
                        const float *tb = a.lutq + (size_t)(slot >> 2) * S * 64 + (slot & 3u);
#pragma unroll
                        for (int s2 = 0; s2 < S; ++s2) {
                            const float tv = tb[(s2 * 16 + row.code(s2)) * 4];
                            acc = s2 == 0 ? tv : acc + tv;
                        }
                        done = true;
                    }
                }
                if (done) {
                } else if (tabs) {
                    const float *tb = s_tab + lo_[u] * (S * 16);
#pragma unroll
                    for (int s2 = 0; s2 < S; ++s2) {
                        const uint32_t code = (w[u][s2 >> 3] >> (4 * (s2 & 7))) & 15u;
                        const float tv = tb[s2 * 16 + code];
                        acc = s2 == 0 ? tv : acc + tv;
                    }
                } else {
                    const uint32_t slot = staged ? s_slot[lo_[u]] : a.slot_of[(size_t)q * P + lo_[u]];
                    const float *tb = a.lutq + (size_t)(slot >> 2) * S * 64 + (slot & 3u);
#pragma unroll
                    for (int s2 = 0; s2 < S; ++s2) {   // (fully unrolled: a dynamic index would push w[] to scratch)
                        const uint32_t code = (w[u][s2 >> 3] >> (4 * (s2 & 7))) & 15u;
                        const float tv = tb[(s2 * 16 + code) * 4];
                        acc = s2 == 0 ? tv : acc + tv;
                    }
                }
                key = make_key(acc, vpos[u]);
                keep = key <= T && row_allowed(ix, a.allow, a.allow_stride, q, a.allow_bits, csr[u]);
            }
            uint32_t wtot;
            const uint32_t wpre = wave_prefix_count(keep, &wtot);
            uint32_t base = 0;
            if (lane == 0 && wtot) base = atomicAdd(&s_out, wtot);
            base = (uint32_t)__shfl((int)base, 0);
            if (keep && base + wpre < a.cap) out[base + wpre] = key;
        }
    }
    __syncthreads();
    if (tid == 0) a.cand_cnt[q] = s_out;   // > cap: select_rerank reports the overflow
}

// The refine behind adc_smfmac_bits_kernel64 (flat hashers: one leaf, P = 1): block per query, the query's table staged
// in LDS as above; the survivors come from the query's row of the bitmap (sp_store_item_bits gives the bit -> point
// map) and their plane rows from ix.codes_sp.  The row is ~1 % dense, so a thread that scored the bits of its own words
// would leave three lanes in four idle: every wave takes the row 256 words at a time (one 16-byte load per lane, the
// next one in flight), its lanes push the points of their words' set bits onto the wave's LDS queue (a DPP prefix gives
// each lane its place), and whenever the queue holds kRefineBitsU full waves of points they are popped off its end
// and scored side by side -- allow bit first, then the plane-row gather, SpRow decode, the sequential f32 sum, the key
// and key <= T, as adc_refine_kernel does them.  A chunk that holds more points than the queue has room for (dense
// rows: a bound every point meets) is pushed in rounds.  All blocks walk their rows upwards from word 0, so the batch
// sweeps the plane array roughly together and its lines repeat in the L2s.
#ifndef SCANN_REFINE_BITS_THREADS
#define SCANN_REFINE_BITS_THREADS 256
#endif
constexpr uint32_t kRefineBitsThreads = SCANN_REFINE_BITS_THREADS;   // (512: refine 135 us against 119 us at the flagship)
constexpr uint32_t kRefineBitsU = 4;            // points per lane scored side by side
constexpr uint32_t kRefineBitsQueue = 1024;     // points a wave's queue holds
static_assert(kRefineBitsQueue > 2 * 64 * kRefineBitsU, "room for a push on top of what a pop leaves");

template <typename C>
__global__ __launch_bounds__(kRefineBitsThreads, kRefineBitsThreads >= 512 ? 8 : 4) void adc_refine_bits_kernel(TxhIndexDev ix, RefineArgs a) {
    constexpr int S = C::S;
    constexpr int SPW = SpLayout<S>::SPW;
    constexpr uint32_t U = kRefineBitsU, POP = 64u * U, NWAVES = kRefineBitsThreads / 64u;
    static_assert(C::BITS == 4 && kSpRange64 == 1024, "plane rows; 32 bitmap words per (query, range)");
    extern __shared__ __attribute__((aligned(16))) float s_tab[];       // [S][16]
    __shared__ uint32_t s_queue[NWAVES][kRefineBitsQueue];
    __shared__ uint32_t s_out;
    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t T = a.thr[q];
    const uint32_t vb = a.vbase[(size_t)q * 2];                         // (P = 1: [nq][2])
    const uint32_t lb = ix.leaf_off[a.tokens[q]];
    const uint32_t slot = a.slot_of[q];
    if (tid == 0) s_out = 0;
    for (uint32_t e = tid; e < (uint32_t)S * 16u; e += kRefineBitsThreads)   // this query's table, de-interleaved: [s][16]
        s_tab[e] = slot == kInvalid ? 0.0f : a.lutq[((size_t)(slot >> 2) * S * 16 + e) * 4 + (slot & 3u)];
    __syncthreads();
    uint64_t *out = a.cand + (size_t)q * a.cap;
    const uint4 *row4 = reinterpret_cast<const uint4 *>(a.surv + (size_t)q * a.surv_stride);
    const uint32_t n4 = a.surv_stride / 4u;
    uint32_t *queue = s_queue[wave];

    // scores the n <= POP points queue[0 .. n) (n wave-uniform)
    auto score = [&](const uint32_t *pts, uint32_t n) {
        uint32_t j[U];
        bool ok[U];
        uint4 rw[U][SPW / 4];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            const uint32_t e = lane + 64u * u;
            ok[u] = e < n;
            j[u] = ok[u] ? pts[e] : 0u;
        }
        if (a.allow) {   // (block-uniform)
#pragma unroll
            for (uint32_t u = 0; u < U; ++u)
                ok[u] = ok[u] && row_allowed(ix, a.allow, a.allow_stride, q, a.allow_bits, lb + j[u]);
        }
#pragma unroll
        for (uint32_t u = 0; u < U; ++u)
#pragma unroll
            for (int x = 0; x < SPW / 4; ++x)
                rw[u][x] = reinterpret_cast<const uint4 *>(ix.codes_sp + (size_t)(lb + (ok[u] ? j[u] : 0u)) * SPW)[x];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            uint32_t w[SPW];
#pragma unroll
            for (int x = 0; x < SPW / 4; ++x) {
                w[4 * x] = rw[u][x].x; w[4 * x + 1] = rw[u][x].y; w[4 * x + 2] = rw[u][x].z; w[4 * x + 3] = rw[u][x].w;
            }
            SpRow<S> r;
            r.decode(w);
            float acc = 0.0f;
#pragma unroll
            for (int s2 = 0; s2 < S; ++s2) {
                const float tv = s_tab[s2 * 16 + r.code(s2)];
                acc = s2 == 0 ? tv : acc + tv;
            }
            const uint64_t key = make_key(acc, vb + j[u]);
            const bool keep = ok[u] && key <= T;
            uint32_t wtot;
            const uint32_t wpre = wave_prefix_count(keep, &wtot);
            uint32_t base = 0;
            if (lane == 0 && wtot) base = atomicAdd(&s_out, wtot);
            base = (uint32_t)__shfl((int)base, 0);
            if (keep && base + wpre < a.cap) out[base + wpre] = key;
        }
    };

    uint32_t qn = 0;   // points in the wave's queue (wave-uniform)
    uint4 nxt = wave * 64u + lane < n4 ? row4[wave * 64u + lane] : make_uint4(0u, 0u, 0u, 0u);
    for (uint32_t c = wave; c * 64u < n4; c += NWAVES) {
        uint32_t w[4] = {nxt.x, nxt.y, nxt.z, nxt.w};
        {
            const uint32_t i4 = (c + NWAVES) * 64u + lane;
            nxt = i4 < n4 ? row4[i4] : make_uint4(0u, 0u, 0u, 0u);
        }
        const uint32_t cnt = (uint32_t)(__popc(w[0]) + __popc(w[1]) + __popc(w[2]) + __popc(w[3]));
        const uint32_t incl = wave_incl_scan(cnt);
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        if (total == 0) continue;
        const uint32_t gw = (c * 64u + lane) * 4u;   // the lane's first word: range gw >> 5, words gw & 31 .. + 3
        const uint32_t p0 = (gw >> 5) * kSpRange64;
        uint32_t sq = incl - cnt;                    // the lane's next point in the chunk's order
        for (uint32_t base = 0; base < total;) {
            const uint32_t take = min(total - base, kRefineBitsQueue - qn);
            const uint32_t lim = base + take;
#pragma unroll
            for (uint32_t x = 0; x < 4; ++x) {
                const uint32_t wl = (gw & 31u) + x, tt = wl >> 1, h = wl & 1u;
                while (w[x] && sq < lim) {
                    const uint32_t bpos = (uint32_t)__ffs((int)w[x]) - 1u;
                    w[x] &= w[x] - 1u;
                    const uint32_t r = 15u - (bpos & 15u);
                    const uint32_t jrel = (2u * tt + (bpos >> 4)) * 32u + 4u * h + (r & 3u) + ((r >> 2) << 3);
                    queue[qn + sq - base] = p0 + jrel;
                    ++sq;
                }
            }
            qn += take;
            base = lim;
            __builtin_amdgcn_wave_barrier();
            while (qn >= POP) {
                qn -= POP;
                score(queue + qn, POP);
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (qn) score(queue, qn);   // (fewer than POP are left)
    __syncthreads();
    if (tid == 0) a.cand_cnt[q] = s_out;   // > cap: select_rerank reports the overflow
}

// =====================================================================================
// launchers
// =====================================================================================
// fold: lut8_build_kernel's mode (-1: plain tables before any bound exists, K5d; 1: the sparse prefilter's folded tables)
int launch_lut8_build(const TxhWork &w, uint32_t S, int fold, hipStream_t st) {
    SCANN_TRY(launch(lut8_build_kernel, dim3(w.max_quads), dim3(256), 0, st, S, w.lutq, w.counters, w.lut8,
                     reinterpret_cast<Lut8Meta *>(w.lut8_meta), w.pair_q, w.pair_thr, w.mfma_thr1, fold));
    return SCANN_HIP_OK;
}

// K6d / K6e + refine (4-bit codes)
int launch_prefilter_refine(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
    return with_codec(ix, [&](auto codec) -> int {
        using C = decltype(codec);
        if constexpr (C::BITS == 4) {
            const int cus = num_cus();
            SCANN_TRY(launch_lut8_build(w, (uint32_t)C::S, w.scan == TxhScan::Smfmac ? 1 : 0, st));
            const bool codes_in_list = w.codes_in_list;
            MfmaArgs ma;
            ma.thr1 = w.mfma_thr1;
            ma.pair_off = w.pair_off; ma.tile_off = w.tile_off; ma.pair_q = w.pair_q; ma.pair_vbase = w.pair_vbase;
            ma.counters = w.counters; ma.lut8 = w.lut8; ma.meta = reinterpret_cast<const Lut8Meta *>(w.lut8_meta);
            ma.pair_thr = w.pair_thr; ma.cand32_cnt = w.cand32_cnt; ma.cand32 = w.cand32; ma.cand32_codes = codes_in_list ? w.cand32_codes : nullptr; ma.cap32 = w.cap32;
            ma.allow = w.allow; ma.allow_bits = w.allow_bits;
            ma.surv = w.sp_bitmap ? w.surv : nullptr; ma.surv_stride = w.surv_stride;
            if (ev0) SCANN_HIP_CHECK(hipEventRecord(ev0, st));
            const bool words = w.sp_words;
            const dim3 mgrid((uint32_t)cus * 4u), mblock(kMfmaWaves * 64);   // 4 workgroups per CU (4 waves each)
            if (w.scan == TxhScan::Smfmac && w.sp_pairs64) {   // 64-pair items: two resident workgroups per CU
                if constexpr (C::S <= 32) {
                    if (words) return fail(SCANN_HIP_INTERNAL, "64-pair items take the lane-walk flush");
                    const dim3 grid64((uint32_t)cus * 2u);
                    if (w.sp_bitmap) SCANN_TRY(launch(adc_smfmac_bits_kernel64<C::S>, grid64, mblock, 0, st, ix, ma));
                    else if (w.allow && w.allow_stride) SCANN_TRY(launch(adc_smfmac_pq_kernel64<C::S>, grid64, mblock, 0, st, ix, ma, w.allow_stride));
                    else SCANN_TRY(launch(adc_smfmac_kernel64<C::S>, grid64, mblock, 0, st, ix, ma));
                } else {
                    return fail(SCANN_HIP_INTERNAL, "64-pair items are compiled for S <= 32");
                }
            } else if (w.allow && w.allow_stride) {   // one bitmap per query: the instantiation that forms the query's address
                void (*scan)(TxhIndexDev, MfmaArgs, uint64_t) =
                    w.scan == TxhScan::Mfma16   ? adc_mfma16_pq_kernel<C::S>
                    : w.scan == TxhScan::Mfma32 ? adc_mfma_pq_kernel<C::S>
                    : C::S <= 32                ? (words ? adc_smfmac_pq_kernel<C::S, true> : adc_smfmac_pq_kernel<C::S, false>)
                                                : (words ? adc_smfmac_wide_pq_kernel<C::S, true> : adc_smfmac_wide_pq_kernel<C::S, false>);
                SCANN_TRY(launch(scan, mgrid, mblock, 0, st, ix, ma, w.allow_stride));
            } else {
                void (*scan)(TxhIndexDev, MfmaArgs) =
                    w.scan == TxhScan::Mfma16   ? adc_mfma16_kernel<C::S>
                    : w.scan == TxhScan::Mfma32 ? adc_mfma_kernel<C::S>
                    : C::S <= 32                ? (words ? adc_smfmac_kernel<C::S, true> : adc_smfmac_kernel<C::S, false>)
                                                : (words ? adc_smfmac_wide_kernel<C::S, true> : adc_smfmac_wide_kernel<C::S, false>);
                SCANN_TRY(launch(scan, mgrid, mblock, 0, st, ix, ma));
            }
            if (ev1) SCANN_HIP_CHECK(hipEventRecord(ev1, st));
            RefineArgs ra;
            ra.P = w.P; ra.cap = w.cap; ra.cap32 = w.cap32; ra.tokens = w.tokens; ra.vbase = w.vbase;
            ra.slot_of = w.slot_of; ra.lutq = w.lutq; ra.thr = w.thr; ra.cand32_cnt = w.cand32_cnt;
            ra.cand32 = w.cand32; ra.cand32_codes = codes_in_list ? w.cand32_codes : nullptr; ra.cand_cnt = w.cand_cnt; ra.cand = w.cand; ra.counters = w.counters;
            ra.allow = w.allow; ra.allow_bits = w.allow_bits; ra.allow_stride = w.allow_stride;
            ra.planes = (w.scan == TxhScan::Smfmac && ra.cand32_codes) ? 1 : 0;
            ra.surv = ma.surv; ra.surv_stride = ma.surv_stride;
            if (w.sp_bitmap) {   // the scan left bitmaps, not lists
                if (w.scan != TxhScan::Smfmac || !w.sp_pairs64 || w.P != 1 || !ra.surv)
                    return fail(SCANN_HIP_INTERNAL, "survivor bitmaps are the 64-pair sparse prefilter's, P = 1");
                if constexpr (C::S <= 32) {   // (as the 64-pair items themselves)
                    SCANN_TRY(launch(adc_refine_bits_kernel<C>, dim3(w.nq), dim3(kRefineBitsThreads), (size_t)C::S * 16 * sizeof(float), st, ix, ra));
                    return SCANN_HIP_OK;
                } else {
                    return fail(SCANN_HIP_INTERNAL, "64-pair items are compiled for S <= 32");
                }
            }
            const size_t lds_rf = w.P <= kRefineTablesMax ? (size_t)w.P * C::S * 16 * sizeof(float) : 16;
            SCANN_TRY(launch(adc_refine_kernel<C>, dim3(w.nq), dim3(kRefineThreads), lds_rf, st, ix, ra));
            return SCANN_HIP_OK;
        } else {
            return fail(SCANN_HIP_INTERNAL, "the integer-MFMA prefilter takes 4-bit codes");
        }
    });
}

int launch_codes_sp_build(const uint32_t *d_codes, uint64_t n, uint32_t S, uint32_t *d_codes_sp, hipStream_t st) {
    if (n == 0) return SCANN_HIP_OK;
    SCANN_TRY(launch(codes_sp_build_kernel, dim3((uint32_t)ceil_div_u64(n, 256)), dim3(256), 0, st, d_codes, n, S, d_codes_sp));
    return SCANN_HIP_OK;
}

}  // namespace scann

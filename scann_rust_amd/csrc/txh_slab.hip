// txh_slab.hip -- K6s / K5s: the batched LUT16 scan and its sample pass for 4-bit indexes with 96 .. 512 subspaces
// (S a multiple of 32).  adc_scan_kernel<Codec<S, 4>> keeps all S/8 code words of a point in registers and a whole
// quad-interleaved table (S x 256 B) twice in LDS; at S = 384 that is 96 registers per point and 192 KB.  Here the
// subspaces are walked in SLABS of 32:
//
//   work item   (leaf chunk of scan_tile_points() = 512 points, group of <= kSlabQuads query quads): the gather scan's
//               geometry with qpt = kSlabQuads, cut by the same work-list kernels, pulled with grab_tile, decoded with
//               decode_item.
//   slab t      one uint4 of codes per point (subspaces 32 t .. 32 t + 31, Codec<32, 4>'s register form) and
//               32 x 16 float4 = 8 KB of table per quad.  Slabs are the OUTER loop, the item's quads the inner one: a
//               lane unpacks its two points' uint4 once and gathers with it from every quad's slab table, one
//               ds_read_b128 per (point, subspace, quad) serving four queries.  acc[quad][query][point] stays in
//               registers from the first slab to the last, so a point's codes are read once per work item.
//   tables      two buffers of kSlabQuads x 8 KB.  While slab t is gathered, slab t + 1 of every quad lands in the other
//               buffer by LDS-DMA (global_load_lds, destination = wave-uniform base + lane x 16) next to the lanes' next
//               uint4 of codes; one s_waitcnt vmcnt(0) and one barrier per slab.  lutq is [quad][s][16] float4, so a
//               quad's slab is 8 KB contiguous.
//   sum         lut[0][c0], then + lut[s][cs] for s ascending, every add on its own (-ffp-contract=off): the sequence
//               does not know where a slab ends, and it is the reference's (hashes/lut.rs:74-82).
//   filter      after the last slab: make_key, key <= T, row_allowed -- adc_scan_body's.  Survivors are staged per
//               (quad, query) in LDS; the flush reserves global slots with one returning atomic per query and copies
//               the lists out, 256 entries at a time.  A full stage falls back to the direct append.
//
// The sample pass is the same body: gather_slab() is the one function both kernels accumulate with, so the value a
// sample holds and the value the scan compares against the bound come from one instruction sequence.
#include "launch.h"
#include "txh_dev.h"
#include "txh_stages.h"

namespace scann {

namespace {

constexpr int kSlabLut4 = (int)kSlabSub * 16;                       // float4 of one quad's slab (8 KB)
constexpr int kSlabBuf4 = (int)kSlabQuads * kSlabLut4;              // ... of one buffer
using SlabCodec = Codec<(int)kSlabSub, 4>;                          // a slab's codes: 4 words, 8 registers
static_assert(SlabCodec::NWORDS == 4 && SlabCodec::PPT == 2, "a slab is one uint4 per point, two points per thread");
static_assert(2 * kSlabBuf4 * 16 <= 65536, "ds_read immediate offset");
static_assert(kSlabStage <= kScanThreads, "the flush copies one survivor per thread");

struct SlabArgs {
    const uint32_t *pair_off, *tile_off, *pair_q;
    uint32_t *counters;
    const float *lutq;
    uint32_t total_slot, queue_slot;   // counters[] slots: number of tiles, first of the eight tile queues
    const uint64_t *allow;             // optional allow-bitmap(s), bit = datapoint index
    uint64_t allow_bits, allow_stride;
    // scan
    const uint32_t *pair_vbase;
    const uint64_t *pair_thr;
    uint32_t *cand_cnt;
    uint64_t *cand;
    uint32_t cap;
    // sample
    const uint32_t *pair_sbase;
    uint32_t *samp;
    uint32_t scap, st;
};

constexpr size_t slab_lds_bytes(bool sample) {
    return (size_t)2 * kSlabBuf4 * 16 +
           (sample ? 0 : (size_t)kSlabQuads * 4 * kSlabStage * 8 + (size_t)3 * kSlabQuads * 4 * 4) + 16;
}
// two workgroups per CU: 2 x (64 KB of tables + 8.2 KB of stage) = 144.4 KB of the CU's 160
static_assert(2 * slab_lds_bytes(false) <= kMaxLdsBytes, "two scan workgroups per CU");

// Slab t of quads [0, nqd) of the item -> table buffer `buf` (LDS-DMA; not waited for here).
__device__ __forceinline__ void stage_slab(float4 *lut_s, const float4 *gl, uint32_t S, uint32_t nqd, uint32_t t,
                                           uint32_t buf, uint32_t tid) {
    for (uint32_t qi = 0; qi < nqd; ++qi) {
        const float4 *g = gl + (size_t)qi * S * 16 + (size_t)t * kSlabLut4;
        float4 *d = lut_s + buf * kSlabBuf4 + qi * kSlabLut4;
#pragma unroll
        for (int it = 0; it < kSlabLut4 / (int)kScanThreads; ++it) {
            const uint32_t e0 = (tid & ~63u) + it * kScanThreads;   // wave-uniform
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(g + e0 + (tid & 63u)),
                                             (__attribute__((address_space(3))) void *)(d + e0), 16, 0, 0);
        }
    }
}

// One slab of NP points of the lane against the tables of quads [0, nqd); bufoff: byte offset of the slab's table
// buffer (0 or 32 KB), OR-ed into the code's byte offset so that one copy of the code serves both buffers and the
// quad and subspace stay in the read's immediate.
template <int NP>
__device__ __forceinline__ void gather_slab(const float4 *lut_s, uint32_t bufoff, uint32_t nqd,
                                            uint32_t (&regs)[2][SlabCodec::REGS], float (&acc)[kSlabQuads][4][2]) {
    const char *lb = reinterpret_cast<const char *>(lut_s);
#pragma unroll
    for (int qi = 0; qi < (int)kSlabQuads; ++qi) {
        if ((uint32_t)qi < nqd) {   // wave-uniform
            // keep the byte extractions next to their reads (cf. scan_quad_compute: hoisted, they are 64 registers)
#pragma unroll
            for (int i = 0; i < NP; ++i)
#pragma unroll
                for (int ri = 0; ri < SlabCodec::REGS; ++ri) asm volatile("" : "+v"(regs[i][ri]));
            const char *lq = lb + qi * kSlabLut4 * 16;
            float4 v[2][NP];
#pragma unroll
            for (int i = 0; i < NP; ++i)
                v[0][i] = *reinterpret_cast<const float4 *>(lq + (SlabCodec::offset(regs[i], 0) | bufoff));
#pragma unroll
            for (int s = 0; s < (int)kSlabSub; ++s) {
                if (s + 1 < (int)kSlabSub) {
#pragma unroll
                    for (int i = 0; i < NP; ++i)
                        v[(s + 1) & 1][i] = *reinterpret_cast<const float4 *>(
                            lq + (s + 1) * SlabCodec::SUB_BYTES + (SlabCodec::offset(regs[i], s + 1) | bufoff));
                }
#pragma unroll
                for (int i = 0; i < NP; ++i) {
                    const float4 x = v[s & 1][i];
                    acc[qi][0][i] = acc[qi][0][i] + x.x;
                    acc[qi][1][i] = acc[qi][1][i] + x.y;
                    acc[qi][2][i] = acc[qi][2][i] + x.z;
                    acc[qi][3][i] = acc[qi][3][i] + x.w;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
}

// All slabs of one work item for NP points of the lane (rows crow[]): acc[quad][query][point] = lut[0][c0] + lut[1][c1] +
// ... in subspace order.  The sums start from -0: (-0) + x is x for every x, bit for bit (+0 would turn a -0 entry into
// +0), so subspace 0 needs no instruction sequence of its own and slab boundaries are invisible in the result.
// On entry no lane reads the table buffers; on exit a barrier has passed since the last read.
template <int NP>
__device__ __forceinline__ void walk_slabs(float4 *lut_s, const float4 *gl, uint32_t S, uint32_t nslabs, uint32_t nqd,
                                           const uint32_t *const (&crow)[2], uint32_t tid,
                                           float (&acc)[kSlabQuads][4][2]) {
#pragma unroll
    for (int qi = 0; qi < (int)kSlabQuads; ++qi)
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[qi][p][i] = -0.0f;
    uint4 raw[NP];
    stage_slab(lut_s, gl, S, nqd, 0, 0, tid);
#pragma unroll
    for (int i = 0; i < NP; ++i) raw[i] = *reinterpret_cast<const uint4 *>(crow[i]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (uint32_t t = 0; t < nslabs; ++t) {
        uint32_t regs[2][SlabCodec::REGS];
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const uint32_t w[4] = {raw[i].x, raw[i].y, raw[i].z, raw[i].w};
            SlabCodec::unpack(w, regs[i]);
        }
        if (t + 1 < nslabs) {   // slab t + 1: tables into the idle buffer, codes into raw; both land under the gather
            stage_slab(lut_s, gl, S, nqd, t + 1, (t + 1) & 1u, tid);
#pragma unroll
            for (int i = 0; i < NP; ++i) raw[i] = *reinterpret_cast<const uint4 *>(crow[i] + (size_t)(t + 1) * 4);
        }
        gather_slab<NP>(lut_s, (t & 1u) * (uint32_t)(kSlabBuf4 * 16), nqd, regs, acc);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the LDS-DMA prefetch and the next codes have landed
        __syncthreads();
    }
}

// SAMPLE = false: K6s, the scan.  SAMPLE = true: K5s, the scan's arithmetic over every st-th point of each selected leaf
// (adc_sample_kernel's tiles and outputs).
template <bool SAMPLE>
__device__ __forceinline__ void slab_body(const TxhIndexDev &ix, const SlabArgs &a) {
    extern __shared__ __attribute__((aligned(16))) float4 lut_s[];   // [2][kSlabQuads][kSlabLut4]
    constexpr int NL = (int)kSlabQuads * 4;                          // (quad, query) lists of an item
    uint64_t (*ckey_s)[kSlabStage] = reinterpret_cast<uint64_t (*)[kSlabStage]>(lut_s + 2 * kSlabBuf4);   // [NL]
    uint32_t *ccnt_s = SAMPLE ? reinterpret_cast<uint32_t *>(lut_s + 2 * kSlabBuf4)
                              : reinterpret_cast<uint32_t *>(ckey_s + NL);   // [NL] live counters (LDS atomics)
    uint32_t *cbase_s = ccnt_s + NL;                                         // [NL] global base slots of the flush
    uint32_t *cq_s = cbase_s + NL;                                           // [NL] query ids
    uint32_t &tile_sh = SAMPLE ? ccnt_s[0] : cq_s[NL];
    const uint32_t tid = threadIdx.x;
    const uint32_t total_tiles = a.counters[a.total_slot];
    const uint32_t S = ix.S, nw = ix.nw, nslabs = S / kSlabSub;
    const uint32_t st = SAMPLE ? a.st : 1u;
    if (!SAMPLE && tid < (uint32_t)NL) ccnt_s[tid] = 0;

    for (;;) {
        if (tid == 0) tile_sh = grab_tile(a.counters + a.queue_slot, total_tiles);
        __syncthreads();
        const uint32_t tile = __builtin_amdgcn_readfirstlane(tile_sh);
        if (tile == kInvalid) break;

        const WorkItem item = decode_item(ix, a.tile_off, a.pair_off, tile);
        const uint32_t lb = item.lb, slot0 = item.slot0;
        const uint32_t size = (item.size + st - 1) / st;            // points of the leaf this pass visits
        const uint32_t nquads = (item.slot_end - slot0) >> 2;
        const uint32_t nchunks = (size + kScanTP - 1) / kScanTP;
        if (nchunks == 0 || nquads == 0) {                           // (an empty leaf has no items)
            __syncthreads();
            continue;
        }
        const uint32_t chunk = item.local % nchunks, qg = item.local / nchunks;
        const uint32_t q0 = min(qg * kSlabQuads, nquads);
        const uint32_t nqd = min(kSlabQuads, nquads - q0);          // quads of this item
        const uint32_t c0 = chunk * kScanTP;
        const uint32_t npts = min(kScanTP, size - c0);
        const uint32_t nsub = (npts + kScanThreads - 1) / kScanThreads;

        // the lane's two points: row of the code array (a point past the end reads the leaf's first row and is dropped)
        const uint32_t *crow[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const uint32_t j = c0 + tid + kScanThreads * i;
            crow[i] = ix.codes + (size_t)(lb + (j < size ? j * st : 0u)) * nw;
        }
        const float4 *gl = reinterpret_cast<const float4 *>(a.lutq) + (size_t)((slot0 >> 2) + q0) * S * 16;

        float acc[kSlabQuads][4][2];
        if (nsub == 1) walk_slabs<1>(lut_s, gl, S, nslabs, nqd, crow, tid, acc);   // wave-uniform
        else walk_slabs<2>(lut_s, gl, S, nslabs, nqd, crow, tid, acc);

        if constexpr (SAMPLE) {
#pragma unroll
            for (int qi = 0; qi < (int)kSlabQuads; ++qi) {
                if ((uint32_t)qi >= nqd) continue;   // wave-uniform
                const uint32_t slot = slot0 + (q0 + qi) * 4;
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const uint32_t pq = uniform_load(a.pair_q + slot + p);
                    if (pq == kInvalid) continue;    // wave-uniform
                    uint32_t *dst = a.samp + (size_t)pq * a.scap + uniform_load(a.pair_sbase + slot + p);
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const uint32_t j = c0 + tid + kScanThreads * i;
                        if (i < (int)nsub && j < size)   // a sample of a row the query's list rejects is absent
                            dst[j] = row_allowed(ix, a.allow, a.allow_stride, pq, a.allow_bits, lb + j * st)
                                         ? f32_to_ordered(acc[qi][p][i]) : 0xFFFFFFFFu;
                    }
                }
            }
        } else {
            // threshold filter: survivors go to the LDS stage of their (quad, query)
#pragma unroll
            for (int qi = 0; qi < (int)kSlabQuads; ++qi) {
                if ((uint32_t)qi >= nqd) continue;   // wave-uniform
                const uint32_t slot = slot0 + (q0 + qi) * 4;
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const uint32_t pq = uniform_load(a.pair_q + slot + p);
                    if (pq == kInvalid) continue;    // wave-uniform: the padding of a partial quad
                    const uint64_t T = uniform_load(a.pair_thr + slot + p);
                    const uint32_t Thi = (uint32_t)(T >> 32);
                    const float Tf = (Thi == 0xFFFFFFFFu) ? __builtin_inff() : ordered_to_f32(Thi);
                    const uint32_t vb = uniform_load(a.pair_vbase + slot + p);
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        if (i < (int)nsub && acc[qi][p][i] <= Tf) {
                            const uint32_t j = c0 + tid + kScanThreads * i;
                            if (j < size) {
                                const uint64_t key = make_key(acc[qi][p][i], vb + j);
                                if (key <= T && row_allowed(ix, a.allow, a.allow_stride, pq, a.allow_bits, lb + j)) {
                                    const uint32_t sl = atomicAdd(&ccnt_s[qi * 4 + p], 1u);
                                    if (sl < kSlabStage) {
                                        ckey_s[qi * 4 + p][sl] = key;
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
            __syncthreads();
            // flush: one returning global atomic per (quad, query) list, then the lists, a thread per entry
            if (tid < (uint32_t)NL) {
                const uint32_t gn = min(ccnt_s[tid], kSlabStage);
                uint32_t gq = kInvalid, gbase = 0;
                if (gn) {   // (a list of a quad past nqd or of a padding slot is empty)
                    gq = a.pair_q[slot0 + q0 * 4 + tid];
                    gbase = atomicAdd(&a.cand_cnt[gq], gn);
                }
                ccnt_s[tid] = gn;
                cbase_s[tid] = gbase;
                cq_s[tid] = gq;
            }
            __syncthreads();
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                const uint32_t n_l = ccnt_s[l];
                if (tid < n_l) {
                    const uint32_t pos = cbase_s[l] + tid;
                    if (pos < a.cap) a.cand[(size_t)cq_s[l] * a.cap + pos] = ckey_s[l][tid];
                }
            }
            __syncthreads();
            if (tid < (uint32_t)NL) ccnt_s[tid] = 0;
        }
        __syncthreads();
    }
}

}  // namespace

// two workgroups of four waves per CU (LDS); 256 VGPRs a lane at that occupancy, of which the body takes about half
__global__ __launch_bounds__(kScanThreads, 2) void adc_slab_scan_kernel(TxhIndexDev ix, SlabArgs a) {
    slab_body<false>(ix, a);
}
__global__ __launch_bounds__(kScanThreads, 2) void adc_slab_sample_kernel(TxhIndexDev ix, SlabArgs a) {
    slab_body<true>(ix, a);
}

bool txh_slab_layout(const TxhIndexDev &ix) {
    return ix.code_bits == 4 && !ix.exact_scan && ix.S > 64 && ix.S <= kSlabMaxS && ix.S % kSlabSub == 0;
}

static int slab_args(const TxhIndexDev &ix, const TxhWork &w, bool sample, SlabArgs *out) {
    if (!txh_slab_layout(ix) || ix.nw != ix.S / 8)
        return fail(SCANN_HIP_INTERNAL, "the slab scan takes 4-bit codes with 96 .. 512 subspaces, a multiple of 32");
    if ((sample ? w.sqpt : w.qpt) != kSlabQuads || scan_tile_points(ix) != kScanTP)
        return fail(SCANN_HIP_INTERNAL, "the slab scan's work items are 512 points x 4 quads");
    SlabArgs a{};
    a.pair_off = w.pair_off; a.pair_q = w.pair_q; a.counters = w.counters; a.lutq = w.lutq;
    a.allow = w.allow; a.allow_bits = w.allow_bits; a.allow_stride = w.allow ? w.allow_stride : 0;
    if (sample) {
        a.tile_off = w.stile_off; a.total_slot = CNT_TOTAL_STILES; a.queue_slot = CNT_XS;
        a.pair_sbase = w.pair_sbase; a.samp = w.samp; a.scap = w.scap; a.st = w.st ? w.st : 1u;
    } else {
        a.tile_off = w.tile_off; a.total_slot = CNT_TOTAL_TILES; a.queue_slot = CNT_XQ;
        a.pair_vbase = w.pair_vbase; a.pair_thr = w.pair_thr; a.cand_cnt = w.cand_cnt; a.cand = w.cand; a.cap = w.cap;
        a.st = 1;
    }
    *out = a;
    return SCANN_HIP_OK;
}

int launch_slab_sample(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st) {
    SlabArgs a;
    SCANN_TRY(slab_args(ix, w, true, &a));
    return launch(adc_slab_sample_kernel, dim3((uint32_t)num_cus() * 2u), dim3(kScanThreads), slab_lds_bytes(true), st, ix, a);
}

int launch_slab_scan(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st) {
    SlabArgs a;
    SCANN_TRY(slab_args(ix, w, false, &a));
    return launch(adc_slab_scan_kernel, dim3((uint32_t)num_cus() * 2u), dim3(kScanThreads), slab_lds_bytes(false), st, ix, a);
}

}  // namespace scann

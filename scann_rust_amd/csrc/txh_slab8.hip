// txh_slab8.hip -- K6t / K5t: the batched ADC scan and its sample pass for byte-code indexes (16 < K <= 256, 256-slot
// tables) with 24 .. 128 subspaces, S a multiple of 8.  adc_scan_kernel<Codec<S, 8>> keeps all S/4 code words of 8
// points in registers and a whole quad-interleaved table (S x 4 KB) twice in LDS: 128 KB at S = 16, where with_codec
// stops.  Here the subspaces are walked in SLABS of 4:
//
//   work item   (leaf chunk of scan_tile_points() = 2048 points, group of <= kSlab8Quads = 2 query quads): the gather
//               scan's geometry with qpt = 2, cut by the same work-list kernels, pulled with grab_tile, decoded with
//               decode_item.  256 threads, 8 points a thread (Codec<., 8>::PPT): a byte-code table is 16x a LUT16
//               table per subspace, and the table bytes staged per gather are 4096 / points-per-item per subspace and
//               quad -- 2 B per 16 B gathered at 2048 points, 8 B at the 512 points of txh_slab.hip.
//   slab t      one u32 of codes per point (subspaces 4 t .. 4 t + 3) and 4 x 256 float4 = 16 KB of table per quad.
//               Slabs are the OUTER loop, the item's quads the inner one: a lane's code word is read once per item and
//               gathers from both quads' slab tables, one ds_read_b128 per (point, subspace, quad) serving four
//               queries.  acc[quad][query][point] (64 registers) lives from the first slab to the last.
//   tables      two buffers of kSlab8Quads x 16 KB = 64 KB.  While slab t is gathered, slab t + 1 of both quads lands in
//               the other buffer by LDS-DMA (global_load_lds, destination = wave-uniform base + lane x 16) next to the
//               lanes' next code words; one s_waitcnt vmcnt(0) and one barrier per slab.  lutq is [quad][s][256] float4,
//               so a quad's slab is 16 KB contiguous.  The buffer is a byte offset OR-ed into the code's byte offset:
//               one copy of the gather, the quad and the subspace in the read's immediate.
//   sum         lut[0][c0], then + lut[s][cs] for s ascending, every add on its own (-ffp-contract=off, no packed f32
//               forms): the accumulators start at -0, so neither subspace 0 nor a slab boundary has an instruction
//               sequence of its own, and the sequence is the reference's (hashes/lut.rs:74-82).
//   filter      after the last slab: make_key, key <= T, row_allowed -- adc_scan_body's.  Survivors are staged per
//               (quad, query) in LDS; the flush reserves global slots with one returning atomic per list and copies
//               the lists out, a thread per entry.  A full stage falls back to the direct append.
//
// The sample pass is the same body: gather_slab8() is the one function both kernels accumulate with, so the value a
// sample holds and the value the scan compares against the bound come from one instruction sequence.
#include "launch.h"
#include "txh_dev.h"
#include "txh_stages.h"

namespace scann {

namespace {

constexpr int kS8Pts = 8;                                            // points per thread (Codec<., 8>::PPT)
constexpr uint32_t kS8TP = kScanThreads * kS8Pts;                    // points per work item
constexpr int kS8Sub4 = 256;                                         // float4 of one subspace's table (4 KB)
constexpr int kS8Lut4 = (int)kSlab8Sub * kS8Sub4;                    // ... of one quad's slab (16 KB)
constexpr int kS8Buf4 = (int)kSlab8Quads * kS8Lut4;                  // ... of one buffer (32 KB)
constexpr int kS8Lists = (int)kSlab8Quads * 4;                       // (quad, query) lists of an item
static_assert(kSlab8Sub == 4, "a slab is one u32 of byte codes per point");
static_assert(Codec<8, 8>::PPT == kS8Pts && Codec<8, 8>::KP == kS8Sub4, "the byte-code tile of the work lists");
static_assert(2 * kS8Buf4 * 16 <= 65536, "ds_read immediate offset");
static_assert(kSlab8Stage <= kScanThreads, "the flush copies one survivor per thread");

struct Slab8Args {
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

constexpr size_t slab8_lds_bytes(bool sample) {
    return (size_t)2 * kS8Buf4 * 16 + (sample ? 0 : (size_t)kS8Lists * kSlab8Stage * 8 + (size_t)3 * kS8Lists * 4) + 16;
}
// two workgroups per CU: 2 x (64 KB of tables + 12.1 KB of stage) = 152.2 KB of the CU's 160
static_assert(2 * slab8_lds_bytes(false) <= kMaxLdsBytes, "two scan workgroups per CU");

// Slab t of quads [0, nqd) of the item -> table buffer `buf` (LDS-DMA; not waited for here).
__device__ __forceinline__ void stage_slab8(float4 *lut_s, const float4 *gl, uint32_t S, uint32_t nqd, uint32_t t,
                                            uint32_t buf, uint32_t tid) {
    for (uint32_t qi = 0; qi < nqd; ++qi) {
        const float4 *g = gl + (size_t)qi * S * kS8Sub4 + (size_t)t * kS8Lut4;
        float4 *d = lut_s + buf * kS8Buf4 + qi * kS8Lut4;
#pragma unroll
        for (int it = 0; it < kS8Lut4 / (int)kScanThreads; ++it) {
            const uint32_t e0 = (tid & ~63u) + it * kScanThreads;   // wave-uniform
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(g + e0 + (tid & 63u)),
                                             (__attribute__((address_space(3))) void *)(d + e0), 16, 0, 0);
        }
    }
}

// One slab of the lane's first 2 NG points against the tables of quads [0, nqd); cw[i]: point i's four byte codes;
// bufoff: byte offset of the slab's table buffer (0 or 32 KB), OR-ed into the code's byte offset.  The reads of a quad
// are one software pipeline over (point pair, subspace), one step deep as scan_quad_compute's: the two ds_read_b128 of
// step k + 1 are in flight while step k is added.  A point's four entries are added in subspace order.
template <int NG>
__device__ __forceinline__ void gather_slab8(const float4 *lut_s, uint32_t bufoff, uint32_t nqd, uint32_t (&cw)[kS8Pts],
                                             float (&acc)[kSlab8Quads][4][kS8Pts]) {
    const char *lb = reinterpret_cast<const char *>(lut_s);
    constexpr int NSTEP = NG * (int)kSlab8Sub;
#pragma unroll
    for (int qi = 0; qi < (int)kSlab8Quads; ++qi) {
        if ((uint32_t)qi < nqd) {   // wave-uniform
            // keep the byte extractions next to their reads (hoisted out of the quad loop they are 64 registers)
#pragma unroll
            for (int i = 0; i < 2 * NG; ++i) asm volatile("" : "+v"(cw[i]));
            const char *lq = lb + qi * kS8Lut4 * 16;
            float4 v[2][2];
            auto issue = [&](int k, int slot) {
                const int g = k / (int)kSlab8Sub, s = k % (int)kSlab8Sub;
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    v[slot][i] = *reinterpret_cast<const float4 *>(
                        lq + s * kS8Sub4 * 16 + ((((cw[2 * g + i] >> (8 * s)) & 0xFFu) << 4) | bufoff));
            };
            issue(0, 0);
#pragma unroll
            for (int k = 0; k < NSTEP; ++k) {
                if (k + 1 < NSTEP) issue(k + 1, (k + 1) & 1);
                const int g = k / (int)kSlab8Sub;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const float4 x = v[k & 1][i];
                    acc[qi][0][2 * g + i] = acc[qi][0][2 * g + i] + x.x;
                    acc[qi][1][2 * g + i] = acc[qi][1][2 * g + i] + x.y;
                    acc[qi][2][2 * g + i] = acc[qi][2][2 * g + i] + x.z;
                    acc[qi][3][2 * g + i] = acc[qi][3][2 * g + i] + x.w;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
}

// All slabs of one work item for the lane's first 2 NG points (code rows row[], in words of the code array):
// acc[quad][query][point] = lut[0][c0] + lut[1][c1] + ... in subspace order.  The sums start from -0: (-0) + x is x for
// every x, bit for bit (+0 would turn a -0 entry into +0).  Points from 2 NG on keep -0 and are never read.
// On entry no lane reads the table buffers; on exit a barrier has passed since the last read.
template <int NG>
__device__ __forceinline__ void walk_slabs8(float4 *lut_s, const float4 *gl, const uint32_t *codes, uint32_t S,
                                            uint32_t nslabs, uint32_t nqd, const uint32_t (&row)[kS8Pts], uint32_t tid,
                                            float (&acc)[kSlab8Quads][4][kS8Pts]) {
#pragma unroll
    for (int qi = 0; qi < (int)kSlab8Quads; ++qi)
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int i = 0; i < kS8Pts; ++i) acc[qi][p][i] = -0.0f;
    uint32_t raw[2 * NG];
    stage_slab8(lut_s, gl, S, nqd, 0, 0, tid);
#pragma unroll
    for (int i = 0; i < 2 * NG; ++i) raw[i] = codes[(size_t)row[i] * nslabs];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (uint32_t t = 0; t < nslabs; ++t) {
        uint32_t cw[kS8Pts];
#pragma unroll
        for (int i = 0; i < 2 * NG; ++i) cw[i] = raw[i];
        if (t + 1 < nslabs) {   // slab t + 1: tables into the idle buffer, codes into raw; both land under the gather
            stage_slab8(lut_s, gl, S, nqd, t + 1, (t + 1) & 1u, tid);
#pragma unroll
            for (int i = 0; i < 2 * NG; ++i) raw[i] = codes[(size_t)row[i] * nslabs + t + 1];
        }
        gather_slab8<NG>(lut_s, (t & 1u) * (uint32_t)(kS8Buf4 * 16), nqd, cw, acc);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the LDS-DMA prefetch and the next codes have landed
        __syncthreads();
    }
}

// SAMPLE = false: K6t, the scan.  SAMPLE = true: K5t, the scan's arithmetic over every st-th point of each selected leaf
// (adc_sample_kernel's tiles and outputs).
template <bool SAMPLE>
__device__ __forceinline__ void slab8_body(const TxhIndexDev &ix, const Slab8Args &a) {
    extern __shared__ __attribute__((aligned(16))) float4 lut_s[];   // [2][kSlab8Quads][kS8Lut4]
    constexpr int NL = kS8Lists;
    uint64_t (*ckey_s)[kSlab8Stage] = reinterpret_cast<uint64_t (*)[kSlab8Stage]>(lut_s + 2 * kS8Buf4);   // [NL]
    uint32_t *ccnt_s = SAMPLE ? reinterpret_cast<uint32_t *>(lut_s + 2 * kS8Buf4)
                              : reinterpret_cast<uint32_t *>(ckey_s + NL);   // [NL] live counters (LDS atomics)
    uint32_t *cbase_s = ccnt_s + NL;                                         // [NL] global base slots of the flush
    uint32_t *cq_s = cbase_s + NL;                                           // [NL] query ids
    uint32_t &tile_sh = SAMPLE ? ccnt_s[0] : cq_s[NL];
    const uint32_t tid = threadIdx.x;
    const uint32_t total_tiles = a.counters[a.total_slot];
    const uint32_t S = ix.S, nslabs = S / kSlab8Sub;                 // (== ix.nw: a slab is one word of a code row)
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
        const uint32_t nchunks = (size + kS8TP - 1) / kS8TP;
        if (nchunks == 0 || nquads == 0) {                           // (an empty leaf has no items)
            __syncthreads();
            continue;
        }
        const uint32_t chunk = item.local % nchunks, qg = item.local / nchunks;
        const uint32_t q0 = min(qg * kSlab8Quads, nquads);
        const uint32_t nqd = min(kSlab8Quads, nquads - q0);         // quads of this item
        const uint32_t c0 = chunk * kS8TP;
        const uint32_t npts = min(kS8TP, size - c0);
        const uint32_t nsub = (npts + kScanThreads - 1) / kScanThreads;

        // the lane's points: row of the code array (a point past the end reads the leaf's first row and is dropped)
        uint32_t row[kS8Pts];
#pragma unroll
        for (int i = 0; i < kS8Pts; ++i) {
            const uint32_t j = c0 + tid + kScanThreads * i;
            row[i] = lb + (j < size ? j * st : 0u);
        }
        const float4 *gl = reinterpret_cast<const float4 *>(a.lutq) + (size_t)((slot0 >> 2) + q0) * S * kS8Sub4;

        float acc[kSlab8Quads][4][kS8Pts];
        switch ((nsub + 1) >> 1) {   // wave-uniform: pairs of points, as scan_quad_dispatch
            case 1: walk_slabs8<1>(lut_s, gl, ix.codes, S, nslabs, nqd, row, tid, acc); break;
            case 2: walk_slabs8<2>(lut_s, gl, ix.codes, S, nslabs, nqd, row, tid, acc); break;
            case 3: walk_slabs8<3>(lut_s, gl, ix.codes, S, nslabs, nqd, row, tid, acc); break;
            default: walk_slabs8<4>(lut_s, gl, ix.codes, S, nslabs, nqd, row, tid, acc); break;
        }

        if constexpr (SAMPLE) {
#pragma unroll
            for (int qi = 0; qi < (int)kSlab8Quads; ++qi) {
                if ((uint32_t)qi >= nqd) continue;   // wave-uniform
                const uint32_t slot = slot0 + (q0 + qi) * 4;
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const uint32_t pq = uniform_load(a.pair_q + slot + p);
                    if (pq == kInvalid) continue;    // wave-uniform
                    uint32_t *dst = a.samp + (size_t)pq * a.scap + uniform_load(a.pair_sbase + slot + p);
#pragma unroll
                    for (int i = 0; i < kS8Pts; ++i) {
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
            for (int qi = 0; qi < (int)kSlab8Quads; ++qi) {
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
                    for (int i = 0; i < kS8Pts; ++i) {
                        if (i < (int)nsub && acc[qi][p][i] <= Tf) {
                            const uint32_t j = c0 + tid + kScanThreads * i;
                            if (j < size) {
                                const uint64_t key = make_key(acc[qi][p][i], vb + j);
                                if (key <= T && row_allowed(ix, a.allow, a.allow_stride, pq, a.allow_bits, lb + j)) {
                                    const uint32_t sl = atomicAdd(&ccnt_s[qi * 4 + p], 1u);
                                    if (sl < kSlab8Stage) {
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
                const uint32_t gn = min(ccnt_s[tid], kSlab8Stage);
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

// two workgroups of four waves per CU (LDS): 256 VGPRs a lane at that occupancy
__global__ __launch_bounds__(kScanThreads, 2) void adc_slab8_scan_kernel(TxhIndexDev ix, Slab8Args a) {
    slab8_body<false>(ix, a);
}
__global__ __launch_bounds__(kScanThreads, 2) void adc_slab8_sample_kernel(TxhIndexDev ix, Slab8Args a) {
    slab8_body<true>(ix, a);
}

bool txh_slab8_layout(const TxhIndexDev &ix) {
    return ix.code_bits == 8 && !ix.exact_scan && txh_slab8_shape(ix.S, ix.K);
}

static int slab8_args(const TxhIndexDev &ix, const TxhWork &w, bool sample, Slab8Args *out) {
    if (!txh_slab8_layout(ix) || ix.nw != ix.S / kSlab8Sub || ix.kp != (uint32_t)kS8Sub4)
        return fail(SCANN_HIP_INTERNAL, "the byte-code slab scan takes 8-bit codes with 24 .. 128 subspaces, a multiple of 8");
    if ((sample ? w.sqpt : w.qpt) != kSlab8Quads || scan_tile_points(ix) != kS8TP)
        return fail(SCANN_HIP_INTERNAL, "the byte-code slab scan's work items are 2048 points x 2 quads");
    Slab8Args a{};
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

int launch_slab8_sample(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st) {
    Slab8Args a;
    SCANN_TRY(slab8_args(ix, w, true, &a));
    return launch(adc_slab8_sample_kernel, dim3((uint32_t)num_cus() * 2u), dim3(kScanThreads), slab8_lds_bytes(true), st, ix, a);
}

int launch_slab8_scan(const TxhIndexDev &ix, const TxhWork &w, hipStream_t st) {
    Slab8Args a;
    SCANN_TRY(slab8_args(ix, w, false, &a));
    return launch(adc_slab8_scan_kernel, dim3((uint32_t)num_cus() * 2u), dim3(kScanThreads), slab8_lds_bytes(false), st, ix, a);
}

}  // namespace scann

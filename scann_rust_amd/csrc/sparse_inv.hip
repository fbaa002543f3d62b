// sparse_inv.hip -- the posting-list route of sparse brute force (DESIGN.md 3.3j "row-blocked postings"): the scan
// reads only the stored entries whose dimension the query holds, and still sums every (query, row) pair in the
// reference's order -- ascending dimension, one f32 multiply and one f32 add per shared dimension, from +0.0.
//
// Layout (scann_hip_sparse_build_postings, built on the device from the handle's CSR arrays):
//   rows are cut into blocks of kSparseBlockRows.  Block b owns directory entries [blk_dir[b], blk_dir[b + 1]):
//   dir_dim[j] the ascending distinct dimensions stored by the block's rows, dir_start[j] the first posting of
//   dimension j's list (the list ends where the next begins; dir_start[entries] = nnz).  Postings are two planes,
//   post_row u16 (the row inside its block) and post_val f32, ascending by row inside a list.
//     inv_keys_kernel   one wave per row: key (block << 32 | dimension), payload (row in block << 32 | value bits)
//     hipcub SortPairs  stable LSD radix sort by key: CSR's row order survives inside a list
//     hipcub Select     the positions where the key changes: one per directory entry
//     inv_dir_kernel    directory entries and the blocks' directory ranges from those positions
//     inv_split_kernel  the sorted payload cut into the two planes
//
// Scan (sparse_inv_scan_kernel, grid (queries, chunks of blocks), 16 waves), per block of the chunk:
//   lookup    thread t binary-searches the block's directory for query term t: the term's posting range, empty on a miss
//   ownership wave w owns rows [w B/16, (w + 1) B/16) of the block and their LDS accumulators: it zeroes them, adds to
//             them and reads them back, and no other wave touches them -- no barrier and no atomic guards a sum.
//             64 terms at a time, lane i cuts the wave's row range out of term i's list (two binary searches on the
//             u16 plane); the cuts go round by lane shuffle and the wave walks the terms in ascending dimension, its
//             lanes striding over a cut: acc[row] = acc[row] + q * x, unfused.  Rows of one list are distinct, so
//             lanes never meet; two terms are two instructions of one wave, and LDS serves a wave in program order.
//   epilogue  per owned row the measure's epilogue of sparse.hip, the allow bitmap, the key, and the append-and-
//             bitonic selection of sparse_dev.h with one buffer: every row of the block gets a key, touched or not.
// The chunk's k best keys go to partial[query][chunk][k]; sparse.hip's merge kernel finishes the search.
#include <hipcub/hipcub.hpp>

#include "launch.h"
#include "sparse_dev.h"

namespace scann {
namespace {

constexpr uint32_t kInvBuildThreads = 256;
constexpr uint32_t kB = kSparseBlockRows;

__global__ __launch_bounds__(kInvBuildThreads) void inv_keys_kernel(const uint64_t *__restrict__ off, const uint32_t *__restrict__ dims,
                                                                    const float *__restrict__ vals, uint32_t n,
                                                                    uint64_t *__restrict__ keys, uint64_t *__restrict__ pay) {
    const uint64_t row = (uint64_t)blockIdx.x * (kInvBuildThreads / 64) + (threadIdx.x >> 6);
    if (row >= n) return;
    const uint64_t hk = (row / kB) << 32, hp = (row % kB) << 32;
    for (uint64_t e = off[row] + (threadIdx.x & 63u); e < off[row + 1]; e += 64) {
        keys[e] = hk | dims[e];
        pay[e] = hp | __builtin_bit_cast(uint32_t, vals[e]);
    }
}

// position i of the sorted keys opens a posting list
struct InvIsHead {
    const uint64_t *keys;
    __host__ __device__ bool operator()(uint32_t i) const { return i == 0 || keys[i] != keys[i - 1]; }
};

// heads[j]: where directory entry j's list starts in the sorted keys.  blk_dir[b] becomes the first entry whose block
// is at least b: entry j writes it for the blocks after its predecessor's up to its own, the last entry for the rest.
__global__ __launch_bounds__(kInvBuildThreads) void inv_dir_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ heads,
                                                                   uint32_t ndir, uint32_t nnz, uint32_t blocks,
                                                                   uint32_t *__restrict__ dir_dim, uint32_t *__restrict__ dir_start,
                                                                   uint32_t *__restrict__ blk_dir) {
    const uint32_t j = blockIdx.x * kInvBuildThreads + threadIdx.x;
    if (j >= ndir) return;
    const uint32_t s = heads[j];
    const uint64_t key = keys[s];
    const uint32_t b = (uint32_t)(key >> 32);
    dir_dim[j] = (uint32_t)key;
    dir_start[j] = s;
    for (uint32_t bb = j ? (uint32_t)(keys[heads[j - 1]] >> 32) + 1u : 0u; bb <= b; ++bb) blk_dir[bb] = j;
    if (j == ndir - 1) {
        dir_start[ndir] = nnz;
        for (uint32_t bb = b + 1; bb <= blocks; ++bb) blk_dir[bb] = ndir;
    }
}

__global__ __launch_bounds__(kInvBuildThreads) void inv_split_kernel(const uint64_t *__restrict__ pay, uint32_t nnz,
                                                                     uint16_t *__restrict__ post_row, float *__restrict__ post_val) {
    const uint32_t i = blockIdx.x * kInvBuildThreads + threadIdx.x;
    if (i >= nnz) return;
    const uint64_t p = pay[i];
    post_row[i] = (uint16_t)(p >> 32);
    post_val[i] = __builtin_bit_cast(float, (uint32_t)p);
}

struct InvScanArgs {
    // postings
    const uint32_t *blk_dir, *dir_dim, *dir_start;
    const uint16_t *post_row;
    const float *post_val;
    const float *row_norm;
    const uint32_t *row_len;
    uint32_t n, blocks;
    int measure;
    uint32_t cap_log;
    SparseInvArgs q;
};

// first position of [lo, hi) whose row is at least v (rows ascend inside a list)
__device__ __forceinline__ uint32_t inv_lower_bound(const uint16_t *__restrict__ rows, uint32_t lo, uint32_t hi, uint32_t v) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (rows[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// orders the wave's LDS accesses on either side of it: what one lane stored, another lane's later access sees
__device__ __forceinline__ void inv_wave_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one posting's step of its row's accumulator.  mode 0: the f32 sum (the multiply and the add are never fused);
// mode 1: the count of shared dimensions; mode 2: of those where both values are non-zero (qv is then 1.0 or 0.0)
__device__ __forceinline__ void inv_add(uint32_t *acc, int mode, uint32_t row, float qv, float x) {
    if (mode == 0) {
        float *f = reinterpret_cast<float *>(acc);
        f[row] = __fadd_rn(f[row], __fmul_rn(qv, x));
    } else {
        acc[row] += (mode == 1 || (qv != 0.0f && x != 0.0f)) ? 1u : 0u;
    }
}

template <bool SELECT, bool STATS>
__global__ __launch_bounds__(kSparseThreads) void sparse_inv_scan_kernel(const InvScanArgs a) {
    extern __shared__ __align__(16) unsigned char inv_lds[];
    uint32_t *acc = reinterpret_cast<uint32_t *>(inv_lds);       // [kB]: f32 sums or u32 counts
    uint32_t *t_lo = acc + kB;                                   // [kSparseSlots]: term t's postings in this block
    uint32_t *t_hi = t_lo + kSparseSlots;
    float *t_q = reinterpret_cast<float *>(t_hi + kSparseSlots); // [kSparseSlots]: the query's value of term t
    uint64_t *buf = reinterpret_cast<uint64_t *>(t_q + kSparseSlots);   // [1 << cap_log]
    __shared__ uint32_t s_cnt[1];
    __shared__ uint64_t s_thr[1];

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t q = blockIdx.x, chunk = blockIdx.y;
    const int measure = a.measure;
    const int mode = (measure == SCANN_HIP_SPARSE_JACCARD || measure == SCANN_HIP_SPARSE_DICE) ? 1
                     : measure == SCANN_HIP_SPARSE_NONZERO_INTERSECT                           ? 2
                                                                                               : 0;
    const uint64_t qo = a.q.q_off[q];
    const uint32_t qlen = (uint32_t)(a.q.q_off[q + 1] - qo);   // (at most kSparseSlots: the driver's check)
    const float qn2 = a.q.q_norm[q];
    uint32_t my_dim = 0;
    if (tid < qlen) {
        my_dim = a.q.q_dims[qo + tid];
        const float v = a.q.q_vals[qo + tid];
        t_q[tid] = mode == 0 ? v : (mode == 1 || v != 0.0f) ? 1.0f : 0.0f;
    }
    if (tid == 0) {
        s_cnt[0] = 0;
        s_thr[0] = SCANN_KEY_MAX;
    }
    const uint32_t b0 = chunk * a.q.chunk_blocks;
    const uint32_t b1 = min(b0 + a.q.chunk_blocks, a.blocks);
    const uint32_t w0 = wave * kSparseWaveRows;   // the wave's first row of a block
    const uint32_t cap_log = a.cap_log;
    unsigned long long visited = 0;

    for (uint32_t b = b0; b < b1; ++b) {
        __syncthreads();   // every wave has cut the previous block's ranges
        if (tid < qlen) {
            uint32_t lo = a.blk_dir[b], hi = a.blk_dir[b + 1];
            const uint32_t end = hi;
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (a.dir_dim[mid] < my_dim) lo = mid + 1;
                else hi = mid;
            }
            const bool hit = lo < end && a.dir_dim[lo] == my_dim;   // below the first, above the last, between two: a miss
            t_lo[tid] = hit ? a.dir_start[lo] : 0u;
            t_hi[tid] = hit ? a.dir_start[lo + 1] : 0u;
        }
        __syncthreads();

        for (uint32_t i = lane; i < kSparseWaveRows; i += 64) acc[w0 + i] = 0u;   // (+0.0f or the count 0)
        for (uint32_t t0 = 0; t0 < qlen; t0 += 64) {
            const uint32_t t = t0 + lane, nt = min(64u, qlen - t0);
            uint32_t lo = 0, hi = 0;
            float qv = 0.0f;
            if (t < qlen) {
                lo = t_lo[t];
                hi = t_hi[t];
                qv = t_q[t];
            }
            const uint32_t clo = inv_lower_bound(a.post_row, lo, hi, w0);
            const uint32_t chi = inv_lower_bound(a.post_row, clo, hi, w0 + kSparseWaveRows);
            if (STATS) visited += chi - clo;
            // term i's cut, and its first stride fetched while term i - 1 is added
            uint32_t c0 = (uint32_t)__shfl((int)clo, 0), c1 = (uint32_t)__shfl((int)chi, 0);
            float qi = __shfl(qv, 0);
            uint32_t r = 0;
            float x = 0.0f;
            if (lane < c1 - c0) {   // (positions are compared as lengths: c0 + lane may pass 2^32)
                r = a.post_row[c0 + lane];
                if (mode != 1) x = a.post_val[c0 + lane];
            }
            for (uint32_t i = 0; i < nt; ++i) {
                const uint32_t nx = min(i + 1, 63u);   // (every lane shuffles; past the last term the cut is emptied)
                uint32_t n0 = (uint32_t)__shfl((int)clo, (int)nx), n1 = (uint32_t)__shfl((int)chi, (int)nx);
                const float nq = __shfl(qv, (int)nx);
                if (i + 1 >= nt) n0 = n1 = 0u;
                uint32_t nr = 0;
                float nxv = 0.0f;
                if (lane < n1 - n0) {
                    nr = a.post_row[n0 + lane];
                    if (mode != 1) nxv = a.post_val[n0 + lane];
                }
                if (c0 < c1) {   // (uniform)
                    inv_wave_order();   // after the zeroing and after the term before
                    if (lane < c1 - c0) inv_add(acc, mode, r, qi, x);
                    for (uint32_t o = 64 + lane; o < c1 - c0; o += 64)   // (a cut holds at most kSparseWaveRows postings)
                        inv_add(acc, mode, a.post_row[c0 + o], qi, mode != 1 ? a.post_val[c0 + o] : 0.0f);
                }
                c0 = n0;
                c1 = n1;
                qi = nq;
                r = nr;
                x = nxv;
            }
        }
        inv_wave_order();

        // the owned rows, 64 at a time: one round of the workgroup is one row per thread
        for (uint32_t r0 = 0; r0 < kSparseWaveRows; r0 += 64) {
            const uint32_t local = w0 + r0 + lane;
            const uint64_t row = (uint64_t)b * kB + local;
            if (row < a.n) {
                const uint32_t rw = (uint32_t)row;
                const float av = mode == 0 ? reinterpret_cast<const float *>(acc)[local] : (float)acc[local];
                const uint32_t xlen = mode == 1 ? a.row_len[rw] : 0u;
                const float xn2 = measure == SCANN_HIP_COSINE ? a.row_norm[rw] : 0.0f;
                const float dist = sparse_distance(measure, av, xlen, xn2, qlen, qn2);
                if (!SELECT) {
                    a.q.out[(size_t)q * a.n + rw] = dist;
                } else if (!a.q.allow || (rw < a.q.allow_bits && ((a.q.allow[rw >> 6] >> (rw & 63u)) & 1ull))) {
                    const uint64_t key = make_key(dist, rw);
                    // (the buffer has room: it held at most cap - kSparseThreads keys when the round began)
                    if (key < s_thr[0]) buf[atomicAdd(&s_cnt[0], 1u)] = key;
                }
            }
            if (SELECT) {
                __syncthreads();   // the round's appends are done
                const int full = __syncthreads_or(tid == 0 && s_cnt[0] > (1u << cap_log) - kSparseThreads);
                if (full) sparse_compact<1>(buf, cap_log, a.q.k, s_cnt, s_thr);
            }
        }
    }
    if (SELECT) {
        __syncthreads();
        sparse_compact<1>(buf, cap_log, a.q.k, s_cnt, s_thr);
        for (uint32_t i = tid; i < a.q.k; i += kSparseThreads) a.q.partial[((size_t)q * a.q.chunks + chunk) * a.q.k + i] = buf[i];
    }
    if (STATS) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) visited += shfl_xor_t<uint64_t>(visited, o);
        if (lane == 0) atomicAdd(&a.q.stats[0], visited);
    }
}

}  // namespace

int sparse_inv_scan(scann_hip_sparse_index *ix, const SparseInvArgs &q) {
    InvScanArgs a{};
    a.blk_dir = ix->inv_blk_dir.as<uint32_t>();
    a.dir_dim = ix->inv_dir_dim.as<uint32_t>();
    a.dir_start = ix->inv_dir_start.as<uint32_t>();
    a.post_row = ix->inv_rows.as<uint16_t>();
    a.post_val = ix->inv_vals.as<float>();
    a.row_norm = ix->d_norm.as<float>();
    a.row_len = ix->d_len.as<uint32_t>();
    a.n = (uint32_t)ix->n;
    a.blocks = ix->inv_blocks;
    a.measure = ix->measure;
    a.q = q;
    const bool select = q.out == nullptr;
    while ((1u << a.cap_log) < sparse_inv_select_cap(q.k)) ++a.cap_log;
    const dim3 grid(q.nq, q.chunks), block(kSparseThreads);
    const size_t lds = sparse_inv_lds(q.k, select);
    if (select) {
        if (q.stats) return launch(sparse_inv_scan_kernel<true, true>, grid, block, lds, ix->stream, a);
        return launch(sparse_inv_scan_kernel<true, false>, grid, block, lds, ix->stream, a);
    }
    if (q.stats) return launch(sparse_inv_scan_kernel<false, true>, grid, block, lds, ix->stream, a);
    return launch(sparse_inv_scan_kernel<false, false>, grid, block, lds, ix->stream, a);
}

}  // namespace scann

using namespace scann;

extern "C" {

int scann_hip_sparse_build_postings(scann_hip_sparse_index *ix) {
    if (!ix) return fail(SCANN_HIP_INVALID_ARGUMENT, "index is null");
    std::lock_guard<std::mutex> lock(ix->mu);
    if (ix->inv) return SCANN_HIP_OK;
    if (ix->nnz >= 0xFFFFFFFFull) return fail(SCANN_HIP_UNIMPLEMENTED, "postings of more than 2^32 - 2 stored entries: offsets are u32");
    const uint32_t n = (uint32_t)ix->n, nnz = (uint32_t)ix->nnz;
    const uint32_t blocks = (uint32_t)ceil_div_u64(ix->n, kB);
    if (n == 0) {
        ix->inv = true;
        return SCANN_HIP_OK;
    }
    SCANN_HIP_CHECK(hipSetDevice(ix->device));
    hipStream_t st = ix->stream;
    DevBuf blk_dir, dir_dim, dir_start, post_row, post_val;
    SCANN_TRY(blk_dir.ensure(((size_t)blocks + 1) * 4));
    SCANN_TRY(post_row.ensure((size_t)nnz * 2));
    SCANN_TRY(post_val.ensure((size_t)nnz * 4));
    uint32_t ndir = 0;
    if (nnz) {
        DevBuf keys, pay, skeys, spay, heads, count, tmp;
        SCANN_TRY(keys.ensure((size_t)nnz * 8));
        SCANN_TRY(pay.ensure((size_t)nnz * 8));
        SCANN_TRY(skeys.ensure((size_t)nnz * 8));
        SCANN_TRY(spay.ensure((size_t)nnz * 8));
        SCANN_TRY(heads.ensure((size_t)nnz * 4));
        SCANN_TRY(count.ensure(4));
        SCANN_TRY(launch(inv_keys_kernel, dim3(ceil_div_u32(n, kInvBuildThreads / 64)), dim3(kInvBuildThreads), 0, st,
                         ix->d_off.as<uint64_t>(), ix->d_dims.as<uint32_t>(), ix->d_vals.as<float>(), n, keys.as<uint64_t>(), pay.as<uint64_t>()));
        int end_bit = 32;
        while (end_bit < 64 && ((uint64_t)(blocks - 1) >> (end_bit - 32))) ++end_bit;
        size_t sort_bytes = 0, select_bytes = 0;
        const InvIsHead is_head{skeys.as<uint64_t>()};
        hipcub::CountingInputIterator<uint32_t> positions(0u);
        SCANN_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, keys.as<uint64_t>(), skeys.as<uint64_t>(), pay.as<uint64_t>(),
                                                           spay.as<uint64_t>(), (uint64_t)nnz, 0, end_bit, st));
        SCANN_HIP_CHECK(hipcub::DeviceSelect::If(nullptr, select_bytes, positions, heads.as<uint32_t>(), count.as<uint32_t>(), (int64_t)nnz,
                                                 is_head, st));
        SCANN_TRY(tmp.ensure(sort_bytes > select_bytes ? sort_bytes : select_bytes));
        SCANN_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp.p, sort_bytes, keys.as<uint64_t>(), skeys.as<uint64_t>(), pay.as<uint64_t>(),
                                                           spay.as<uint64_t>(), (uint64_t)nnz, 0, end_bit, st));
        SCANN_HIP_CHECK(hipcub::DeviceSelect::If(tmp.p, select_bytes, positions, heads.as<uint32_t>(), count.as<uint32_t>(), (int64_t)nnz,
                                                 is_head, st));
        SCANN_HIP_CHECK(hipMemcpyAsync(&ndir, count.p, 4, hipMemcpyDeviceToHost, st));
        SCANN_HIP_CHECK(hipStreamSynchronize(st));
        SCANN_TRY(dir_dim.ensure((size_t)ndir * 4));
        SCANN_TRY(dir_start.ensure(((size_t)ndir + 1) * 4));
        SCANN_TRY(launch(inv_dir_kernel, dim3(ceil_div_u32(ndir, kInvBuildThreads)), dim3(kInvBuildThreads), 0, st, skeys.as<uint64_t>(),
                         heads.as<uint32_t>(), ndir, nnz, blocks, dir_dim.as<uint32_t>(), dir_start.as<uint32_t>(), blk_dir.as<uint32_t>()));
        SCANN_TRY(launch(inv_split_kernel, dim3(ceil_div_u32(nnz, kInvBuildThreads)), dim3(kInvBuildThreads), 0, st, spay.as<uint64_t>(), nnz,
                         post_row.as<uint16_t>(), post_val.as<float>()));
        SCANN_HIP_CHECK(hipStreamSynchronize(st));   // the temporaries go with this scope
    } else {   // rows without entries: every directory is empty
        SCANN_TRY(dir_dim.ensure(4));
        SCANN_TRY(dir_start.ensure(4));
        SCANN_HIP_CHECK(hipMemsetAsync(blk_dir.p, 0, ((size_t)blocks + 1) * 4, st));
        SCANN_HIP_CHECK(hipMemsetAsync(dir_start.p, 0, 4, st));
        SCANN_HIP_CHECK(hipStreamSynchronize(st));
    }
    ix->inv_blk_dir.take(blk_dir);
    ix->inv_dir_dim.take(dir_dim);
    ix->inv_dir_start.take(dir_start);
    ix->inv_rows.take(post_row);
    ix->inv_vals.take(post_val);
    ix->inv_blocks = blocks;
    ix->inv_bytes = ix->inv_blk_dir.bytes + ix->inv_dir_dim.bytes + ix->inv_dir_start.bytes + ix->inv_rows.bytes + ix->inv_vals.bytes;
    ix->inv = true;
    return SCANN_HIP_OK;
}

void scann_hip_sparse_postings_info(scann_hip_sparse_index *ix, uint64_t *out) {
    if (!out) return;
    for (int i = 0; i < 5; ++i) out[i] = 0;
    out[1] = kB;
    if (!ix) return;
    std::lock_guard<std::mutex> lock(ix->mu);
    out[0] = ix->inv_blocks;
    out[2] = ix->inv_bytes;
    out[3] = ix->inv_chunks;
    out[4] = ix->inv_visited;
}

}  // extern "C"

// ktree.hip -- the hierarchical partitioner (ktree.h): every node of one tree level trains in lockstep, so the number
// of launches per k-means++ round and per Lloyd iteration does not depend on how many nodes the level has.
//
// LEVEL ORDER.  A level keeps its rows as a permutation idx[] of the datapoints in (node, ascending datapoint) order:
// node y is the contiguous slice [base, base + cnt) of positions.  Rows are GATHERED through idx (never copied into
// level order); min_d, the assignment and the distances are indexed by position.  A node is cut into TILES of 256
// consecutive positions, counted from the node's own base, so no tile straddles two nodes and tile t of a node holds
// exactly the values block t of km_sum_f64_kernel sums when the primitive runs on a handle of the node's rows alone.
// Every node of a level that trains has more than num_children members, so all of them train k = num_children centres.
//
//   kt_mind_kernel        one k-means++ round: min_d against the node's newest pick + the tile's f64 partial sum
//   kt_pick_kernel        km_total_pick_kernel per node: total in the primitive's chunk order, the D^2 pick
//   kt_assign_kernel      assign_nearest_kernel per tile against the tile's node's centres (sequential scalar order)
//   kt_assign_avx_kernel  assign_nearest_avx_kernel, the same way (dim >= simd_threshold)
//                         both add the tile's partial sum and the node's smallest positive term (inertia)
//   kt_step_kernel        per node: total, the exactness test, the sequential chain where it fails, fit_single's stop
//   kt_update_kernel      km_update_kernel with one workgroup per (cluster, node); also the leaf centres
//   kt_* (small)          keys / offsets / gathers of the centre update and of the next level's order
//
// Centre update and next level: ONE stable radix sort of (key0[node] + cluster -> position); key0 is a prefix sum over
// the level's nodes in order (num_children keys for a node that trains, one for a node that already is a leaf), so
// the sorted positions are (node, cluster, ascending datapoint): the members of every cluster for the update, and,
// after the final assignment, the next level's order with every child a contiguous slice -- a parent that became a
// leaf keeps its place, so the last level's node order is collect_leaves' depth-first order and its idx[] is the CSR.
//
// The level's node table (at most 16384 entries of 16 bytes) is kept by the HOST: it reads the cluster offsets once
// per level and the per-node stop records once per iteration, and uploads the tile list it derives from the node
// sizes.  No row, distance or assignment crosses to the host.
#include "ktree.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "launch.h"
#include "txh.h"

namespace scann {

namespace {

constexpr uint32_t kKtTile = 256;   // positions per tile == values per block of km_sum_f64_kernel
constexpr int kKtTC = 16, kKtTCWide = 8, kKtDJ = 32, kKtAvxTC = 8;   // assign_nearest_kernel's / _avx_kernel's tiles
constexpr uint32_t kKtUpdFloats = 8192;   // km_update_kernel's staged tile
constexpr uint32_t kKtSeqVals = 4096;     // km_sum_f64_sequential_kernel's staged values

struct KtTile {
    uint32_t node, first, cnt;   // training node, first position, positions (1..256)
};
struct KtTrain {                 // a node that trains at this level (or, for the leaf centres, a leaf)
    uint32_t base, cnt, tile0, key0;
};
struct KtNode {                  // every node of the level, in order
    uint32_t base, key0, train, pad;
};
// per-node record of the Lloyd loop (device resident; the host reads the block once per iteration)
struct KtState {
    double prev, inertia;
    uint32_t iters, converged, frozen, pad;
};
struct KtLevel {
    const uint32_t *idx;
    const KtTile *tiles;
    const KtTrain *tr;
    const KtState *st;       // null: no node is skipped
    const float *centers;    // [training node][C][dim]
    uint32_t C;
};

// km_sum_f64_kernel's block: x of thread t is value t of the tile (0 past its end); s: LDS double[256]
__device__ __forceinline__ void kt_block_sum(float x, double *s, double *partial_out, uint32_t *min_pos_bits) {
    s[threadIdx.x] = (double)x;
    if (min_pos_bits) {   // kernel-uniform
        uint32_t b = x > 0.0f ? __float_as_uint(x) : 0xFFFFFFFFu;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) b = min(b, (uint32_t)__shfl_xor((int)b, o));
        if ((threadIdx.x & 63u) == 0 && b != 0xFFFFFFFFu) atomicMin(min_pos_bits, b);
    }
    __syncthreads();
    for (uint32_t o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *partial_out = s[0];
}

__global__ void kt_iota_kernel(uint32_t *__restrict__ idx, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) idx[i] = (uint32_t)i;
}

// the first seed of every node: stream output 0 mod n_node (kmeans.rs:305-306)
__global__ void kt_first_pick_kernel(const KtTrain *__restrict__ tr, uint32_t T, uint64_t z0, uint32_t C,
                                     uint32_t *__restrict__ picks) {
    const uint32_t y = blockIdx.x * blockDim.x + threadIdx.x;
    if (y < T) picks[(size_t)y * C] = (uint32_t)(z0 % tr[y].cnt);
}

// km_mind_update_kernel over a tile, against member picks[node][c - 1] of the tile's node; the tile's partial sum
__global__ __launch_bounds__(256) void kt_mind_kernel(BfIndexDev ix, KtLevel lv, const uint32_t *__restrict__ picks,
                                                      uint32_t c, int first, int avx, float *__restrict__ min_d,
                                                      double *__restrict__ partials) {
    __shared__ double s[256];
    const KtTile tl = lv.tiles[blockIdx.x];
    float v = 0.0f;
    if (threadIdx.x < tl.cnt) {
        const uint32_t p = tl.first + threadIdx.x;
        const uint32_t sel = lv.idx[lv.tr[tl.node].base + picks[(size_t)tl.node * lv.C + c - 1]];
        const float *row = ix.rows + (uint64_t)lv.idx[p] * ix.stride, *y = ix.rows + (uint64_t)sel * ix.stride;
        float d = 0.0f;
        uint32_t j = 0;
        if (avx) {
            float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            for (; j + 8 <= ix.dim; j += 8) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float t = row[j + u] - y[j + u];
                    acc[u] = fmaf(t, t, acc[u]);
                }
            }
            d = ((acc[0] + acc[4]) + (acc[1] + acc[5])) + ((acc[2] + acc[6]) + (acc[3] + acc[7]));
        } else if (((ix.stride & 3u) == 0) && ((reinterpret_cast<uintptr_t>(ix.rows) & 15u) == 0)) {
            for (; j + 4 <= ix.dim; j += 4) {   // 16-byte loads, same sequential sum
                const float4 a = *reinterpret_cast<const float4 *>(row + j);
                const float4 b = *reinterpret_cast<const float4 *>(y + j);
                float t = a.x - b.x; d = d + t * t;
                t = a.y - b.y; d = d + t * t;
                t = a.z - b.z; d = d + t * t;
                t = a.w - b.w; d = d + t * t;
            }
        }
        for (; j < ix.dim; ++j) {
            const float t = row[j] - y[j];
            d = d + t * t;
        }
        v = (first || d < min_d[p]) ? d : min_d[p];
        min_d[p] = v;
    }
    kt_block_sum(v, s, partials + blockIdx.x, nullptr);
}

// km_total_pick_kernel for node blockIdx.x: its tiles' partials in the primitive's chunk order, then the pick among its
// members; the draw is (u, zfb mod n_node).  picks[node][c] receives the member number.
__global__ __launch_bounds__(256) void kt_pick_kernel(const KtTrain *__restrict__ tr, const double *__restrict__ partials,
                                                      const float *__restrict__ min_d, double u, uint64_t zfb,
                                                      uint32_t C, uint32_t c, uint32_t *__restrict__ picks) {
    __shared__ double s_chunk[256];
    __shared__ float s_vals[256];
    __shared__ uint32_t s_blk;
    __shared__ double s_cum, s_total;
    const uint32_t t = threadIdx.x;
    const KtTrain nd = tr[blockIdx.x];
    const uint32_t n = nd.cnt, nb = (n + 255u) / 256u;
    partials += nd.tile0;
    min_d += nd.base;
    uint32_t *pick_out = picks + (size_t)blockIdx.x * C + c;
    const uint32_t per = (nb + 255u) / 256u;
    const uint32_t b0 = min(nb, t * per), b1 = min(nb, b0 + per);
    double mine = 0.0;
    for (uint32_t b = b0; b < b1; ++b) mine += partials[b];
    s_chunk[t] = mine;
    __syncthreads();
    if (t == 0) {
        double total = 0.0;
        for (uint32_t q = 0; q < 256; ++q) total += s_chunk[q];
        s_total = total;
        s_blk = 0xFFFFFFFFu;
        if (!(total > 0.0)) {
            *pick_out = (uint32_t)(zfb % n);
        } else {
            const double thr = u * total;
            double cum = 0.0;
            uint32_t q = 0;
            for (; q + 1 < 256; ++q) {   // chunk holding the threshold
                if (cum + s_chunk[q] >= thr) break;
                cum += s_chunk[q];
            }
            uint32_t b = min(nb, q * per);
            const uint32_t be = min(nb, b + per);
            for (; b + 1 < be; ++b) {    // tile inside the chunk
                if (cum + partials[b] >= thr) break;
                cum += partials[b];
            }
            s_blk = min(b, nb - 1);
            s_cum = cum;
        }
    }
    __syncthreads();
    if (s_blk == 0xFFFFFFFFu) return;
    const uint32_t i0 = s_blk * 256u;
    s_vals[t] = (i0 + t < n) ? min_d[i0 + t] : 0.0f;
    __syncthreads();
    if (t == 0) {
        const double thr = u * s_total;
        const uint32_t cnt = min(256u, n - i0);
        double cum = s_cum;
        uint32_t sel = cnt - 1;
        for (uint32_t i = 0; i < cnt; ++i) {
            cum += (double)s_vals[i];
            if (cum >= thr) {
                sel = i;
                break;
            }
        }
        *pick_out = i0 + sel;
    }
}

// centers[node][c][:] = the row of member picks[node][c]
__global__ void kt_gather_seeds_kernel(BfIndexDev ix, KtLevel lv, const uint32_t *__restrict__ picks, uint64_t total,
                                       float *__restrict__ centers) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const uint64_t yc = e / ix.dim;
    const uint32_t j = (uint32_t)(e - yc * ix.dim), y = (uint32_t)(yc / lv.C);
    centers[e] = ix.rows[(uint64_t)lv.idx[lv.tr[y].base + picks[yc]] * ix.stride + j];
}

// assign_nearest_kernel on one tile: thread t scores position first + t against its node's C centres, staged in LDS
// TC at a time.  Dynamic LDS: max(TC * dimp * 4, 2048) bytes -- the tile's partial sum reuses it.
template <int TC>
__global__ __launch_bounds__(256) void kt_assign_kernel(BfIndexDev ix, KtLevel lv, uint32_t *__restrict__ out_idx,
                                                        float *__restrict__ out_dist, double *__restrict__ partials,
                                                        uint32_t *__restrict__ min_pos) {
    extern __shared__ __attribute__((aligned(16))) float cs[];   // [TC][dimp]
    const KtTile tl = lv.tiles[blockIdx.x];
    if (lv.st[tl.node].frozen) return;   // (block-uniform)
    const uint32_t dim = ix.dim, dimp = (dim + 3u) & ~3u, k = lv.C;
    const float *centers = lv.centers + (size_t)tl.node * k * dim;
    const bool act = threadIdx.x < tl.cnt;
    const uint32_t p = tl.first + (act ? threadIdx.x : 0u);
    const float *row = ix.rows + (uint64_t)lv.idx[p] * ix.stride;
    const bool vec = ((ix.stride & 3u) == 0) && ((reinterpret_cast<uintptr_t>(ix.rows) & 15u) == 0);
    float best = __builtin_inff();
    uint32_t bi = 0;
    for (uint32_t c0 = 0; c0 < k; c0 += TC) {
        for (uint32_t e = threadIdx.x; e < TC * dimp; e += blockDim.x) {
            const uint32_t c = e / dimp, j = e - c * dimp;
            cs[e] = (c0 + c < k && j < dim) ? centers[(size_t)(c0 + c) * dim + j] : 0.0f;
        }
        __syncthreads();
        float acc[TC];
#pragma unroll
        for (int c = 0; c < TC; ++c) acc[c] = 0.0f;
        for (uint32_t j0 = 0; j0 < dim; j0 += kKtDJ) {
            float x[kKtDJ];
            if (vec && j0 + kKtDJ <= dim) {
#pragma unroll
                for (int j = 0; j < kKtDJ; j += 4) {
                    const float4 v = *reinterpret_cast<const float4 *>(row + j0 + j);
                    x[j] = v.x; x[j + 1] = v.y; x[j + 2] = v.z; x[j + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < kKtDJ; ++j) x[j] = (j0 + j < dim) ? row[j0 + j] : 0.0f;
            }
            const uint32_t nj = min((uint32_t)kKtDJ, dim - j0);
#pragma unroll
            for (int c = 0; c < TC; ++c) {
                const float *cr = cs + c * dimp + j0;
                float a = acc[c];
                if (nj == (uint32_t)kKtDJ) {
#pragma unroll
                    for (int j = 0; j < kKtDJ; ++j) {
                        const float d = x[j] - cr[j];
                        a = a + d * d;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < kKtDJ; ++j)
                        if ((uint32_t)j < nj) {
                            const float d = x[j] - cr[j];
                            a = a + d * d;
                        }
                }
                acc[c] = a;
            }
        }
#pragma unroll
        for (int c = 0; c < TC; ++c)
            if (c0 + c < k && acc[c] < best) {
                best = acc[c];
                bi = c0 + c;
            }
        __syncthreads();
    }
    if (act) {
        out_idx[p] = bi;
        out_dist[p] = best;
    }
    kt_block_sum(act ? best : 0.0f, reinterpret_cast<double *>(cs), partials + blockIdx.x, min_pos + tl.node);
}

// assign_nearest_avx_kernel on one tile (squared_l2_avx2's summation order)
__global__ __launch_bounds__(256) void kt_assign_avx_kernel(BfIndexDev ix, KtLevel lv, uint32_t *__restrict__ out_idx,
                                                            float *__restrict__ out_dist, double *__restrict__ partials,
                                                            uint32_t *__restrict__ min_pos) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) float cs[];   // [kKtAvxTC][dimp]
    const KtTile tl = lv.tiles[blockIdx.x];
    if (lv.st[tl.node].frozen) return;   // (block-uniform)
    const uint32_t dim = ix.dim, dimp = (dim + 3u) & ~3u, chunks = dim >> 3, k = lv.C;
    const float *centers = lv.centers + (size_t)tl.node * k * dim;
    const bool act = threadIdx.x < tl.cnt;
    const uint32_t p = tl.first + (act ? threadIdx.x : 0u);
    const float *row = ix.rows + (uint64_t)lv.idx[p] * ix.stride;
    const bool vec = ((ix.stride & 3u) == 0) && ((reinterpret_cast<uintptr_t>(ix.rows) & 15u) == 0);
    float best = __builtin_inff();
    uint32_t bi = 0;
    for (uint32_t c0 = 0; c0 < k; c0 += kKtAvxTC) {
        for (uint32_t e = threadIdx.x; e < kKtAvxTC * dimp; e += blockDim.x) {
            const uint32_t c = e / dimp, j = e - c * dimp;
            cs[e] = (c0 + c < k && j < dim) ? centers[(size_t)(c0 + c) * dim + j] : 0.0f;
        }
        __syncthreads();
        f32x2 acc[kKtAvxTC][4];
#pragma unroll
        for (int c = 0; c < kKtAvxTC; ++c)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[c][u] = f32x2{0.0f, 0.0f};
        for (uint32_t ch = 0; ch < chunks; ++ch) {
            float4 xa, xb;
            if (vec) {
                xa = *reinterpret_cast<const float4 *>(row + 8 * ch);
                xb = *reinterpret_cast<const float4 *>(row + 8 * ch + 4);
            } else {
                xa = make_float4(row[8 * ch], row[8 * ch + 1], row[8 * ch + 2], row[8 * ch + 3]);
                xb = make_float4(row[8 * ch + 4], row[8 * ch + 5], row[8 * ch + 6], row[8 * ch + 7]);
            }
            const f32x2 x[4] = {f32x2{xa.x, xa.y}, f32x2{xa.z, xa.w}, f32x2{xb.x, xb.y}, f32x2{xb.z, xb.w}};
#pragma unroll
            for (int c = 0; c < kKtAvxTC; ++c) {
                const float4 ca = *reinterpret_cast<const float4 *>(cs + c * dimp + 8 * ch);
                const float4 cb = *reinterpret_cast<const float4 *>(cs + c * dimp + 8 * ch + 4);
                const f32x2 cv[4] = {f32x2{ca.x, ca.y}, f32x2{ca.z, ca.w}, f32x2{cb.x, cb.y}, f32x2{cb.z, cb.w}};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const f32x2 d = x[u] - cv[u];
                    acc[c][u] = __builtin_elementwise_fma(d, d, acc[c][u]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < kKtAvxTC; ++c) {
            // chains 0..7 = acc[0].x acc[0].y acc[1].x acc[1].y acc[2].x ...: (v0+v4, v1+v5), (v2+v6, v3+v7)
            const f32x2 s01 = acc[c][0] + acc[c][2], s23 = acc[c][1] + acc[c][3];
            float r = (s01.x + s01.y) + (s23.x + s23.y);
            for (uint32_t j = chunks * 8; j < dim; ++j) {   // scalar tail, not fused
                const float d = row[j] - cs[c * dimp + j];
                r = r + d * d;
            }
            if (c0 + c < k && r < best) {
                best = r;
                bi = c0 + c;
            }
        }
        __syncthreads();
    }
    if (act) {
        out_idx[p] = bi;
        out_dist[p] = best;
    }
    kt_block_sum(act ? best : 0.0f, reinterpret_cast<double *>(cs), partials + blockIdx.x, min_pos + tl.node);
}

__global__ void kt_init_state_kernel(KtState *__restrict__ st, uint32_t *__restrict__ min_pos, uint32_t T) {
    const uint32_t y = blockIdx.x * blockDim.x + threadIdx.x;
    if (y >= T) return;
    st[y].prev = (double)INFINITY;
    st[y].inertia = 0.0;
    st[y].iters = st[y].converged = st[y].frozen = st[y].pad = 0;
    min_pos[y] = 0xFFFFFFFFu;
}

// Node blockIdx.x, unless frozen: the inertia of the assignment just made -- the primitive's tree sum over the node's
// tiles, the exactness test (km_tree_sum_is_exact), and where it fails the sum in member order
// (km_sum_f64_sequential_kernel: waves 1-3 stage the next 4096 values while lane 0 adds) -- then fit_single's
// convergence test of iteration `it` (kmeans.rs:226-246), or with `final` only the inertia (kmeans.rs:248-255).
__global__ __launch_bounds__(256) void kt_step_kernel(const KtTrain *__restrict__ tr, KtState *__restrict__ st,
                                                      const double *__restrict__ partials,
                                                      const float *__restrict__ dist, uint32_t *__restrict__ min_pos,
                                                      uint32_t it, double threshold, int final) {
    __shared__ double s_chunk[256];
    __shared__ float s_x[2][kKtSeqVals];
    __shared__ double s_total;
    __shared__ int s_need;
    const uint32_t y = blockIdx.x, tid = threadIdx.x;
    if (st[y].frozen) return;   // (block-uniform)
    const KtTrain nd = tr[y];
    const uint32_t n = nd.cnt, nb = (n + 255u) / 256u;
    partials += nd.tile0;
    const float *v = dist + nd.base;
    const uint32_t per = (nb + 255u) / 256u;
    const uint32_t b0 = min(nb, tid * per), b1 = min(nb, b0 + per);
    double mine = 0.0;
    for (uint32_t b = b0; b < b1; ++b) mine += partials[b];
    s_chunk[tid] = mine;
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        for (uint32_t q = 0; q < 256; ++q) total += s_chunk[q];
        const uint32_t mp = min_pos[y];
        bool exact = false;
        if (mp == 0xFFFFFFFFu) {
            exact = true;
        } else if (total == total && total < (double)INFINITY) {
            int e = 0;
            (void)frexpf(__uint_as_float(mp), &e);
            const int ge = max(e - 24, -149);
            exact = total <= ldexp(1.0, ge + 53);
        }
        s_total = total;
        s_need = exact ? 0 : 1;
    }
    __syncthreads();
    double total = s_total;
    if (s_need) {   // (block-uniform)
        auto stage = [&](uint32_t i0, uint32_t buf, uint32_t t0, uint32_t nt) {
            const uint32_t cnt = min(kKtSeqVals, n - i0);
            for (uint32_t f = t0; f < cnt; f += nt) s_x[buf][f] = v[i0 + f];
        };
        stage(0, 0, tid, 256);
        __syncthreads();
        double sum = 0.0;
        uint32_t buf = 0;
        for (uint32_t i0 = 0; i0 < n; i0 += kKtSeqVals, buf ^= 1u) {
            const uint32_t cnt = min(kKtSeqVals, n - i0);
            if (tid >= 64) {
                if (i0 + kKtSeqVals < n) stage(i0 + kKtSeqVals, buf ^ 1u, tid - 64, 192);
            } else if (tid == 0) {
                for (uint32_t f = 0; f < cnt; ++f) sum += (double)s_x[buf][f];
            }
            __syncthreads();
        }
        total = sum;   // (thread 0's)
    }
    if (tid != 0) return;
    min_pos[y] = 0xFFFFFFFFu;   // for the next assignment
    st[y].inertia = total;
    if (final) return;
    st[y].iters = it + 1;
    const double prev = st[y].prev;
    const double rel = fabs(prev - total) / (prev + 1e-10);
    if (rel < threshold) {
        st[y].converged = 1;
        st[y].frozen = 1;
    } else {
        st[y].prev = total;
    }
}

// position p -> (key0 of its node + its cluster where the node trains, p)
__global__ void kt_keys_kernel(const KtNode *__restrict__ nodes, uint32_t m, const uint32_t *__restrict__ assign,
                               uint64_t n, uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    uint32_t lo = 0, hi = m;   // the last node whose base is <= p
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (nodes[mid].base <= p) lo = mid; else hi = mid;
    }
    const KtNode nd = nodes[lo];
    keys[p] = nd.key0 + (nd.train ? assign[p] : 0u);
    vals[p] = (uint32_t)p;
}

// offsets[t] = first position whose key is >= t, t <= num_keys
__global__ void kt_offsets_kernel(const uint32_t *__restrict__ sorted, uint64_t n, uint32_t num_keys,
                                  uint32_t *__restrict__ offsets) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > num_keys) return;
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (sorted[mid] < t) lo = mid + 1; else hi = mid;
    }
    offsets[t] = (uint32_t)lo;
}

// out[q][:] = the row at level position order[q] (order null: q): member order, so that the update streams
__global__ void kt_gather_rows_kernel(BfIndexDev ix, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ order,
                                      uint64_t n, float *__restrict__ out) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * ix.dim) return;
    const uint64_t q = e / ix.dim;
    const uint32_t j = (uint32_t)(e - q * ix.dim);
    out[e] = ix.rows[(uint64_t)idx[order ? order[q] : (uint32_t)q] * ix.stride + j];
}

__global__ void kt_permute_kernel(const uint32_t *__restrict__ idx, const uint32_t *__restrict__ order, uint64_t n,
                                  uint32_t *__restrict__ out) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) out[q] = idx[order[q]];
}

// leaf[idx[p]] = the leaf whose slice holds position p
__global__ void kt_leaf_of_row_kernel(const uint32_t *__restrict__ idx, const uint32_t *__restrict__ leaf_off, uint32_t L,
                                      uint64_t n, uint32_t *__restrict__ leaf) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    uint32_t lo = 0, hi = L;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (leaf_off[mid] <= p) lo = mid; else hi = mid;
    }
    leaf[idx[p]] = lo;
}

// km_update_kernel's arithmetic for cluster blockIdx.x of node blockIdx.y: per dimension the f64 sum of the members in
// ascending datapoint order (positions offsets[key0 + c] .. of grows, [position][dim]), divided by the count, cast to
// f32; an empty cluster c takes the node's member c % n_node (kmeans.rs:405-408).  centers [node][C][dim].
__global__ __launch_bounds__(256) void kt_update_kernel(BfIndexDev ix, const uint32_t *__restrict__ idx,
                                                        const KtTrain *__restrict__ tr, const KtState *__restrict__ st,
                                                        const float *__restrict__ grows,
                                                        const uint32_t *__restrict__ offsets, uint32_t C,
                                                        float *__restrict__ centers) {
    __shared__ __attribute__((aligned(16))) float s_x[kKtUpdFloats];
    const uint32_t y = blockIdx.y, c = blockIdx.x, tid = threadIdx.x, dim = ix.dim;
    const bool lin = dim <= 256 && (dim & 3u) == 0 && (reinterpret_cast<uintptr_t>(grows) & 15u) == 0;
    if (st && st[y].frozen) return;   // (block-uniform)
    const KtTrain nd = tr[y];
    const uint32_t b = offsets[nd.key0 + c], e = offsets[nd.key0 + c + 1];
    float *out = centers + ((size_t)y * C + c) * dim;
    if (e == b) {
        const float *row = ix.rows + (uint64_t)idx[nd.base + c % nd.cnt] * ix.stride;
        for (uint32_t j = tid; j < dim; j += blockDim.x) out[j] = row[j];
        return;
    }
    for (uint32_t j0 = 0; j0 < dim; j0 += 256) {   // slabs of <= 256 dimensions, one chain per thread
        const uint32_t dw = min(256u, dim - j0);
        const uint32_t tm = kKtUpdFloats / dw;       // members per staged tile
        double sum = 0.0;
        for (uint32_t m0 = b; m0 < e; m0 += tm) {
            const uint32_t nm = min(tm, e - m0);
            __syncthreads();
            if (lin) {   // (kernel-uniform) one slab: the tile is nm * dim consecutive floats, at most 8 float4 per thread
                const float4 *src = reinterpret_cast<const float4 *>(grows + (uint64_t)m0 * dim);
                const uint32_t cnt4 = (nm * dim) >> 2;
                float4 v[8];
#pragma unroll
                for (uint32_t u = 0; u < 8; ++u)   // all loads in flight before the first store
                    v[u] = tid + u * 256 < cnt4 ? src[tid + u * 256] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
                for (uint32_t u = 0; u < 8; ++u)
                    if (tid + u * 256 < cnt4) reinterpret_cast<float4 *>(s_x)[tid + u * 256] = v[u];
            } else {
                for (uint32_t f = tid; f < nm * dw; f += blockDim.x) {
                    const uint32_t mm = f / dw, jj = f - mm * dw;
                    s_x[f] = grows[(uint64_t)(m0 + mm) * dim + j0 + jj];
                }
            }
            __syncthreads();
            if (tid < dw)
                for (uint32_t mm = 0; mm < nm; ++mm) sum += (double)s_x[mm * dw + tid];
        }
        if (tid < dw) out[j0 + tid] = (float)(sum / (double)(e - b));
    }
}

inline float ms_since(std::chrono::steady_clock::time_point &t) {
    const auto now = std::chrono::steady_clock::now();
    const float ms = std::chrono::duration<float, std::milli>(now - t).count();
    t = now;
    return ms;
}

int launch_kt_assign(const BfIndexDev &src, bool avx, uint32_t tiles, hipStream_t st, const KtLevel &lv, uint32_t *assign,
                     float *dist, double *partials, uint32_t *min_pos) {
    const uint32_t dimp = (src.dim + 3u) & ~3u;
    if (avx) {
        const size_t lds = std::max<size_t>((size_t)kKtAvxTC * dimp * 4, 2048);
        return launch(kt_assign_avx_kernel, dim3(tiles), dim3(256), lds, st, src, lv, assign, dist, partials, min_pos);
    }
    const int tc = (size_t)kKtTC * dimp * 4 <= kMaxLdsBytes ? kKtTC : kKtTCWide;
    return with_value<kKtTC, kKtTCWide>(tc, [&](auto t) {
        const size_t lds = std::max<size_t>((size_t)t() * dimp * 4, 2048);
        return launch(kt_assign_kernel<t()>, dim3(tiles), dim3(256), lds, st, src, lv, assign, dist, partials, min_pos);
    });
}

struct HostNode {
    uint32_t base, cnt, depth;
    bool leaf;
};

}  // namespace

int ktree_check(const scann_hip_tree_config &tree) {
    if (tree.num_children == 0)   // kmeans.rs:165-169
        return fail(SCANN_HIP_INVALID_ARGUMENT, "Number of clusters must be positive");
    if (tree.max_depth > kTreeMaxDepth)
        return fail(SCANN_HIP_UNIMPLEMENTED, "hierarchical build: max_depth > " + std::to_string(kTreeMaxDepth));
    return SCANN_HIP_OK;
}

int ktree_build_device(const BfIndexDev &src, const scann_hip_tree_config &tree, uint32_t simd_threshold, hipStream_t st,
                       BuildParts *out, DevBuf *d_leaf, scann_hip_build_report *rep, scann_hip_tree_report *trep) {
    SCANN_TRY(ktree_check(tree));
    const uint64_t n = src.n;
    const uint32_t dim = src.dim, C = tree.num_children;
    const bool avx = dim >= simd_threshold;   // kmeans.rs:419-431
    const uint32_t nb256 = (uint32_t)ceil_div_u64(n, 256);
    float seed_ms = 0.0f, lloyd_ms = 0.0f;
    if (trep) std::memset(trep, 0, sizeof(*trep));

    DevBuf d_idx, d_idx2, d_vals, d_assign, d_part, d_tiles, d_train, d_nodes, d_state, d_minpos, d_picks, d_cent, d_keys,
        d_skeys, d_pos, d_spos, d_tmp, d_off, d_grows;
    SCANN_TRY(d_idx.ensure(n * 4));
    SCANN_TRY(launch(kt_iota_kernel, dim3(nb256), dim3(256), 0, st, d_idx.as<uint32_t>(), n));
    std::vector<HostNode> nodes{HostNode{0u, (uint32_t)n, 0u, false}};
    size_t tmp_bytes = 0;
    bool level_bufs = false;
    auto t = std::chrono::steady_clock::now();

    for (uint32_t d = 0;; ++d) {
        // ---- which nodes train (build_node's leaf tests, kmeans_tree.rs:219-226), their tiles and sort keys ----
        std::vector<KtTrain> train;
        std::vector<KtTile> tiles;
        std::vector<KtNode> knodes(nodes.size());
        std::vector<uint32_t> node_train(nodes.size(), 0xFFFFFFFFu);
        uint32_t num_keys = 0;
        for (size_t i = 0; i < nodes.size(); ++i) {
            HostNode &nd = nodes[i];
            if (!nd.leaf && (d >= tree.max_depth || nd.cnt <= tree.min_leaf_size || nd.cnt <= C)) nd.leaf = true;
            knodes[i] = KtNode{nd.base, num_keys, nd.leaf ? 0u : 1u, 0u};
            if (nd.leaf) {
                num_keys += 1;
                continue;
            }
            node_train[i] = (uint32_t)train.size();
            train.push_back(KtTrain{nd.base, nd.cnt, (uint32_t)tiles.size(), num_keys});
            for (uint32_t f = 0; f < nd.cnt; f += kKtTile)
                tiles.push_back(KtTile{node_train[i], nd.base + f, std::min(kKtTile, nd.cnt - f)});
            num_keys += C;   // (a node that trains has more than C members: num_keys stays below n + the leaf count)
        }
        const uint32_t T = (uint32_t)train.size(), nt = (uint32_t)tiles.size(), m = (uint32_t)nodes.size();
        if (T == 0) break;

        if (!level_bufs) {   // every buffer whose size depends on n alone, once
            SCANN_TRY(d_idx2.ensure(n * 4));
            SCANN_TRY(d_vals.ensure(n * 4));     // min_d of the seeding, the distances of the loop: by position
            SCANN_TRY(d_assign.ensure(n * 4));
            SCANN_TRY(d_keys.ensure(n * 4));
            SCANN_TRY(d_skeys.ensure(n * 4));
            SCANN_TRY(d_pos.ensure(n * 4));
            SCANN_TRY(d_spos.ensure(n * 4));
            SCANN_TRY(d_grows.ensure(n * dim * 4));
            SCANN_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, d_keys.as<uint32_t>(),
                                                               d_skeys.as<uint32_t>(), d_pos.as<uint32_t>(),
                                                               d_spos.as<uint32_t>(), (int)n, 0, 32, st));
            SCANN_TRY(d_tmp.ensure(tmp_bytes));
            level_bufs = true;
        }
        SCANN_TRY(upload(d_train, train.data(), train.size() * sizeof(KtTrain)));
        SCANN_TRY(upload(d_tiles, tiles.data(), tiles.size() * sizeof(KtTile)));
        SCANN_TRY(upload(d_nodes, knodes.data(), knodes.size() * sizeof(KtNode)));
        SCANN_TRY(d_part.ensure((size_t)nt * 8));
        SCANN_TRY(d_state.ensure((size_t)T * sizeof(KtState)));
        SCANN_TRY(d_minpos.ensure((size_t)T * 4));
        SCANN_TRY(d_picks.ensure((size_t)T * C * 4));
        SCANN_TRY(d_cent.ensure((size_t)T * C * dim * 4));
        SCANN_TRY(d_off.ensure(((size_t)num_keys + 1) * 4));
        SCANN_TRY(launch(kt_init_state_kernel, dim3(ceil_div_u32(T, 256)), dim3(256), 0, st, d_state.as<KtState>(),
                         d_minpos.as<uint32_t>(), T));
        KtLevel lv;
        lv.idx = d_idx.as<uint32_t>();
        lv.tiles = d_tiles.as<KtTile>();
        lv.tr = d_train.as<KtTrain>();
        lv.st = d_state.as<KtState>();
        lv.centers = d_cent.as<float>();
        lv.C = C;

        // ---- seeding: kmeans_plusplus_init of every node with the stream of seed + d, round by round ----
        {
            uint64_t z = tree.seed + d;   // kmeans_tree.rs:235
            const uint64_t z0 = km_seed_stream_next(z);
            SCANN_TRY(launch(kt_first_pick_kernel, dim3(ceil_div_u32(T, 256)), dim3(256), 0, st, lv.tr, T, z0, C,
                             d_picks.as<uint32_t>()));
            for (uint32_t c = 1; c < C; ++c) {
                SCANN_TRY(launch(kt_mind_kernel, dim3(nt), dim3(256), 0, st, src, lv, (const uint32_t *)d_picks.as<uint32_t>(),
                                 c, c == 1 ? 1 : 0, avx ? 1 : 0, d_vals.as<float>(), d_part.as<double>()));
                const double u = (double)(km_seed_stream_next(z) >> 11) * (1.0 / 9007199254740992.0);
                const uint64_t zfb = km_seed_stream_next(z);
                SCANN_TRY(launch(kt_pick_kernel, dim3(T), dim3(256), 0, st, lv.tr, (const double *)d_part.as<double>(),
                                 (const float *)d_vals.as<float>(), u, zfb, C, c, d_picks.as<uint32_t>()));
            }
            const uint64_t total = (uint64_t)T * C * dim;
            SCANN_TRY(launch(kt_gather_seeds_kernel, dim3((uint32_t)ceil_div_u64(total, 256)), dim3(256), 0, st, src, lv,
                             (const uint32_t *)d_picks.as<uint32_t>(), total, d_cent.as<float>()));
            SCANN_HIP_CHECK(hipStreamSynchronize(st));
        }
        const float level_seed_ms = ms_since(t);
        seed_ms += level_seed_ms;

        // ---- Lloyd loop, every node with its own prev / inertia / iteration count / converged flag ----
        std::vector<KtState> hs(T);
        int end_bit = 1;
        while (end_bit < 32 && (1ull << end_bit) < num_keys) ++end_bit;
        auto sort_by_cluster = [&]() -> int {
            SCANN_TRY(launch(kt_keys_kernel, dim3(nb256), dim3(256), 0, st, (const KtNode *)d_nodes.as<KtNode>(), m,
                             (const uint32_t *)d_assign.as<uint32_t>(), n, d_keys.as<uint32_t>(), d_pos.as<uint32_t>()));
            SCANN_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(d_tmp.p, tmp_bytes, d_keys.as<uint32_t>(),
                                                               d_skeys.as<uint32_t>(), d_pos.as<uint32_t>(),
                                                               d_spos.as<uint32_t>(), (int)n, 0, end_bit, st));
            return launch(kt_offsets_kernel, dim3(ceil_div_u32(num_keys + 1, 256)), dim3(256), 0, st,
                          (const uint32_t *)d_skeys.as<uint32_t>(), n, num_keys, d_off.as<uint32_t>());
        };
        auto assign_and_step = [&](uint32_t it, int final) -> int {
            SCANN_TRY(launch_kt_assign(src, avx, nt, st, lv, d_assign.as<uint32_t>(), d_vals.as<float>(),
                                       d_part.as<double>(), d_minpos.as<uint32_t>()));
            return launch(kt_step_kernel, dim3(T), dim3(256), 0, st, lv.tr, d_state.as<KtState>(),
                          (const double *)d_part.as<double>(), (const float *)d_vals.as<float>(), d_minpos.as<uint32_t>(),
                          it, tree.kmeans_convergence, final);
        };
        for (uint32_t it = 0; it < tree.kmeans_iterations; ++it) {
            SCANN_TRY(assign_and_step(it, 0));
            SCANN_HIP_CHECK(hipMemcpyAsync(hs.data(), d_state.p, (size_t)T * sizeof(KtState), hipMemcpyDeviceToHost, st));
            SCANN_HIP_CHECK(hipStreamSynchronize(st));
            bool active = false;
            for (const auto &h : hs) active = active || !h.frozen;
            if (!active) break;
            // update_centers of the active nodes: members of every (node, cluster) in ascending datapoint order
            SCANN_TRY(sort_by_cluster());
            SCANN_TRY(launch(kt_gather_rows_kernel, dim3((uint32_t)ceil_div_u64(n * dim, 256)), dim3(256), 0, st, src, lv.idx,
                             (const uint32_t *)d_spos.as<uint32_t>(), n, d_grows.as<float>()));
            SCANN_TRY(launch(kt_update_kernel, dim3(C, T), dim3(256), 0, st, src, lv.idx, lv.tr, lv.st,
                             (const float *)d_grows.as<float>(), (const uint32_t *)d_off.as<uint32_t>(), C,
                             d_cent.as<float>()));
        }
        // the assignment of the final centres (kmeans.rs:248-255); a converged node already holds it
        SCANN_TRY(assign_and_step(0, 1));
        SCANN_HIP_CHECK(hipMemcpyAsync(hs.data(), d_state.p, (size_t)T * sizeof(KtState), hipMemcpyDeviceToHost, st));

        // ---- children: the non-empty clusters in order; the sorted positions are the next level's order ----
        SCANN_TRY(sort_by_cluster());
        std::vector<uint32_t> off((size_t)num_keys + 1);
        SCANN_HIP_CHECK(hipMemcpyAsync(off.data(), d_off.p, off.size() * 4, hipMemcpyDeviceToHost, st));
        SCANN_TRY(launch(kt_permute_kernel, dim3(nb256), dim3(256), 0, st, lv.idx, (const uint32_t *)d_spos.as<uint32_t>(), n,
                         d_idx2.as<uint32_t>()));
        SCANN_HIP_CHECK(hipStreamSynchronize(st));
        std::swap(d_idx.p, d_idx2.p);
        std::swap(d_idx.bytes, d_idx2.bytes);
        std::vector<HostNode> next;
        next.reserve(nodes.size());
        for (size_t i = 0; i < nodes.size(); ++i) {
            const HostNode &nd = nodes[i];
            const uint32_t k0 = knodes[i].key0;
            if (nd.leaf) {
                next.push_back(HostNode{off[k0], nd.cnt, nd.depth, true});
                continue;
            }
            uint32_t nonempty = 0;
            for (uint32_t c = 0; c < C; ++c) nonempty += off[k0 + c + 1] > off[k0 + c] ? 1u : 0u;
            if (nonempty <= 1) {   // kmeans_tree.rs:252-256: nothing was split off
                next.push_back(HostNode{off[k0], nd.cnt, nd.depth, true});
                continue;
            }
            for (uint32_t c = 0; c < C; ++c)
                if (off[k0 + c + 1] > off[k0 + c])
                    next.push_back(HostNode{off[k0 + c], off[k0 + c + 1] - off[k0 + c], d + 1, false});
        }
        if (rep && d == 0) {   // (level 0 holds the root alone)
            rep->partition_iterations = hs[0].iters;
            rep->partition_converged = (int32_t)hs[0].converged;
            rep->partition_inertia = hs[0].inertia;
        }
        const float level_lloyd_ms = ms_since(t);
        lloyd_ms += level_lloyd_ms;
        if (trep) {
            trep->level_nodes[d] = T;
            for (const auto &h : hs) {
                trep->level_iterations[d] += h.iters;
                trep->level_converged[d] += h.converged;
            }
            trep->stage_ms[2 * d] = level_seed_ms;
            trep->stage_ms[2 * d + 1] = level_lloyd_ms;
        }
        nodes.swap(next);
        // every node ends as at least one leaf
        if (nodes.size() > kMaxLeavesSelect)
            return fail(SCANN_HIP_UNIMPLEMENTED, "hierarchical build: " + std::to_string(nodes.size()) + " nodes at depth " +
                                                     std::to_string(d + 1) + ", more than " +
                                                     std::to_string(kMaxLeavesSelect) + " leaves");
    }

    // ---- the leaves: the last level's nodes in order; compute_center of each (kmeans_tree.rs:270-284) ----
    const uint32_t L = (uint32_t)nodes.size();
    out->L = L;
    out->off.assign((size_t)L + 1, 0u);
    std::vector<KtTrain> leaves(L);
    uint32_t depth_reached = 0;
    for (uint32_t l = 0; l < L; ++l) {
        out->off[l] = nodes[l].base;
        leaves[l] = KtTrain{nodes[l].base, nodes[l].cnt, 0u, l};
        depth_reached = std::max(depth_reached, nodes[l].depth);
        if (trep) trep->level_leaves[nodes[l].depth] += 1;
    }
    out->off[L] = (uint32_t)n;
    if (trep) {
        trep->num_leaves = L;
        trep->depth_reached = depth_reached;
    }
    SCANN_TRY(upload(out->leaf_off, out->off.data(), out->off.size() * 4));
    SCANN_TRY(upload(d_train, leaves.data(), leaves.size() * sizeof(KtTrain)));
    SCANN_TRY(out->centers.ensure((size_t)L * dim * 4));
    SCANN_TRY(d_leaf->ensure(n * 4));
    SCANN_TRY(d_grows.ensure(n * dim * 4));
    SCANN_TRY(launch(kt_gather_rows_kernel, dim3((uint32_t)ceil_div_u64(n * dim, 256)), dim3(256), 0, st, src,
                     (const uint32_t *)d_idx.as<uint32_t>(), (const uint32_t *)nullptr, n, d_grows.as<float>()));
    SCANN_TRY(launch(kt_update_kernel, dim3(1, L), dim3(256), 0, st, src, (const uint32_t *)d_idx.as<uint32_t>(),
                     (const KtTrain *)d_train.as<KtTrain>(), (const KtState *)nullptr, (const float *)d_grows.as<float>(),
                     (const uint32_t *)out->leaf_off.as<uint32_t>(), 1u, out->centers.as<float>()));
    SCANN_TRY(launch(kt_leaf_of_row_kernel, dim3(nb256), dim3(256), 0, st, (const uint32_t *)d_idx.as<uint32_t>(),
                     (const uint32_t *)out->leaf_off.as<uint32_t>(), L, n, d_leaf->as<uint32_t>()));
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    out->leaf_ids.take(d_idx);
    lloyd_ms += ms_since(t);
    if (rep) {
        rep->stage_ms[0] = seed_ms;
        rep->stage_ms[1] = lloyd_ms;
    }
    return SCANN_HIP_OK;
}

}  // namespace scann

// build.hip -- scann_hip_txh_build (scann_hip.h "device build"): partitioner, residual training rows, codebook, codes
// and CSR layout of a tree / flat-hasher index, from rows that are already on the device.  The k-means cores
// (seeding, Lloyd loop, the f64 reductions and the ordered centre update) are bf.hip's; this unit adds
//
//   build_residual_kernel    training rows x - centres[token(x)], same stride, pad columns zero
//   cb_mind_all_kernel       one k-means++ round of EVERY subspace: min_d[s][i] against subspace s's last pick
//   cb_assign_all_kernel     one Lloyd assignment of EVERY subspace: code[s][i], dist[s][i]
//   cb_* (small)             keys / offsets / gather of the batched centre update, the per-subspace stop, seeds
//   build_ids_kernel, build_pack_codes_kernel    the CSR ids and the code words through the CSR permutation
//
// The two cb_*_all kernels read each training row once per pass: a workgroup stages a tile of 64 rows (the columns of a
// GROUP of subspaces) in LDS with coalesced float4 loads, next to the group's codebook, and lane r of wave w scores row
// r against subspace w, w + 4, ... of the group -- the codebook reads are LDS broadcasts, the row reads conflict-free
// (odd tile pitch).  Every (row, subspace) gets assign_nearest_kernel's arithmetic: sequential scalar sum of
// (x - c)^2 in f32 (this unit is compiled with -ffp-contract=off like the rest), strict '<', lowest index, so a NaN
// distance never wins and an all-NaN row takes code 0 at +inf.
//
// Batched centre update: ONE stable radix sort (hipcub SortPairs) of the n S pairs (s K + code -> row) over the
// ceil(log2(S K)) key bits.  The pairs are generated subspace by subspace in ascending row order, so stability alone
// gives every (subspace, code) its members in ascending row order -- 2 radix passes over 32-bit keys where the
// per-subspace loop sorts S times n 64-bit keys over 33+ bits.  A counting sort on the 8-bit codes would need a
// stable intra-block rank per (subspace, code); the library sort already is that.
#include "build.h"

#include <hipcub/hipcub.hpp>

#include <chrono>
#include <cmath>
#include <cstring>

#include "ktree.h"
#include "launch.h"
#include "txh.h"

namespace scann {

namespace {

constexpr uint32_t kCbRows = 64;         // rows per tile: one per lane
constexpr uint32_t kCbTileCols = 128;    // a group's columns, unless one subspace alone is wider
constexpr uint32_t kCbStateWords = 8;    // CbState in u32 words

// per-subspace record of the batched Lloyd loop (device resident; the host reads the block once per iteration)
struct CbState {
    double prev, inertia;
    uint32_t iters, converged, frozen, need_seq;
};
static_assert(sizeof(CbState) == kCbStateWords * 4, "CbState is addressed in words");
struct CbTotal {   // km_sum_f64_kernel / km_total_pick_kernel's outputs of one subspace
    double total;
    uint32_t min_pos, pad;
};

struct CbArgs {
    const float *train;   // [n][stride]
    uint64_t n;
    uint32_t stride, dsub, S, K, k, G;   // K: codebook pitch in centres, k = min(K, n) trained ones, G: subspaces per group
    uint32_t vec;                        // float4 tile loads (stride % 4 == 0, 16-byte aligned rows, dsub G % 4 == 0)
};

__global__ __launch_bounds__(256) void build_residual_kernel(const float *__restrict__ rows, uint64_t n, uint32_t dim,
                                                             uint32_t stride, const float *__restrict__ centers,
                                                             const uint32_t *__restrict__ token, float *__restrict__ out,
                                                             int vec) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (vec) {   // (kernel-uniform) one float4 per thread
        const uint32_t q = stride >> 2;
        if (t >= n * q) return;
        const uint64_t i = t / q;
        const uint32_t j = (uint32_t)(t - i * q) * 4;
        const float4 x = *reinterpret_cast<const float4 *>(rows + i * stride + j);
        const float *c = centers + (size_t)token[i] * dim;
        float4 r;
        r.x = j + 0 < dim ? x.x - c[j + 0] : 0.0f;
        r.y = j + 1 < dim ? x.y - c[j + 1] : 0.0f;
        r.z = j + 2 < dim ? x.z - c[j + 2] : 0.0f;
        r.w = j + 3 < dim ? x.w - c[j + 3] : 0.0f;
        *reinterpret_cast<float4 *>(out + i * stride + j) = r;
    } else {
        if (t >= n * stride) return;
        const uint64_t i = t / stride;
        const uint32_t j = (uint32_t)(t - i * stride);
        out[t] = j < dim ? rows[t] - centers[(size_t)token[i] * dim + j] : 0.0f;
    }
}

// rows i0 .. i0 + 63, columns col0 .. col0 + width - 1 -> tile[r * pitch + column]; rows past n are zero
__device__ __forceinline__ void cb_stage_tile(const CbArgs &a, uint64_t i0, uint32_t col0, uint32_t width, uint32_t pitch,
                                              float *__restrict__ tile) {
    if (a.vec) {
        const uint32_t w4 = width >> 2;
        for (uint32_t q = threadIdx.x; q < kCbRows * w4; q += 256) {
            const uint32_t r = q / w4, j = (q - r * w4) * 4;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (i0 + r < a.n) v = *reinterpret_cast<const float4 *>(a.train + (i0 + r) * a.stride + col0 + j);
            float *d = tile + r * pitch + j;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
    } else {
        for (uint32_t q = threadIdx.x; q < kCbRows * width; q += 256) {
            const uint32_t r = q / width, j = q - r * width;
            tile[r * pitch + j] = i0 + r < a.n ? a.train[(i0 + r) * a.stride + col0 + j] : 0.0f;
        }
    }
}

// DS: dims per subspace known at compile time (the row's values stay in registers); 0: read from the tile
template <int DS>
__global__ __launch_bounds__(256) void cb_assign_all_kernel(CbArgs a, const float *__restrict__ codebook,
                                                            const uint32_t *__restrict__ state_words,
                                                            uint8_t *__restrict__ code, float *__restrict__ dist) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t dsub = DS ? (uint32_t)DS : a.dsub;
    const uint32_t s0 = blockIdx.y * a.G, gs = min(a.G, a.S - s0), width = gs * dsub, pitch = (a.G * dsub) | 1u;
    float *cbs = lds;                                   // [G][k][dsub]
    float *tile = lds + (size_t)a.G * a.k * dsub;       // [64][pitch]
    bool any = false;
    for (uint32_t ls = 0; ls < gs; ++ls) any = any || !state_words[(s0 + ls) * kCbStateWords + 6];
    if (!any) return;   // (block-uniform) every subspace of the group is frozen
    for (uint32_t e = threadIdx.x; e < gs * a.k * dsub; e += 256) {
        const uint32_t ls = e / (a.k * dsub), f = e - ls * (a.k * dsub);
        cbs[e] = codebook[(size_t)(s0 + ls) * a.K * dsub + f];
    }
    const uint32_t r = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t tiles = (a.n + kCbRows - 1) / kCbRows;
    for (uint64_t tI = blockIdx.x; tI < tiles; tI += gridDim.x) {
        const uint64_t i0 = tI * kCbRows;
        __syncthreads();   // the previous tile is read, the codebook is staged
        cb_stage_tile(a, i0, s0 * dsub, width, pitch, tile);
        __syncthreads();
        for (uint32_t ls = w; ls < gs; ls += 4) {   // (wave-uniform)
            const uint32_t s = s0 + ls;
            if (state_words[s * kCbStateWords + 6]) continue;
            const float *x = tile + r * pitch + ls * dsub;
            const float *cb = cbs + (size_t)ls * a.k * dsub;
            float best = __builtin_inff();
            uint32_t bi = 0;
            if constexpr (DS > 0) {
                float xr[DS > 0 ? DS : 1];
#pragma unroll
                for (int j = 0; j < DS; ++j) xr[j] = x[j];
                for (uint32_t c = 0; c < a.k; ++c) {
                    float d = 0.0f;
#pragma unroll
                    for (int j = 0; j < DS; ++j) {
                        const float t = xr[j] - cb[c * DS + j];
                        d = d + t * t;
                    }
                    if (d < best) {
                        best = d;
                        bi = c;
                    }
                }
            } else {
                for (uint32_t c = 0; c < a.k; ++c) {
                    float d = 0.0f;
                    for (uint32_t j = 0; j < dsub; ++j) {
                        const float t = x[j] - cb[c * dsub + j];
                        d = d + t * t;
                    }
                    if (d < best) {
                        best = d;
                        bi = c;
                    }
                }
            }
            if (i0 + r < a.n) {
                code[(uint64_t)s * a.n + i0 + r] = (uint8_t)bi;
                dist[(uint64_t)s * a.n + i0 + r] = best;
            }
        }
    }
}

// min_d[s][i] = min(min_d[s][i], ||x_i - x_pick(s)||^2) over subspace s's columns (km_mind_update_kernel's rule, the
// sequential order); first: overwrite.  picks [S][k]: round c reads column c - 1.
__global__ __launch_bounds__(256) void cb_mind_all_kernel(CbArgs a, const uint32_t *__restrict__ picks, uint32_t c,
                                                          int first, float *__restrict__ min_d) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t dsub = a.dsub;
    const uint32_t s0 = blockIdx.y * a.G, gs = min(a.G, a.S - s0), width = gs * dsub, pitch = (a.G * dsub) | 1u;
    float *sel = lds;                          // [G][dsub]: the picked rows' columns
    float *tile = lds + (size_t)a.G * dsub;    // [64][pitch]
    for (uint32_t e = threadIdx.x; e < width; e += 256) {
        const uint32_t ls = e / dsub;
        sel[e] = a.train[(uint64_t)picks[(size_t)(s0 + ls) * a.k + c - 1] * a.stride + s0 * dsub + e];
    }
    const uint32_t r = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t tiles = (a.n + kCbRows - 1) / kCbRows;
    for (uint64_t tI = blockIdx.x; tI < tiles; tI += gridDim.x) {
        const uint64_t i0 = tI * kCbRows;
        __syncthreads();
        cb_stage_tile(a, i0, s0 * dsub, width, pitch, tile);
        __syncthreads();
        if (i0 + r >= a.n) continue;   // (no barrier below in this iteration)
        for (uint32_t ls = w; ls < gs; ls += 4) {
            const float *x = tile + r * pitch + ls * dsub, *y = sel + ls * dsub;
            float d = 0.0f;
            for (uint32_t j = 0; j < dsub; ++j) {
                const float t = x[j] - y[j];
                d = d + t * t;
            }
            float *m = min_d + (uint64_t)(s0 + ls) * a.n + i0 + r;
            *m = (first || d < *m) ? d : *m;
        }
    }
}

// codebook[s][c][:] = the row picks[s][c]'s columns of subspace s, c < k
__global__ void cb_gather_seeds_kernel(CbArgs a, const uint32_t *__restrict__ picks, float *__restrict__ codebook) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.S * a.k * a.dsub) return;
    const uint32_t s = e / (a.k * a.dsub), f = e - s * (a.k * a.dsub), c = f / a.dsub, j = f - c * a.dsub;
    codebook[((size_t)s * a.K + c) * a.dsub + j] = a.train[(uint64_t)picks[(size_t)s * a.k + c] * a.stride + s * a.dsub + j];
}

// Codebook::train's padding: codes k .. K - 1 repeat centre k - 1
__global__ void cb_pad_kernel(float *__restrict__ codebook, uint32_t S, uint32_t K, uint32_t k, uint32_t dsub) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= S * (K - k) * dsub) return;
    const uint32_t s = e / ((K - k) * dsub), f = e - s * ((K - k) * dsub), c = k + f / dsub, j = f % dsub;
    codebook[((size_t)s * K + c) * dsub + j] = codebook[((size_t)s * K + k - 1) * dsub + j];
}

// one subspace's trained centres [k][dsub] -> codebook[s], padded
__global__ void cb_store_subspace_kernel(const float *__restrict__ centers, float *__restrict__ codebook_s, uint32_t K,
                                         uint32_t k, uint32_t dsub) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= K * dsub) return;
    const uint32_t c = e / dsub, j = e - c * dsub;
    codebook_s[e] = centers[(size_t)min(c, k - 1) * dsub + j];
}

// the exactness test of the tree sums (km_tree_sum_is_exact, per subspace): need_seq = the chain has to be run
__global__ void cb_exact_kernel(const CbTotal *__restrict__ tot, CbState *__restrict__ st, uint32_t S) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S || st[s].frozen) return;
    const double total = tot[s].total;
    const uint32_t mp = tot[s].min_pos;
    bool exact = false;
    if (mp == 0xFFFFFFFFu) {
        exact = true;
    } else if (total == total && total < (double)INFINITY) {
        int e = 0;
        (void)frexpf(__uint_as_float(mp), &e);
        const int ge = max(e - 24, -149);
        exact = total <= ldexp(1.0, ge + 53);
    }
    st[s].need_seq = exact ? 0u : 1u;
}

// fit_single's convergence test (kmeans.rs:226-246) of iteration `it`, per subspace that is still active
__global__ void cb_step_kernel(const CbTotal *__restrict__ tot, CbState *__restrict__ st, uint32_t S, uint32_t it,
                               double threshold) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S || st[s].frozen) return;
    const double inertia = tot[s].total, prev = st[s].prev;
    st[s].iters = it + 1;
    st[s].inertia = inertia;
    st[s].need_seq = 0;
    const double rel = fabs(prev - inertia) / (prev + 1e-10);
    if (rel < threshold) {
        st[s].converged = 1;
        st[s].frozen = 1;
    } else {
        st[s].prev = inertia;
    }
}

__global__ void cb_init_state_kernel(CbState *__restrict__ st, CbTotal *__restrict__ tot, uint32_t S) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    st[s].prev = (double)INFINITY;
    st[s].inertia = 0.0;
    st[s].iters = st[s].converged = st[s].frozen = st[s].need_seq = 0;
    tot[s].total = 0.0;
    tot[s].min_pos = 0xFFFFFFFFu;
    tot[s].pad = 0;
}

__global__ void cb_reset_min_pos_kernel(CbTotal *__restrict__ tot, uint32_t S) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < S) tot[s].min_pos = 0xFFFFFFFFu;
}

// pair p = s n + i: key s K + code[s][i], value i
__global__ void cb_make_pairs_kernel(const uint8_t *__restrict__ code, uint64_t n, uint32_t S, uint32_t K,
                                     uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n * S) return;
    const uint32_t s = (uint32_t)(p / n);
    keys[p] = s * K + code[p];
    vals[p] = (uint32_t)(p - (uint64_t)s * n);
}

// offsets[t] = first position whose key is >= t, t <= S K
__global__ void cb_offsets_kernel(const uint32_t *__restrict__ sorted, uint64_t total, uint32_t SK,
                                  uint32_t *__restrict__ offsets) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > SK) return;
    uint64_t lo = 0, hi = total;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (sorted[mid] < t) lo = mid + 1; else hi = mid;
    }
    offsets[t] = (uint32_t)lo;
}

// position p (subspace p / n) -> its member's columns, contiguous: the update streams them (km_gather_sorted_kernel)
__global__ void cb_gather_kernel(CbArgs a, const uint32_t *__restrict__ vals, const uint32_t *__restrict__ state_words,
                                 float *__restrict__ out) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.n * a.S * a.dsub) return;
    const uint64_t p = e / a.dsub;
    const uint32_t j = (uint32_t)(e - p * a.dsub), s = (uint32_t)(p / a.n);
    if (state_words[s * kCbStateWords + 6]) return;
    out[e] = a.train[(uint64_t)vals[p] * a.stride + s * a.dsub + j];
}

__global__ void build_ids_kernel(const uint64_t *__restrict__ sorted, uint64_t n, uint32_t *__restrict__ ids) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) ids[p] = (uint32_t)sorted[p];
}

// code words of CSR row p = the byte codes of datapoint ids[p] (ids null: p), nibble / byte s of word s / per
__global__ void build_pack_codes_kernel(const uint8_t *__restrict__ code8, const uint32_t *__restrict__ ids, uint64_t n,
                                        uint32_t S, uint32_t nw, uint32_t bits, uint32_t *__restrict__ words) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * nw) return;
    const uint64_t p = e / nw;
    const uint32_t w = (uint32_t)(e - p * nw), per = bits == 4 ? 8u : 4u;
    const uint8_t *c = code8 + (uint64_t)(ids ? ids[p] : (uint32_t)p) * S + w * per;
    uint32_t word = 0;
    for (uint32_t s = 0; s < per; ++s) word |= bits == 4 ? ((uint32_t)c[s] & 15u) << (4 * s) : (uint32_t)c[s] << (8 * s);
    words[e] = word;
}

inline float ms_since(std::chrono::steady_clock::time_point &t) {
    const auto now = std::chrono::steady_clock::now();
    const float ms = std::chrono::duration<float, std::milli>(now - t).count();
    t = now;
    return ms;
}

// subspaces per group: as many as fit in the CU's LDS beside the tile, a tile of at most kCbTileCols columns
uint32_t cb_group_size(uint32_t S, uint32_t k, uint32_t dsub) {
    uint32_t G = 0;
    for (uint32_t g = 1; g <= S; ++g) {
        const size_t bytes = ((size_t)g * k * dsub + (size_t)kCbRows * ((g * dsub) | 1u)) * 4;
        if (bytes > kMaxLdsBytes || (g > 1 && g * dsub > kCbTileCols)) break;
        G = g;
    }
    return G;
}

template <typename... Args>
int launch_assign_all(uint32_t dsub, dim3 grid, size_t lds, hipStream_t st, Args &&...args) {
    const int ds = (dsub == 1 || dsub == 2 || dsub == 4 || dsub == 8 || dsub == 16) ? (int)dsub : 0;
    return with_value<1, 2, 4, 8, 16, 0>(ds, [&](auto t) {
        return launch(cb_assign_all_kernel<t()>, grid, dim3(256), lds, st, args...);
    });
}

// Codebook::train with all subspaces in lockstep; codebook [S][K][dsub] on the device, complete on return
int train_codebook_batched(const BfIndexDev &tv, const scann_hip_build_config &cfg, uint32_t dsub, uint32_t k, uint32_t G,
                           float *d_codebook, hipStream_t st, scann_hip_build_report *rep, float *seed_ms,
                           float *lloyd_ms) {
    const uint32_t S = cfg.num_subspaces, K = cfg.num_codes;
    const uint64_t n = tv.n, total = n * S;
    const uint32_t nb = (uint32_t)ceil_div_u64(n, 256), groups = ceil_div_u32(S, G);
    CbArgs a;
    a.train = tv.rows; a.n = n; a.stride = tv.stride; a.dsub = dsub; a.S = S; a.K = K; a.k = k; a.G = G;
    const uint32_t last_cols = (S - (groups - 1) * G) * dsub;   // every group starts at a multiple of G dsub columns
    a.vec = ((tv.stride & 3u) == 0 && (reinterpret_cast<uintptr_t>(tv.rows) & 15u) == 0 && ((G * dsub) & 3u) == 0 &&
             (last_cols & 3u) == 0) ? 1u : 0u;
    const uint64_t tiles = ceil_div_u64(n, kCbRows);
    const uint32_t gx = (uint32_t)std::min<uint64_t>(tiles, std::max<uint32_t>(1u, 4u * (uint32_t)num_cus() / groups));
    auto t = std::chrono::steady_clock::now();

    // every buffer of the loop, once
    DevBuf d_vals, d_code, d_part, d_tot, d_state, d_picks, d_utab, d_fbtab, d_keys, d_skeys, d_rows, d_srows, d_tmp, d_off,
        d_grows;
    SCANN_TRY(d_vals.ensure(total * 4));                 // min_d of the seeding, dist of the loop: [S][n]
    SCANN_TRY(d_code.ensure(total));
    SCANN_TRY(d_part.ensure((size_t)S * nb * 8));
    SCANN_TRY(d_tot.ensure((size_t)S * sizeof(CbTotal)));
    SCANN_TRY(d_state.ensure((size_t)S * sizeof(CbState)));
    SCANN_TRY(d_picks.ensure((size_t)S * k * 4));
    SCANN_TRY(launch(cb_init_state_kernel, dim3(1), dim3(64), 0, st, d_state.as<CbState>(), d_tot.as<CbTotal>(), S));
    const uint32_t *state_words = d_state.as<uint32_t>();

    // ---- seeding: the S random streams of kmeans_plusplus_init, round by round ----
    {
        std::vector<uint32_t> first(S), fb((size_t)k * S, 0u);
        std::vector<double> us((size_t)k * S, 0.0);
        for (uint32_t s = 0; s < S; ++s) {
            uint64_t z = cfg.seed + s;
            first[s] = (uint32_t)(km_seed_stream_next(z) % n);
            for (uint32_t c = 1; c < k; ++c) {
                us[(size_t)c * S + s] = (double)(km_seed_stream_next(z) >> 11) * (1.0 / 9007199254740992.0);
                fb[(size_t)c * S + s] = (uint32_t)(km_seed_stream_next(z) % n);
            }
        }
        SCANN_TRY(upload(d_utab, us.data(), us.size() * 8));
        SCANN_TRY(upload(d_fbtab, fb.data(), fb.size() * 4));
        SCANN_HIP_CHECK(hipMemcpy2D(d_picks.p, (size_t)k * 4, first.data(), 4, 4, S, hipMemcpyHostToDevice));
        const size_t lds = ((size_t)G * dsub + (size_t)kCbRows * ((G * dsub) | 1u)) * 4;
        for (uint32_t c = 1; c <= k; ++c) {
            SCANN_TRY(launch(cb_mind_all_kernel, dim3(gx, groups), dim3(256), lds, st, a, d_picks.as<uint32_t>(), c,
                             c == 1 ? 1 : 0, d_vals.as<float>()));
            if (c == k) break;
            SCANN_TRY(km_sums_batched(d_vals.as<float>(), n, S, d_part.as<double>(), nullptr, 0, nullptr, 0, st));
            SCANN_TRY(km_totals_batched(d_part.as<double>(), n, S, d_vals.as<float>(), d_utab.as<double>() + (size_t)c * S,
                                        d_fbtab.as<uint32_t>() + (size_t)c * S, &d_tot.as<CbTotal>()->total, 2,
                                        d_picks.as<uint32_t>() + c, k, st));
        }
        SCANN_TRY(launch(cb_gather_seeds_kernel, dim3(ceil_div_u32(S * k * dsub, 256)), dim3(256), 0, st, a,
                         d_picks.as<uint32_t>(), d_codebook));
        SCANN_HIP_CHECK(hipStreamSynchronize(st));
    }
    *seed_ms += ms_since(t);

    // ---- Lloyd loop, every subspace with its own prev / inertia / iteration count / converged flag ----
    std::vector<CbState> hs(S);
    for (auto &h : hs) std::memset(&h, 0, sizeof(h));
    if (cfg.training_iterations) {
        const int end_bit = std::max(1, (int)std::ceil(std::log2((double)S * K)));
        SCANN_TRY(d_keys.ensure(total * 4));
        SCANN_TRY(d_skeys.ensure(total * 4));
        SCANN_TRY(d_rows.ensure(total * 4));
        SCANN_TRY(d_srows.ensure(total * 4));
        SCANN_TRY(d_off.ensure(((size_t)S * K + 1) * 4));
        SCANN_TRY(d_grows.ensure(total * dsub * 4));
        size_t tmp_bytes = 0;
        SCANN_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, d_keys.as<uint32_t>(), d_skeys.as<uint32_t>(),
                                                           d_rows.as<uint32_t>(), d_srows.as<uint32_t>(), (int)total, 0,
                                                           end_bit, st));
        SCANN_TRY(d_tmp.ensure(tmp_bytes));
        const size_t lds = ((size_t)G * k * dsub + (size_t)kCbRows * ((G * dsub) | 1u)) * 4;
        BfIndexDev w0 = tv;   // subspace 0's column window
        w0.dim = dsub;
        for (uint32_t it = 0; it < cfg.training_iterations; ++it) {
            SCANN_TRY(launch_assign_all(dsub, dim3(gx, groups), lds, st, a, (const float *)d_codebook, state_words,
                                        d_code.as<uint8_t>(), d_vals.as<float>()));
            SCANN_TRY(launch(cb_reset_min_pos_kernel, dim3(1), dim3(64), 0, st, d_tot.as<CbTotal>(), S));
            SCANN_TRY(km_sums_batched(d_vals.as<float>(), n, S, d_part.as<double>(), &d_tot.as<CbTotal>()->min_pos, 4,
                                      state_words + 6, kCbStateWords, st));
            SCANN_TRY(km_totals_batched(d_part.as<double>(), n, S, nullptr, nullptr, nullptr, &d_tot.as<CbTotal>()->total,
                                        2, nullptr, 0, st));
            SCANN_TRY(launch(cb_exact_kernel, dim3(1), dim3(64), 0, st, d_tot.as<CbTotal>(), d_state.as<CbState>(), S));
            SCANN_TRY(km_sequential_sums_batched(d_vals.as<float>(), n, S, &d_tot.as<CbTotal>()->total, 2, state_words + 7,
                                                 kCbStateWords, st));
            SCANN_TRY(launch(cb_step_kernel, dim3(1), dim3(64), 0, st, d_tot.as<CbTotal>(), d_state.as<CbState>(), S, it,
                             cfg.convergence_threshold));
            SCANN_HIP_CHECK(hipMemcpyAsync(hs.data(), d_state.p, (size_t)S * sizeof(CbState), hipMemcpyDeviceToHost, st));
            SCANN_HIP_CHECK(hipStreamSynchronize(st));
            bool active = false;
            for (const auto &h : hs) active = active || !h.frozen;
            if (!active) break;
            // update_centers of the active subspaces: members of every (subspace, code) in ascending row order
            SCANN_TRY(launch(cb_make_pairs_kernel, dim3((uint32_t)ceil_div_u64(total, 256)), dim3(256), 0, st,
                             d_code.as<uint8_t>(), n, S, K, d_keys.as<uint32_t>(), d_rows.as<uint32_t>()));
            SCANN_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(d_tmp.p, tmp_bytes, d_keys.as<uint32_t>(),
                                                               d_skeys.as<uint32_t>(), d_rows.as<uint32_t>(),
                                                               d_srows.as<uint32_t>(), (int)total, 0, end_bit, st));
            SCANN_TRY(launch(cb_offsets_kernel, dim3(ceil_div_u32(S * K + 1, 256)), dim3(256), 0, st, d_skeys.as<uint32_t>(),
                             total, S * K, d_off.as<uint32_t>()));
            SCANN_TRY(launch(cb_gather_kernel, dim3((uint32_t)ceil_div_u64(total * dsub, 256)), dim3(256), 0, st, a,
                             d_srows.as<uint32_t>(), state_words, d_grows.as<float>()));
            SCANN_TRY(km_update_batched(w0, d_grows.as<float>(), d_off.as<uint32_t>(), d_codebook, k, K, S, state_words + 6,
                                        kCbStateWords, st));
        }
    }
    if (k < K)
        SCANN_TRY(launch(cb_pad_kernel, dim3(ceil_div_u32(S * (K - k) * dsub, 256)), dim3(256), 0, st, d_codebook, S, K, k,
                         dsub));
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    if (rep)
        for (uint32_t s = 0; s < S; ++s) {
            rep->subspace_iterations[s] = hs[s].iters;
            rep->subspace_converged[s] = (int32_t)hs[s].converged;
        }
    *lloyd_ms += ms_since(t);
    return SCANN_HIP_OK;
}

// Codebook::train as scann.hpp's detail::train_codebook runs it: one seeding and one Lloyd loop per subspace
int train_codebook_per_subspace(const BfIndexDev &tv, const scann_hip_build_config &cfg, uint32_t dsub, uint32_t k,
                                float *d_codebook, KmScratch &sc, hipStream_t st, scann_hip_build_report *rep,
                                float *seed_ms, float *lloyd_ms) {
    const uint32_t S = cfg.num_subspaces, K = cfg.num_codes;
    DevBuf d_sub, d_assign;
    SCANN_TRY(d_sub.ensure((size_t)k * dsub * 4));
    SCANN_TRY(d_assign.ensure(tv.n * 4));
    auto t = std::chrono::steady_clock::now();
    for (uint32_t s = 0; s < S; ++s) {
        SCANN_TRY(bf_kmeans_init_pp_device(tv, s * dsub, dsub, k, cfg.seed + s, cfg.simd_threshold, d_sub.as<float>(), sc, st));
        *seed_ms += ms_since(t);
        uint32_t iters = 0;
        int conv = 0;
        SCANN_TRY(bf_kmeans_lloyd_device(tv, s * dsub, dsub, d_sub.as<float>(), k, cfg.training_iterations,
                                         cfg.convergence_threshold, cfg.simd_threshold, d_assign.as<uint32_t>(), false, sc,
                                         nullptr, &iters, &conv, st));
        SCANN_TRY(launch(cb_store_subspace_kernel, dim3(ceil_div_u32(K * dsub, 256)), dim3(256), 0, st, d_sub.as<float>(),
                         d_codebook + (size_t)s * K * dsub, K, k, dsub));
        SCANN_HIP_CHECK(hipStreamSynchronize(st));
        if (rep) {
            rep->subspace_iterations[s] = iters;
            rep->subspace_converged[s] = conv;
        }
        *lloyd_ms += ms_since(t);
    }
    return SCANN_HIP_OK;
}

}  // namespace

int build_check(const BfIndexDev &src, const scann_hip_build_config &cfg) {
    if (src.fmt || !src.rows) return fail(SCANN_HIP_INVALID_ARGUMENT, "the index holds quantized rows, not f32 rows");
    if (src.n == 0)   // tree_x_hybrid/mod.rs:132-134, hashes/hasher.rs:110-112
        return fail(SCANN_HIP_INVALID_ARGUMENT, "Cannot build from empty dataset");
    if (src.n > 0x7FFFFFFFull) return fail(SCANN_HIP_OUT_OF_RANGE, "device build: at most 2^31 - 1 rows");
    if (cfg.distance_measure < SCANN_HIP_SQUARED_L2 || cfg.distance_measure > SCANN_HIP_COSINE)
        return fail(SCANN_HIP_UNIMPLEMENTED, "distance_measure must be SquaredL2, L2, DotProduct, L1 or Cosine");
    const uint32_t S = cfg.num_subspaces, K = cfg.num_codes;
    if (S == 0 || src.dim % S != 0)   // codebook.rs:154-159
        return fail(SCANN_HIP_INVALID_ARGUMENT, "Dimensionality " + std::to_string(src.dim) +
                                                    " must be divisible by num_subspaces " + std::to_string(S));
    if (K == 0 || K > 256) return fail(SCANN_HIP_UNIMPLEMENTED, "num_codes must be 1..256");
    const uint32_t bits = K <= 16 ? 4u : 8u;
    if (bits == 4 && (S % 8 != 0 || S > 64 || S == 40 || S == 56))
        return fail(SCANN_HIP_UNIMPLEMENTED, "num_subspaces must be 8,16,24,32,48 or 64 for num_codes <= 16");
    if (bits == 8 && S != 4 && S != 8 && S != 16)
        return fail(SCANN_HIP_UNIMPLEMENTED, "num_subspaces must be 4, 8 or 16 for 16 < num_codes <= 256");
    if (std::min<uint64_t>(cfg.num_partitions, src.n) > kMaxLeavesSelect)
        return fail(SCANN_HIP_UNIMPLEMENTED, "num_partitions > 16384");
    // the assignment kernels stage at least 8 centres of ceil(d / 4) * 4 values (bf.hip): whole rows for the partitioner
    // and the residual tokens, a subspace's columns for the codebook
    const uint32_t widest = cfg.num_partitions ? src.dim : src.dim / S;
    if ((size_t)8 * ((widest + 3u) & ~3u) * 4 > kMaxLdsBytes)
        return fail(SCANN_HIP_RESOURCE_EXHAUSTED, "kernel needs more than 160 KB of LDS");
    return SCANN_HIP_OK;
}

// Steps 2-5 on the partitioner's outputs, whichever partitioner made them: out->centers / leaf_off / leaf_ids / off / L
// and d_leaf (the leaf of every datapoint) for a tree, nothing for a flat hasher.  ms[2] also holds what the caller
// spent since `t` (the flat partitioner's CSR); stages 2..5 of stage_ms.
static int build_after_partition(const BfIndexDev &src, const scann_hip_build_config &cfg, bool tree, hipStream_t st,
                                 BuildParts *out, const DevBuf &d_leaf, KmScratch &sc, float *ms,
                                 std::chrono::steady_clock::time_point t, scann_hip_build_report *rep) {
    const uint64_t n = src.n;
    const uint32_t dim = src.dim, stride = src.stride, S = cfg.num_subspaces, K = cfg.num_codes, dsub = dim / S;
    const bool residual = tree && cfg.use_residuals;
    const uint32_t L = out->L;
    const uint32_t bits = K <= 16 ? 4u : 8u, nw = bits == 4 ? S / 8 : S / 4;
    DevBuf d_token, d_train, d_code8;
    if (tree) {
        // ---- 2 training rows: residuals against partition(x, 1), datapoint order ----
        if (residual) {
            SCANN_TRY(d_token.ensure(n * 4));
            SCANN_TRY(d_train.ensure(n * stride * 4));
            SCANN_TRY(bf_assign_nearest_device(src, out->centers.as<float>(), L, d_token.as<uint32_t>(), nullptr, st));
            const int vec = ((stride & 3u) == 0 && (reinterpret_cast<uintptr_t>(src.rows) & 15u) == 0) ? 1 : 0;
            const uint64_t threads = vec ? n * (stride >> 2) : n * stride;
            SCANN_TRY(launch(build_residual_kernel, dim3((uint32_t)ceil_div_u64(threads, 256)), dim3(256), 0, st, src.rows, n,
                             dim, stride, (const float *)out->centers.as<float>(), (const uint32_t *)d_token.as<uint32_t>(),
                             d_train.as<float>(), vec));
        }
        SCANN_HIP_CHECK(hipStreamSynchronize(st));
        ms[2] = ms_since(t);
    }

    // ---- 3 codebook ----
    BfIndexDev tv = src;
    if (residual) tv.rows = d_train.as<float>();
    const uint32_t kc = (uint32_t)std::min<uint64_t>(K, n);
    SCANN_TRY(out->codebook.ensure((size_t)S * K * dsub * 4));
    const uint32_t G = cb_group_size(S, kc, dsub);
    const bool batched = cfg.batched_codebook && dsub < cfg.simd_threshold && G >= 1 && n * S <= 0x7FFFFFFFull;
    t = std::chrono::steady_clock::now();
    if (batched)
        SCANN_TRY(train_codebook_batched(tv, cfg, dsub, kc, G, out->codebook.as<float>(), st, rep, &ms[3], &ms[4]));
    else
        SCANN_TRY(train_codebook_per_subspace(tv, cfg, dsub, kc, out->codebook.as<float>(), sc, st, rep, &ms[3], &ms[4]));

    // ---- 4 codes: Codebook::encode of x - centres[leaf], through the CSR permutation into packed words ----
    t = std::chrono::steady_clock::now();
    SCANN_TRY(d_code8.ensure(n * S));
    SCANN_TRY(out->codes.ensure(n * nw * 4));
    SCANN_TRY(launch_encode(out->codebook.as<float>(), S, K, dsub, src.rows, n, stride,
                            residual ? out->centers.as<float>() : nullptr, residual ? d_leaf.as<uint32_t>() : nullptr,
                            d_code8.as<uint8_t>(), st));
    SCANN_TRY(launch(build_pack_codes_kernel, dim3((uint32_t)ceil_div_u64(n * nw, 256)), dim3(256), 0, st,
                     (const uint8_t *)d_code8.as<uint8_t>(), (const uint32_t *)(tree ? out->leaf_ids.as<uint32_t>() : nullptr), n,
                     S, nw, bits, out->codes.as<uint32_t>()));
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    ms[5] = ms_since(t);
    if (rep) std::memcpy(rep->stage_ms, ms, 6 * sizeof(float));
    return SCANN_HIP_OK;
}

int build_txh_device(const BfIndexDev &src, const scann_hip_build_config &cfg, hipStream_t st, BuildParts *out,
                     scann_hip_build_report *rep) {
    SCANN_TRY(build_check(src, cfg));
    const uint64_t n = src.n;
    const uint32_t dim = src.dim;
    const bool tree = cfg.num_partitions != 0;
    const uint32_t L = tree ? (uint32_t)std::min<uint64_t>(cfg.num_partitions, n) : 1u;   // kmeans.rs:171-175
    float ms[6] = {};
    KmScratch sc;
    DevBuf d_leaf;
    auto t = std::chrono::steady_clock::now();
    out->L = L;
    out->off.assign((size_t)L + 1, 0u);
    SCANN_TRY(out->leaf_off.ensure(((size_t)L + 1) * 4));
    if (tree) {
        // ---- 1 partitioner ----
        SCANN_TRY(out->centers.ensure((size_t)L * dim * 4));
        SCANN_TRY(d_leaf.ensure(n * 4));
        SCANN_TRY(bf_kmeans_init_pp_device(src, 0, dim, L, cfg.kmeans_seed, cfg.simd_threshold, out->centers.as<float>(), sc, st));
        ms[0] = ms_since(t);
        double inertia = 0.0;
        uint32_t iters = 0;
        int conv = 0;
        SCANN_TRY(bf_kmeans_lloyd_device(src, 0, dim, out->centers.as<float>(), L, cfg.kmeans_iterations,
                                         cfg.kmeans_convergence, cfg.simd_threshold, d_leaf.as<uint32_t>(), true, sc,
                                         &inertia, &iters, &conv, st));
        SCANN_HIP_CHECK(hipStreamSynchronize(st));
        if (rep) {
            rep->partition_iterations = iters;
            rep->partition_converged = conv;
            rep->partition_inertia = inertia;
        }
        ms[1] = ms_since(t);
        // ---- CSR: the sorted (leaf << 32 | index) keys are the lists, ascending datapoint index inside each leaf ----
        SCANN_TRY(out->leaf_ids.ensure(n * 4));
        SCANN_TRY(bf_kmeans_csr_device(d_leaf.as<uint32_t>(), n, L, sc, st));
        SCANN_TRY(launch(build_ids_kernel, dim3((uint32_t)ceil_div_u64(n, 256)), dim3(256), 0, st, sc.dsorted.as<uint64_t>(), n,
                         out->leaf_ids.as<uint32_t>()));
        SCANN_HIP_CHECK(hipMemcpyAsync(out->leaf_off.p, sc.doff.p, ((size_t)L + 1) * 4, hipMemcpyDeviceToDevice, st));
        SCANN_HIP_CHECK(hipMemcpyAsync(out->off.data(), sc.doff.p, ((size_t)L + 1) * 4, hipMemcpyDeviceToHost, st));
    } else {
        out->off[1] = (uint32_t)n;
        SCANN_HIP_CHECK(hipMemcpyAsync(out->leaf_off.p, out->off.data(), 8, hipMemcpyHostToDevice, st));
        SCANN_HIP_CHECK(hipStreamSynchronize(st));
    }
    return build_after_partition(src, cfg, tree, st, out, d_leaf, sc, ms, t, rep);
}

int build_txh_hierarchical_device(const BfIndexDev &src, const scann_hip_tree_config &tree,
                                  const scann_hip_build_config &cfg, hipStream_t st, BuildParts *out,
                                  scann_hip_build_report *rep, scann_hip_tree_report *trep) {
    SCANN_TRY(build_check(src, cfg));
    float ms[6] = {};
    KmScratch sc;
    DevBuf d_leaf;
    scann_hip_build_report tree_rep;
    std::memset(&tree_rep, 0, sizeof(tree_rep));
    SCANN_TRY(ktree_build_device(src, tree, cfg.simd_threshold, st, out, &d_leaf, &tree_rep, trep));
    if (rep) {
        rep->partition_iterations = tree_rep.partition_iterations;
        rep->partition_converged = tree_rep.partition_converged;
        rep->partition_inertia = tree_rep.partition_inertia;
    }
    ms[0] = tree_rep.stage_ms[0];
    ms[1] = tree_rep.stage_ms[1];
    return build_after_partition(src, cfg, true, st, out, d_leaf, sc, ms, std::chrono::steady_clock::now(), rep);
}

}  // namespace scann

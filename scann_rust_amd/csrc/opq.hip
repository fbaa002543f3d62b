// opq.hip -- OPQ training on the device (opq.h): the sample gather, the distortion, the fused-decode
// cross-covariance on v_mfma_f64_16x16x4_f64, the one-sided Jacobi SVD and the polar assembly, the alternation's
// driver and the entry points scann_hip_opq_cross_covariance / scann_hip_opq_polar.  (scann_hip_opq_train itself is
// in api_create.hip, which owns scann_hip_index.)
#include "opq.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "build.h"
#include "handle.h"
#include "launch.h"
#include "project.h"
#include "txh.h"

namespace scann {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kOpqPitch = kOpqPanel + 4;   // f64 words per staged row: rows r and r + 1 start 8 banks apart
static_assert(kOpqPanel == 64 && kOpqStage == 32, "the thread maps below are written for 64-column panels, 32-row stages");

// ---- 1 sample ------------------------------------------------------------------------------------------------------
// X[t][:] = rows[splitmix64(seed, 0, ns)[t] % n][:dim]; one thread per element (pca_sample_kernel's stream)
__global__ __launch_bounds__(256) void opq_gather_kernel(const float *__restrict__ rows, uint64_t n, uint32_t dim, uint32_t stride,
                                                         uint64_t seed, uint64_t ns, float *__restrict__ X) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ns * dim) return;
    const uint64_t t = e / dim;
    const uint32_t j = (uint32_t)(e - t * dim);
    uint64_t z = seed + (t + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    X[e] = rows[(z % n) * stride + j];
}

// ---- 2c distortion -------------------------------------------------------------------------------------------------
// sum in a fixed order: a thread's strided elements ascending, then a halving tree over the 256 threads
__device__ __forceinline__ double opq_block_sum(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + o];
        __syncthreads();
    }
    const double tot = red[0];
    __syncthreads();
    return tot;
}

// err[r] = sum over j of (y[r][j] - codebook[s][code[r][s]][j - s dsub])^2 in f64: wave w of the block owns row
// 4 blockIdx.x + w, a lane its columns lane, lane + 64, ... ascending, then a halving tree over the lanes
__global__ __launch_bounds__(256) void opq_row_error_kernel(const float *__restrict__ Y, uint64_t n, uint32_t dim,
                                                            const float *__restrict__ codebook, uint32_t K, uint32_t dsub,
                                                            const uint8_t *__restrict__ codes, uint32_t S,
                                                            double *__restrict__ err) {
    const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (r >= n) return;   // (wave-uniform; no barrier below)
    double e = 0.0;
    for (uint32_t j = lane; j < dim; j += 64) {
        const uint32_t s = j / dsub;
        const double c = (double)codebook[((size_t)s * K + codes[r * S + s]) * dsub + (j - s * dsub)];
        const double t = (double)Y[r * dim + j] - c;
        e = e + t * t;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) e = e + __shfl_down(e, o);
    if (lane == 0) err[r] = e;
}

// *out = (sum of v[0 .. n)) * scale, one workgroup
__global__ __launch_bounds__(256) void opq_sum_kernel(const double *__restrict__ v, uint64_t n, double scale, double *__restrict__ out) {
    __shared__ double red[256];
    double s = 0.0;
    for (uint64_t i = threadIdx.x; i < n; i += 256) s = s + v[i];
    const double tot = opq_block_sum(s, red);
    if (threadIdx.x == 0) *out = tot * scale;
}

// ---- 2d cross-covariance -------------------------------------------------------------------------------------------
// One stage of 32 rows: wave w owns the 16-column band w of the A panel against the four 16-column tiles of the B panel,
// D = A * B + D on v_mfma_f64_16x16x4_f64 with
//   A: lane l holds A[i = l & 15][k = l >> 4]  = xa[4 kk + (l >> 4)][16 w + (l & 15)]
//   B: lane l holds B[k = l >> 4][j = l & 15]  = yb[4 kk + (l >> 4)][16 t + (l & 15)]
//   D: register g of lane l is D[row = (l >> 4) + 4 g][col = l & 15]
// so acc[t][g] += sum over the stage's rows of xa[.][16 w + (l >> 4) + 4 g] * yb[.][16 t + (l & 15)].
__device__ __forceinline__ void opq_mfma_stage(const double (*xa)[kOpqPitch], const double (*yb)[kOpqPitch], f64x4 (&acc)[4],
                                               uint32_t w, uint32_t lane) {
#pragma unroll
    for (uint32_t kk = 0; kk < kOpqStage / 4; ++kk) {
        const uint32_t r = 4u * kk + (lane >> 4);
        const double a = xa[r][16u * w + (lane & 15u)];
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t) {
            const double b = yb[r][16u * t + (lane & 15u)];
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
        }
    }
}

struct OpqCrossArgs {
    const float *rows;       // [n][stride]
    uint64_t n, per;         // per: rows of one run (a multiple of kOpqStage)
    uint32_t dim, stride, npanels;
    const float *codebook;   // [S][K][dsub]
    uint32_t S, K, dsub;
    const uint8_t *codes;    // [n][code_pitch]
    uint32_t code_pitch, packed4;
};

// Workgroup (pair, run): panel pair (I, J) -- columns 64 I .. of X against columns 64 J .. of Yhat, EVERY pair (M is not
// symmetric) -- over the run's rows, staged 32 at a time:
//   xa[row][column of I] = the X element widened;
//   yb[row][column of J] = the centroid element the row's code selects, widened: thread (sc, sr) owns column 64 J + sc of
//     rows sr, sr + 4, ...; its subspace s = column / dsub is fixed, so it reads one code byte (or nibble) per row and
//     one float of cbs, the panel's slice of the codebook in LDS: cbs[c][sc] = codebook[s][c][column - s dsub] (bank =
//     sc whatever the code, so a wave's 64 reads never conflict).  Yhat is never written to memory.
// Rows past the run's end and columns past dim are zeros and are never read.  The partial panel ([64][64] f64 per
// (run, pair)) is written whole; opq_cross_reduce_kernel adds the runs in ascending order.
__global__ __launch_bounds__(256) void opq_cross_kernel(OpqCrossArgs a, double *__restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) double opq_lds[];
    double(*xa)[kOpqPitch] = reinterpret_cast<double(*)[kOpqPitch]>(opq_lds);
    double(*yb)[kOpqPitch] = xa + kOpqStage;
    float *cbs = reinterpret_cast<float *>(yb + kOpqStage);   // [K][64]
    const uint32_t I = blockIdx.x / a.npanels, J = blockIdx.x - I * a.npanels;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint64_t t0 = (uint64_t)blockIdx.y * a.per, t1 = std::min<uint64_t>(a.n, t0 + a.per);
    for (uint32_t e = tid; e < a.K * kOpqPanel; e += 256) {
        const uint32_t c = e / kOpqPanel, col = J * kOpqPanel + (e % kOpqPanel);
        float v = 0.0f;
        if (col < a.dim) {
            const uint32_t s = col / a.dsub;
            v = a.codebook[((size_t)s * a.K + c) * a.dsub + (col - s * a.dsub)];
        }
        cbs[e] = v;
    }
    const uint32_t sc = tid & 63u, sr = tid >> 6;   // staging: column sc of rows sr + 4 u
    const uint32_t ca = I * kOpqPanel + sc, cb = J * kOpqPanel + sc;
    const uint32_t s = cb / a.dsub;                 // (unused when cb >= dim)
    const uint32_t cbyte = a.packed4 ? s >> 1 : s, cshift = a.packed4 ? 4u * (s & 1u) : 0u, cmask = a.packed4 ? 15u : 255u;
    f64x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (uint64_t s0 = t0; s0 < t1; s0 += kOpqStage) {
        __syncthreads();   // the previous stage is read; (first pass) the codebook slice is staged
#pragma unroll
        for (uint32_t u = 0; u < kOpqStage / 4; ++u) {
            const uint32_t r = sr + 4u * u;
            double x = 0.0, y = 0.0;
            if (s0 + r < t1) {
                if (ca < a.dim) x = (double)a.rows[(s0 + r) * a.stride + ca];
                if (cb < a.dim) {
                    const uint32_t code = ((uint32_t)a.codes[(s0 + r) * a.code_pitch + cbyte] >> cshift) & cmask;
                    y = (double)cbs[code * kOpqPanel + sc];
                }
            }
            xa[r][sc] = x;
            yb[r][sc] = y;
        }
        __syncthreads();
        opq_mfma_stage(xa, yb, acc, w, lane);
    }
    double *out = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (kOpqPanel * kOpqPanel);
#pragma unroll
    for (uint32_t t = 0; t < 4; ++t)
#pragma unroll
        for (uint32_t g = 0; g < 4; ++g)
            out[(size_t)(16u * w + (lane >> 4) + 4u * g) * kOpqPanel + 16u * t + (lane & 15u)] = acc[t][g];
}

// M[i][j] = sum over the runs, ascending; stored at i * dim + j, or at j * dim + i when transposed
__global__ __launch_bounds__(256) void opq_cross_reduce_kernel(const double *__restrict__ partial, uint32_t nruns, uint32_t npairs,
                                                               uint32_t npanels, uint32_t dim, int transposed,
                                                               double *__restrict__ M) {
    const uint32_t I = blockIdx.x / npanels, J = blockIdx.x - I * npanels;
    for (uint32_t e = threadIdx.x; e < kOpqPanel * kOpqPanel; e += 256) {
        const uint32_t i = I * kOpqPanel + e / kOpqPanel, j = J * kOpqPanel + e % kOpqPanel;
        if (i >= dim || j >= dim) continue;
        double s = 0.0;
        for (uint32_t r = 0; r < nruns; ++r) s = s + partial[((size_t)r * npairs + blockIdx.x) * (kOpqPanel * kOpqPanel) + e];
        M[transposed ? (size_t)j * dim + i : (size_t)i * dim + j] = s;
    }
}

// ---- 2e polar factor -----------------------------------------------------------------------------------------------
// Round `round` (0 .. m - 2) of the circle method over m players (m even), pca_jacobi_round_kernel's pairing: pair 0 is
// (round, m - 1), pair k >= 1 is ((round + k) mod (m - 1), (round - k) mod (m - 1)); p < q.
__device__ __forceinline__ void opq_pair(uint32_t k, uint32_t round, uint32_t m, uint32_t *p, uint32_t *q) {
    uint32_t a, b;
    if (k == 0) {
        a = round;
        b = m - 1;
    } else {
        a = (round + k) % (m - 1);
        b = (round + (m - 1) - k) % (m - 1);
    }
    *p = a < b ? a : b;
    *q = a < b ? b : a;
}

// One round of the one-sided (Hestenes) Jacobi SVD, one workgroup per pair (p, q) of the round.  Mt and Vt are [d][d]
// row-major, so column p of M and column p of V are the contiguous rows p.  The workgroup holds rows p and q in
// registers (NU doubles each per lane, element lane + 256 u), reduces alpha = ||m_p||^2, beta = ||m_q||^2 and gamma =
// m_p . m_q (a lane's elements ascending, then a halving tree over the 256 lanes), and applies
//   zeta = (beta - alpha) / (2 gamma), t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)), c = 1 / sqrt(1 + t^2), s = t c
//   m_p' = c m_p - s m_q, m_q' = s m_p + c m_q        (and the same to rows p, q of Vt)
// in place: the round's pairs are disjoint.  gamma == 0 or a zero column: no rotation.  rec[pair] keeps the largest
// |gamma| / sqrt(alpha beta) the pair slot has seen since the host cleared it (a NaN sticks).  m = d rounded up to even;
// the pair that holds player d of an odd d is the bye.
template <int NU>
__global__ __launch_bounds__(256) void opq_hestenes_round_kernel(double *__restrict__ Mt, double *__restrict__ Vt, uint32_t d,
                                                                 uint32_t m, uint32_t round, double *__restrict__ rec) {
    __shared__ double red[3][256];
    uint32_t p, q;
    opq_pair(blockIdx.x, round, m, &p, &q);
    if (q >= d) return;   // (block-uniform) the bye
    const uint32_t tid = threadIdx.x;
    double *rp = Mt + (size_t)p * d, *rq = Mt + (size_t)q * d;
    double mp[NU], mq[NU];
    double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const uint32_t i = tid + 256u * u;
        mp[u] = i < d ? rp[i] : 0.0;
        mq[u] = i < d ? rq[i] : 0.0;
        al = al + mp[u] * mp[u];
        be = be + mq[u] * mq[u];
        ga = ga + mp[u] * mq[u];
    }
    red[0][tid] = al;
    red[1][tid] = be;
    red[2][tid] = ga;
    __syncthreads();
    for (uint32_t o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            red[0][tid] = red[0][tid] + red[0][tid + o];
            red[1][tid] = red[1][tid] + red[1][tid + o];
            red[2][tid] = red[2][tid] + red[2][tid + o];
        }
        __syncthreads();
    }
    const double alpha = red[0][0], beta = red[1][0], gamma = red[2][0];
    if (gamma == 0.0 || alpha == 0.0 || beta == 0.0) return;   // (block-uniform)
    if (tid == 0) {
        const double r = fabs(gamma) / (sqrt(alpha) * sqrt(beta));
        if (!(r <= rec[blockIdx.x])) rec[blockIdx.x] = r;
    }
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const uint32_t i = tid + 256u * u;
        if (i < d) {
            rp[i] = c * mp[u] - s * mq[u];
            rq[i] = s * mp[u] + c * mq[u];
        }
    }
    double *vp = Vt + (size_t)p * d, *vq = Vt + (size_t)q * d;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const uint32_t i = tid + 256u * u;
        if (i < d) {
            const double a = vp[i], b = vq[i];
            vp[i] = c * a - s * b;
            vq[i] = s * a + c * b;
        }
    }
}

// A = 0 with a unit diagonal, [d][d]
__global__ __launch_bounds__(256) void opq_identity_kernel(double *__restrict__ A, uint32_t d) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < (uint64_t)d * d) A[e] = (e / d == e % d) ? 1.0 : 0.0;
}

__global__ __launch_bounds__(256) void opq_clear_kernel(double *__restrict__ v, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) v[i] = 0.0;
}

// sigma[j] = ||row j of Mt||, one workgroup per row
__global__ __launch_bounds__(256) void opq_sigma_kernel(const double *__restrict__ Mt, uint32_t d, double *__restrict__ sigma) {
    __shared__ double red[256];
    const double *r = Mt + (size_t)blockIdx.x * d;
    double s = 0.0;
    for (uint32_t i = threadIdx.x; i < d; i += 256) s = s + r[i] * r[i];
    const double tot = opq_block_sum(s, red);
    if (threadIdx.x == 0) sigma[blockIdx.x] = sqrt(tot);
}

// R[i][k] = sum over j, ascending, of (Mt[j][i] / sigma[j]) * Vt[j][k], cast to f32: the panel pair (I, J) = (i's, k's)
// on the cross kernel's tile map, the j range staged 32 at a time.  A column with sigma[j] == 0 contributes nothing.
// Stored at i * d + k, or at k * d + i when transposed.
__global__ __launch_bounds__(256) void opq_polar_assemble_kernel(const double *__restrict__ Mt, const double *__restrict__ Vt,
                                                                 const double *__restrict__ sigma, uint32_t d, uint32_t npanels,
                                                                 int transposed, float *__restrict__ R) {
    __shared__ double xa[kOpqStage][kOpqPitch];
    __shared__ double yb[kOpqStage][kOpqPitch];
    const uint32_t I = blockIdx.x / npanels, J = blockIdx.x - I * npanels;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t sc = tid & 63u, sr = tid >> 6;
    const uint32_t ca = I * kOpqPanel + sc, cb = J * kOpqPanel + sc;
    f64x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (uint32_t j0 = 0; j0 < d; j0 += kOpqStage) {
        __syncthreads();
#pragma unroll
        for (uint32_t u = 0; u < kOpqStage / 4; ++u) {
            const uint32_t r = sr + 4u * u, j = j0 + r;
            double x = 0.0, y = 0.0;
            if (j < d) {
                const double sg = sigma[j];
                if (ca < d && sg > 0.0) x = Mt[(size_t)j * d + ca] / sg;
                if (cb < d) y = Vt[(size_t)j * d + cb];
            }
            xa[r][sc] = x;
            yb[r][sc] = y;
        }
        __syncthreads();
        opq_mfma_stage(xa, yb, acc, w, lane);
    }
#pragma unroll
    for (uint32_t t = 0; t < 4; ++t)
#pragma unroll
        for (uint32_t g = 0; g < 4; ++g) {
            const uint32_t i = I * kOpqPanel + 16u * w + (lane >> 4) + 4u * g, k = J * kOpqPanel + 16u * t + (lane & 15u);
            if (i < d && k < d) R[transposed ? (size_t)k * d + i : (size_t)i * d + k] = (float)acc[t][g];
        }
}

// ---- drivers -------------------------------------------------------------------------------------------------------
int opq_cross_device(const float *d_rows, uint64_t n, uint32_t d, uint32_t stride, const float *d_codebook, uint32_t S,
                     uint32_t K, uint32_t dsub, const uint8_t *d_codes, int packed4, double *d_out, bool transposed,
                     DevBuf &d_partial, hipStream_t st) {
    const uint32_t npanels = ceil_div_u32(d, kOpqPanel), npairs = npanels * npanels;
    const size_t panel_bytes = (size_t)kOpqPanel * kOpqPanel * 8;
    uint64_t runs = std::min<uint64_t>(kOpqMaxRuns, ceil_div_u64(n, kOpqMinRun));
    runs = std::max<uint64_t>(1, std::min<uint64_t>(runs, kOpqCrossWorkspaceBytes / (npairs * panel_bytes)));
    const uint64_t per = ceil_div_u64(ceil_div_u64(n, runs), kOpqStage) * kOpqStage;
    runs = ceil_div_u64(n, per);
    SCANN_TRY(d_partial.ensure((size_t)runs * npairs * panel_bytes));
    OpqCrossArgs a;
    a.rows = d_rows; a.n = n; a.per = per; a.dim = d; a.stride = stride; a.npanels = npanels;
    a.codebook = d_codebook; a.S = S; a.K = K; a.dsub = dsub;
    a.codes = d_codes; a.code_pitch = packed4 ? (S + 1) / 2 : S; a.packed4 = packed4 ? 1u : 0u;
    const size_t lds = (size_t)2 * kOpqStage * kOpqPitch * 8 + (size_t)K * kOpqPanel * 4;
    SCANN_TRY(launch(opq_cross_kernel, dim3(npairs, (uint32_t)runs), dim3(256), lds, st, a, d_partial.as<double>()));
    SCANN_TRY(launch(opq_cross_reduce_kernel, dim3(npairs), dim3(256), 0, st, (const double *)d_partial.as<double>(),
                     (uint32_t)runs, npairs, npanels, d, transposed ? 1 : 0, d_out));
    return SCANN_HIP_OK;
}

int opq_polar_device(double *d_mt, uint32_t d, float *d_r, bool transposed, bool assemble_singular, double *sigma,
                     uint32_t *out_sweeps, int *out_converged, double *out_min_over_max, int *out_singular,
                     hipStream_t st) {
    const uint32_t m = (d + 1u) & ~1u, pairs = m / 2;
    DevBuf d_vt, d_rec, d_sigma;
    SCANN_TRY(d_vt.ensure((size_t)d * d * 8));
    SCANN_TRY(d_rec.ensure((size_t)pairs * 8));
    SCANN_TRY(d_sigma.ensure((size_t)d * 8));
    SCANN_TRY(launch(opq_identity_kernel, dim3((uint32_t)ceil_div_u64((uint64_t)d * d, 256)), dim3(256), 0, st,
                     d_vt.as<double>(), d));
    const int nu = d <= 256 ? 1 : d <= 512 ? 2 : d <= 1024 ? 4 : 8;
    const double tol = std::ldexp((double)d, -52);
    std::vector<double> rec(pairs);
    uint32_t sweeps = 0;
    int converged = 0;
    while (!converged && sweeps < kOpqMaxSweeps) {
        SCANN_TRY(launch(opq_clear_kernel, dim3(ceil_div_u32(pairs, 256)), dim3(256), 0, st, d_rec.as<double>(), pairs));
        for (uint32_t round = 0; round + 1 < m; ++round) {
            const int status = with_value<1, 2, 4, 8>(nu, [&](auto u) {
                return launch(opq_hestenes_round_kernel<u()>, dim3(pairs), dim3(256), 0, st, d_mt, d_vt.as<double>(), d, m,
                              round, d_rec.as<double>());
            });
            SCANN_TRY(status);
        }
        ++sweeps;
        SCANN_HIP_CHECK(hipMemcpyAsync(rec.data(), d_rec.p, (size_t)pairs * 8, hipMemcpyDeviceToHost, st));
        SCANN_HIP_CHECK(hipStreamSynchronize(st));
        converged = 1;
        for (double r : rec) converged = (converged && r <= tol) ? 1 : 0;   // (a NaN is not <= tol)
    }
    SCANN_TRY(launch(opq_sigma_kernel, dim3(d), dim3(256), 0, st, (const double *)d_mt, d, d_sigma.as<double>()));
    SCANN_HIP_CHECK(hipMemcpyAsync(sigma, d_sigma.p, (size_t)d * 8, hipMemcpyDeviceToHost, st));
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    double smin = sigma[0], smax = sigma[0];
    for (uint32_t j = 1; j < d; ++j) {
        smin = sigma[j] < smin ? sigma[j] : smin;
        smax = sigma[j] > smax ? sigma[j] : smax;
    }
    const int singular = smin > std::ldexp(smax, kOpqSingularExp) ? 0 : 1;   // (M = 0 and a NaN are singular)
    if (!singular || assemble_singular) {
        const uint32_t npanels = ceil_div_u32(d, kOpqPanel);
        SCANN_TRY(launch(opq_polar_assemble_kernel, dim3(npanels * npanels), dim3(256), 0, st, (const double *)d_mt,
                         (const double *)d_vt.as<double>(), (const double *)d_sigma.as<double>(), d, npanels,
                         transposed ? 1 : 0, d_r));
        SCANN_HIP_CHECK(hipStreamSynchronize(st));
    }
    if (out_sweeps) *out_sweeps = sweeps;
    if (out_converged) *out_converged = converged;
    if (out_min_over_max) *out_min_over_max = smax > 0.0 ? smin / smax : 0.0;
    if (out_singular) *out_singular = singular;
    return SCANN_HIP_OK;
}

// the codebook step's configuration: a flat hasher's step 3 with the OPQ configuration's fields
static scann_hip_build_config opq_build_config(const scann_hip_opq_config &cfg) {
    scann_hip_build_config b;
    scann_hip_build_config_default(&b);
    b.num_partitions = 0;
    b.num_subspaces = cfg.num_subspaces;
    b.num_codes = cfg.num_codes;
    b.training_iterations = cfg.training_iterations;
    b.convergence_threshold = cfg.convergence_threshold;
    b.seed = cfg.seed;
    b.simd_threshold = cfg.simd_threshold;
    return b;
}

int opq_check(const BfIndexDev &src, const scann_hip_opq_config &cfg, const scann_hip_projection *init) {
    if (src.fmt || !src.rows) return fail(SCANN_HIP_INVALID_ARGUMENT, "opq_train: the index holds quantized rows, not f32 rows");
    if (src.n == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "opq_train: cannot train on an empty dataset");
    if (src.dim > kOpqMaxDim)
        return fail(SCANN_HIP_RESOURCE_EXHAUSTED, "opq_train: dim " + std::to_string(src.dim) + " is above the limit of " +
                                                      std::to_string(kOpqMaxDim) + " (the Jacobi solve is O(d^3) per sweep)");
    if (cfg.opq_iterations == 0 || cfg.opq_iterations > kOpqMaxIterations)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "opq_train: opq_iterations " + std::to_string(cfg.opq_iterations) +
                                                    " must be in 1.." + std::to_string(kOpqMaxIterations));
    if (init && (init->dev.kind != SCANN_HIP_PROJ_MATRIX || init->dev.in_dim != src.dim || init->dev.out_dim != src.dim))
        return fail(SCANN_HIP_INVALID_ARGUMENT, "opq_train: init must be a MATRIX projection of " + std::to_string(src.dim) +
                                                    " x " + std::to_string(src.dim));
    BfIndexDev view = src;   // the rotated rows: [ns][dim] at stride dim
    view.stride = src.dim;
    return build_check(view, opq_build_config(cfg));
}

static float ms_since(std::chrono::steady_clock::time_point &t) {
    const auto now = std::chrono::steady_clock::now();
    const float ms = std::chrono::duration<float, std::milli>(now - t).count();
    t = now;
    return ms;
}

int opq_train_device(scann_hip_ctx *ctx, const BfIndexDev &src, const scann_hip_opq_config &cfg,
                     const scann_hip_projection *init, hipStream_t st, scann_hip_projection **out,
                     scann_hip_opq_report *rep) {
    SCANN_TRY(opq_check(src, cfg, init));
    const uint64_t n = src.n;
    const uint32_t d = src.dim, S = cfg.num_subspaces, K = cfg.num_codes, dsub = d / S;
    const bool sampled = cfg.max_samples != 0 && cfg.max_samples < n;
    const uint64_t ns = sampled ? cfg.max_samples : n;
    if (ns > SIZE_MAX / 4 / d) return fail(SCANN_HIP_OUT_OF_RANGE, "opq_train: ns * dim overflows");
    scann_hip_opq_report r;
    std::memset(&r, 0, sizeof(r));
    auto t = std::chrono::steady_clock::now();

    // ---- 1 sample ----
    DevBuf d_x;
    const float *x = src.rows;
    uint32_t xstride = src.stride;
    if (sampled) {
        SCANN_TRY(d_x.ensure((size_t)ns * d * 4));
        SCANN_TRY(launch(opq_gather_kernel, dim3((uint32_t)ceil_div_u64(ns * d, 256)), dim3(256), 0, st, src.rows, n, d,
                         src.stride, cfg.seed ^ 0x0B9ull, ns, d_x.as<float>()));
        SCANN_HIP_CHECK(hipStreamSynchronize(st));
        x = d_x.as<float>();
        xstride = d;
    }
    r.stage_ms[0] = ms_since(t);

    std::vector<float> rot((size_t)d * d, 0.0f);   // [out][in] = R^T
    if (init) rot = init->matrix;
    else for (uint32_t i = 0; i < d; ++i) rot[(size_t)i * d + i] = 1.0f;
    DevBuf d_rot, d_next, d_y, d_codebook, d_code8, d_err, d_dist, d_mt, d_partial;
    SCANN_TRY(upload(d_rot, rot.data(), rot.size() * 4));
    SCANN_TRY(d_next.ensure(rot.size() * 4));
    SCANN_TRY(d_y.ensure((size_t)ns * d * 4));
    SCANN_TRY(d_codebook.ensure((size_t)S * K * dsub * 4));
    SCANN_TRY(d_code8.ensure((size_t)ns * S));
    SCANN_TRY(d_err.ensure((size_t)ns * 8));
    SCANN_TRY(d_dist.ensure(8));
    SCANN_TRY(d_mt.ensure((size_t)d * d * 8));
    BfIndexDev view = src;   // Y as the codebook trainer's rows
    view.rows = d_y.as<float>();
    view.n = ns;
    view.stride = d;
    view.rows_b = view.rows_bl = nullptr;
    view.norm2 = nullptr;
    view.max_norm = 0.0f;
    scann_hip_build_config bcfg = opq_build_config(cfg);
    KmScratch sc;
    std::vector<double> sigma(d);
    ProjDev pd;
    pd.kind = SCANN_HIP_PROJ_MATRIX;
    pd.in_dim = pd.out_dim = d;

    for (uint32_t it = 0; it < cfg.opq_iterations; ++it) {
        // ---- a project ----
        pd.matrix = d_rot.as<float>();
        SCANN_TRY(launch_project(pd, x, ns, xstride, d_y.as<float>(), d, st));
        SCANN_HIP_CHECK(hipStreamSynchronize(st));
        r.stage_ms[1] += ms_since(t);
        // ---- b codebook, c encode + distortion ----
        float seed_ms = 0.0f, lloyd_ms = 0.0f;
        if (it == 1) bcfg.training_iterations = cfg.inner_iterations;
        SCANN_TRY(train_codebook_device(view, bcfg, it > 0, d_codebook.as<float>(), sc, st, nullptr, &seed_ms, &lloyd_ms));
        SCANN_TRY(launch_encode(d_codebook.as<float>(), S, K, dsub, d_y.as<float>(), ns, d, nullptr, nullptr,
                                d_code8.as<uint8_t>(), st));
        SCANN_TRY(launch(opq_row_error_kernel, dim3((uint32_t)ceil_div_u64(ns, 4)), dim3(256), 0, st,
                         (const float *)d_y.as<float>(), ns, d, (const float *)d_codebook.as<float>(), K, dsub,
                         (const uint8_t *)d_code8.as<uint8_t>(), S, d_err.as<double>()));
        SCANN_TRY(launch(opq_sum_kernel, dim3(1), dim3(256), 0, st, (const double *)d_err.as<double>(), ns, 1.0 / (double)ns,
                         d_dist.as<double>()));
        SCANN_HIP_CHECK(hipMemcpyAsync(&r.distortion[it], d_dist.p, 8, hipMemcpyDeviceToHost, st));
        SCANN_HIP_CHECK(hipStreamSynchronize(st));
        r.stage_ms[2] += ms_since(t);
        // ---- d cross-covariance ----
        SCANN_TRY(opq_cross_device(x, ns, d, xstride, d_codebook.as<float>(), S, K, dsub, d_code8.as<uint8_t>(), 0,
                                   d_mt.as<double>(), true, d_partial, st));
        SCANN_HIP_CHECK(hipStreamSynchronize(st));
        r.stage_ms[3] += ms_since(t);
        // ---- e polar factor ----
        int singular = 0;
        SCANN_TRY(opq_polar_device(d_mt.as<double>(), d, d_next.as<float>(), true, false, sigma.data(), &r.sweeps[it],
                                   &r.converged[it], &r.sigma_min_over_max[it], &singular, st));
        r.stage_ms[4] += ms_since(t);
        if (singular) {
            r.stopped_singular = 1;
            break;
        }
        std::swap(d_rot.p, d_next.p);
        std::swap(d_rot.bytes, d_next.bytes);
        r.iterations_run = it + 1;
    }
    SCANN_HIP_CHECK(hipMemcpy(rot.data(), d_rot.p, rot.size() * 4, hipMemcpyDeviceToHost));
    SCANN_TRY(scann_hip_projection_create(ctx, SCANN_HIP_PROJ_MATRIX, d, d, rot.data(), nullptr, 0, out));
    if (rep) *rep = r;
    return SCANN_HIP_OK;
}

}  // namespace scann

using namespace scann;

extern "C" {

void scann_hip_opq_config_default(scann_hip_opq_config *c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->opq_iterations = 20;          // OpqConfig::new (projection/opq.rs)
    c->training_iterations = 25;
    c->inner_iterations = 1;
    c->convergence_threshold = 1e-5;
    c->seed = 42;
    c->simd_threshold = 128;
}

int scann_hip_opq_polar(scann_hip_ctx *ctx, const double *M, uint32_t d, float *out_R, double *out_singular,
                        uint32_t *out_sweeps, int *out_converged) {
    if (!ctx) return fail(SCANN_HIP_INVALID_ARGUMENT, "ctx is null");
    if (!M || !out_R || d == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "opq_polar: null M / out_R or d == 0");
    if (d > kOpqMaxDim)
        return fail(SCANN_HIP_RESOURCE_EXHAUSTED, "opq_polar: d " + std::to_string(d) + " is above the limit of " +
                                                      std::to_string(kOpqMaxDim));
    SCANN_TRY(set_device(ctx));
    std::vector<double> mt((size_t)d * d), sigma(d);
    for (uint32_t i = 0; i < d; ++i)
        for (uint32_t j = 0; j < d; ++j) mt[(size_t)j * d + i] = M[(size_t)i * d + j];
    DevBuf d_mt, d_r;
    SCANN_TRY(upload(d_mt, mt.data(), mt.size() * 8));
    SCANN_TRY(d_r.ensure((size_t)d * d * 4));
    SCANN_TRY(opq_polar_device(d_mt.as<double>(), d, d_r.as<float>(), false, true, sigma.data(), out_sweeps, out_converged,
                               nullptr, nullptr, nullptr));
    SCANN_HIP_CHECK(hipMemcpy(out_R, d_r.p, (size_t)d * d * 4, hipMemcpyDeviceToHost));
    if (out_singular) {
        std::sort(sigma.begin(), sigma.end(), [](double a, double b) { return a > b || (a == a && b != b); });   // NaNs last
        std::memcpy(out_singular, sigma.data(), (size_t)d * 8);
    }
    return SCANN_HIP_OK;
}

}  // extern "C"

// pca.hip -- PCA training on the device (pca.h): the sample, the f64 mean, the covariance on
// v_mfma_f64_16x16x4_f64, the round-robin Jacobi solve and the component pass, and the entry points
// scann_hip_projection_arrays / scann_hip_pca_last_stage_ms.  (scann_hip_pca_train itself is in api.hip, which owns
// scann_hip_index.)
#include "pca.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "launch.h"
#include "project.h"

namespace scann {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// ---- 1 sample ------------------------------------------------------------------------------------------------------
// synth.splitmix64(seed, 0, ns)[t]: the (t + 1)-th output of the stream
__global__ __launch_bounds__(256) void pca_sample_kernel(uint64_t seed, uint64_t ns, uint64_t n, uint32_t *__restrict__ sel) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= ns) return;
    uint64_t z = seed + (t + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    sel[t] = (uint32_t)(z % n);
}

// ---- 2 mean --------------------------------------------------------------------------------------------------------
// run c (blockIdx.y) covers sample positions [c * per, min(ns, (c + 1) * per)); one thread per column walks them in
// ascending order
__global__ __launch_bounds__(256) void pca_mean_runs_kernel(const float *__restrict__ rows, const uint32_t *__restrict__ sel,
                                                            uint64_t ns, uint32_t dim, uint32_t stride, uint64_t per,
                                                            double *__restrict__ runs) {
    const uint32_t col = blockIdx.x * 256 + threadIdx.x;
    if (col >= dim) return;
    const uint64_t t0 = (uint64_t)blockIdx.y * per, t1 = std::min<uint64_t>(ns, t0 + per);
    double s = 0.0;
    for (uint64_t t = t0; t < t1; ++t) {
        const uint64_t r = sel ? sel[t] : t;
        s = s + (double)rows[r * stride + col];
    }
    runs[(size_t)blockIdx.y * dim + col] = s;
}

__global__ __launch_bounds__(256) void pca_mean_final_kernel(const double *__restrict__ runs, uint32_t nruns, uint32_t dim,
                                                             uint64_t ns, double *__restrict__ mean64, float *__restrict__ mean32) {
    const uint32_t col = blockIdx.x * 256 + threadIdx.x;
    if (col >= dim) return;
    double s = 0.0;
    for (uint32_t c = 0; c < nruns; ++c) s = s + runs[(size_t)c * dim + col];
    const double m = s / (double)ns;
    mean64[col] = m;
    mean32[col] = (float)m;
}

// ---- 3 covariance --------------------------------------------------------------------------------------------------
// Workgroup (pair, run): panel pair (I, J), I <= J, of kPcaPanel columns each, over the run's rows.  The rows are staged
// kPcaCovStage at a time, widened and centred, as xa[row][column of I] and xb[row][column of J]; rows past the run's end
// and columns past dim are zeros (never read from memory).  Wave w owns the 16-column band w of I against the four
// 16-column tiles of J: one A operand and four B operands per 4 rows, D = A * B + D on v_mfma_f64_16x16x4_f64 with
//   A: lane l holds A[i = l & 15][k = l >> 4]  = xa[4 kk + (l >> 4)][16 w + (l & 15)]
//   B: lane l holds B[k = l >> 4][j = l & 15]  = xb[4 kk + (l >> 4)][16 t + (l & 15)]
//   D: register g of lane l is D[row = (l >> 4) + 4 g][col = l & 15]      (the f64 map, not the f32 one)
// so D[i][j] = sum over the rows of x[.][64 I + 16 w + i] * x[.][64 J + 16 t + j].  The partial panel is written whole
// ([64][64] f64 per (run, pair)); cov_reduce keeps its i <= j half.
constexpr uint32_t kCovPitch = kPcaPanel + 4;
static_assert(kPcaPanel == 64 && kPcaCovStage == 32, "pca_cov_kernel's thread map is written for 64-column panels, 32-row stages");

__global__ __launch_bounds__(256) void pca_cov_kernel(const float *__restrict__ rows, const uint32_t *__restrict__ sel, uint64_t ns,
                                                      uint32_t dim, uint32_t stride, const double *__restrict__ mean64,
                                                      uint64_t per, uint32_t npanels, double *__restrict__ partial) {
    __shared__ double xa[kPcaCovStage][kCovPitch];
    __shared__ double xb[kPcaCovStage][kCovPitch];
    // pair index -> (I, J), I <= J, row-major over the upper triangle
    uint32_t I = 0, rem = blockIdx.x;
    while (rem >= npanels - I) {
        rem -= npanels - I;
        ++I;
    }
    const uint32_t J = I + rem;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint64_t t0 = (uint64_t)blockIdx.y * per, t1 = std::min<uint64_t>(ns, t0 + per);
    const uint32_t sc = tid & 63u, sr = tid >> 6;   // staging: column sc of rows sr + 4 u
    const uint32_t ca = I * kPcaPanel + sc, cb = J * kPcaPanel + sc;
    const double ma = ca < dim ? mean64[ca] : 0.0, mb = cb < dim ? mean64[cb] : 0.0;
    f64x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (uint64_t s0 = t0; s0 < t1; s0 += kPcaCovStage) {
#pragma unroll
        for (uint32_t u = 0; u < kPcaCovStage / 4; ++u) {
            const uint32_t r = sr + 4u * u;
            double a = 0.0, b = 0.0;
            if (s0 + r < t1) {
                const uint64_t src = sel ? sel[s0 + r] : s0 + r;
                const float *x = rows + src * stride;
                if (ca < dim) a = (double)x[ca] - ma;
                if (cb < dim) b = (double)x[cb] - mb;
            }
            xa[r][sc] = a;
            xb[r][sc] = b;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t kk = 0; kk < kPcaCovStage / 4; ++kk) {
            const uint32_t r = 4u * kk + (lane >> 4);
            const double a = xa[r][16u * w + (lane & 15u)];
#pragma unroll
            for (uint32_t t = 0; t < 4; ++t) {
                const double b = xb[r][16u * t + (lane & 15u)];
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    double *out = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (kPcaPanel * kPcaPanel);
#pragma unroll
    for (uint32_t t = 0; t < 4; ++t)
#pragma unroll
        for (uint32_t g = 0; g < 4; ++g)
            out[(size_t)(16u * w + (lane >> 4) + 4u * g) * kPcaPanel + 16u * t + (lane & 15u)] = acc[t][g];
}

// C[i][j] = C[j][i] = (sum over the runs, ascending) / denom for i <= j; C is [m][m], zero outside [dim][dim]
__global__ __launch_bounds__(256) void pca_cov_reduce_kernel(const double *__restrict__ partial, uint32_t nruns, uint32_t npairs,
                                                             uint32_t npanels, uint32_t dim, uint32_t m, double denom,
                                                             double *__restrict__ C) {
    uint32_t I = 0, rem = blockIdx.x;
    while (rem >= npanels - I) {
        rem -= npanels - I;
        ++I;
    }
    const uint32_t J = I + rem;
    for (uint32_t e = threadIdx.x; e < kPcaPanel * kPcaPanel; e += 256) {
        const uint32_t i = I * kPcaPanel + e / kPcaPanel, j = J * kPcaPanel + e % kPcaPanel;
        if (i >= dim || j >= dim || i > j) continue;
        double s = 0.0;
        for (uint32_t r = 0; r < nruns; ++r) s = s + partial[((size_t)r * npairs + blockIdx.x) * (kPcaPanel * kPcaPanel) + e];
        const double v = s / denom;
        C[(size_t)i * m + j] = v;
        C[(size_t)j * m + i] = v;
    }
}

// ---- 4 eigen-solve -------------------------------------------------------------------------------------------------
// Round `round` (0 .. m - 2) of the circle method over m players (m even): pair 0 is (round, m - 1), pair k >= 1 is
// ((round + k) mod (m - 1), (round - k) mod (m - 1)); p < q.
__device__ __forceinline__ void jacobi_pair(uint32_t k, uint32_t round, uint32_t m, uint32_t *p, uint32_t *q) {
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

// The rotation that annihilates a_pq (Rutishauser): t = sgn(tau) / (|tau| + sqrt(1 + tau^2)), tau = (a_qq - a_pp) /
// (2 a_pq); c = 1 / sqrt(1 + t^2), s = t c; a_pq == 0: the identity.
__device__ __forceinline__ void jacobi_rotation(const double *__restrict__ A, uint32_t m, uint32_t p, uint32_t q, double *c,
                                                double *s, double *t) {
    const double apq = A[(size_t)p * m + q];
    if (apq == 0.0) {
        *c = 1.0;
        *s = 0.0;
        *t = 0.0;
        return;
    }
    const double tau = (A[(size_t)q * m + q] - A[(size_t)p * m + p]) / (2.0 * apq);
    const double tt = copysign(1.0, tau) / (fabs(tau) + sqrt(1.0 + tau * tau));
    const double cc = 1.0 / sqrt(1.0 + tt * tt);
    *c = cc;
    *s = tt * cc;
    *t = tt;
}

// One round: Aout = J^T Ain J, Vt = J^T Vt (rows of Vt are the eigenvectors), J the product of the round's m / 2 disjoint
// rotations.  Thread (k1 = blockIdx.y, k2) owns the 2 x 2 block of rows (p1, q1) x columns (p2, q2), which depends on that
// block of Ain alone; it computes the block for k1 <= k2 and writes it and its mirror, so Aout is exactly symmetric.  The
// diagonal block takes a_pp - t a_pq, a_qq + t a_pq and an exact zero.  The same thread rotates columns 2 k2, 2 k2 + 1
// of Vt's rows p1, q1 in place.
__global__ __launch_bounds__(128) void pca_jacobi_round_kernel(const double *__restrict__ Ain, double *__restrict__ Aout,
                                                               double *__restrict__ Vt, uint32_t m, uint32_t round) {
    const uint32_t k1 = blockIdx.y, k2 = blockIdx.x * 128 + threadIdx.x;
    if (k2 >= m / 2) return;
    uint32_t p1, q1, p2, q2;
    jacobi_pair(k1, round, m, &p1, &q1);
    jacobi_pair(k2, round, m, &p2, &q2);
    double c1, s1, t1;
    jacobi_rotation(Ain, m, p1, q1, &c1, &s1, &t1);
#pragma unroll
    for (uint32_t e = 0; e < 2; ++e) {
        const size_t col = 2u * k2 + e;
        const double vp = Vt[(size_t)p1 * m + col], vq = Vt[(size_t)q1 * m + col];
        Vt[(size_t)p1 * m + col] = c1 * vp - s1 * vq;
        Vt[(size_t)q1 * m + col] = s1 * vp + c1 * vq;
    }
    if (k1 > k2) return;
    if (k1 == k2) {
        const double app = Ain[(size_t)p1 * m + p1], aqq = Ain[(size_t)q1 * m + q1], apq = Ain[(size_t)p1 * m + q1];
        Aout[(size_t)p1 * m + p1] = app - t1 * apq;
        Aout[(size_t)q1 * m + q1] = aqq + t1 * apq;
        Aout[(size_t)p1 * m + q1] = 0.0;
        Aout[(size_t)q1 * m + p1] = 0.0;
        return;
    }
    double c2, s2, t2;
    jacobi_rotation(Ain, m, p2, q2, &c2, &s2, &t2);
    const double b00 = Ain[(size_t)p1 * m + p2], b01 = Ain[(size_t)p1 * m + q2];
    const double b10 = Ain[(size_t)q1 * m + p2], b11 = Ain[(size_t)q1 * m + q2];
    const double r00 = c1 * b00 - s1 * b10, r01 = c1 * b01 - s1 * b11;   // J^T B
    const double r10 = s1 * b00 + c1 * b10, r11 = s1 * b01 + c1 * b11;
    const double o00 = c2 * r00 - s2 * r01, o01 = s2 * r00 + c2 * r01;   // (J^T B) J
    const double o10 = c2 * r10 - s2 * r11, o11 = s2 * r10 + c2 * r11;
    Aout[(size_t)p1 * m + p2] = o00;
    Aout[(size_t)p2 * m + p1] = o00;
    Aout[(size_t)p1 * m + q2] = o01;
    Aout[(size_t)q2 * m + p1] = o01;
    Aout[(size_t)q1 * m + p2] = o10;
    Aout[(size_t)p2 * m + q1] = o10;
    Aout[(size_t)q1 * m + q2] = o11;
    Aout[(size_t)q2 * m + q1] = o11;
}

// sum of squares in a fixed order: a thread's strided elements ascending, then a halving tree over the 256 threads
__device__ __forceinline__ double block_sum_256(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

// rowsum[i] = sum over j (j > i when strict) of A[i][j]^2
__global__ __launch_bounds__(256) void pca_sumsq_rows_kernel(const double *__restrict__ A, uint32_t m, int strict,
                                                             double *__restrict__ rowsum) {
    __shared__ double red[256];
    const uint32_t i = blockIdx.x;
    double s = 0.0;
    for (uint32_t j = threadIdx.x; j < m; j += 256)
        if (!strict || j > i) {
            const double a = A[(size_t)i * m + j];
            s = s + a * a;
        }
    const double tot = block_sum_256(s, red);
    if (threadIdx.x == 0) rowsum[i] = tot;
}

__global__ __launch_bounds__(256) void pca_sumsq_final_kernel(const double *__restrict__ rowsum, uint32_t m, double *__restrict__ out) {
    __shared__ double red[256];
    double s = 0.0;
    for (uint32_t i = threadIdx.x; i < m; i += 256) s = s + rowsum[i];
    const double tot = block_sum_256(s, red);
    if (threadIdx.x == 0) *out = tot;
}

__global__ __launch_bounds__(256) void pca_identity_kernel(double *__restrict__ Vt, uint32_t m) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < m) Vt[(size_t)i * m + i] = 1.0;
}

// ---- 5 components --------------------------------------------------------------------------------------------------
// order[rank] = column, rank = eigenvalues above it + equal ones of a lower column; eig[rank] = its eigenvalue.  `order`
// and `eig` are zeroed by the caller: with NaN eigenvalues some ranks collide and the rest stay 0 (in range).
__global__ __launch_bounds__(256) void pca_rank_kernel(const double *__restrict__ A, uint32_t m, uint32_t dim,
                                                       uint32_t *__restrict__ order, double *__restrict__ eig) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= dim) return;
    const double li = A[(size_t)i * m + i];
    uint32_t rank = 0;
    for (uint32_t j = 0; j < dim; ++j) {
        const double lj = A[(size_t)j * m + j];
        rank += (lj > li || (lj == li && j < i)) ? 1u : 0u;
    }
    order[rank] = i;
    eig[rank] = li;
}

// component j (blockIdx.x) = row order[j] of Vt, its sign such that the largest-magnitude entry (lowest index on ties)
// is positive, cast to f32
__global__ __launch_bounds__(256) void pca_components_kernel(const double *__restrict__ Vt, uint32_t m, uint32_t dim,
                                                             const uint32_t *__restrict__ order, float *__restrict__ matrix) {
    __shared__ double bmag[256];
    __shared__ uint32_t bidx[256];
    const double *v = Vt + (size_t)order[blockIdx.x] * m;
    double mag = -1.0;
    uint32_t at = 0;
    for (uint32_t i = threadIdx.x; i < dim; i += 256) {
        const double a = fabs(v[i]);
        if (a > mag) {   // ascending i: the first of equal magnitudes stays
            mag = a;
            at = i;
        }
    }
    bmag[threadIdx.x] = mag;
    bidx[threadIdx.x] = at;
    __syncthreads();
    for (uint32_t o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            const double a = bmag[threadIdx.x + o];
            const uint32_t ai = bidx[threadIdx.x + o];
            if (a > bmag[threadIdx.x] || (a == bmag[threadIdx.x] && ai < bidx[threadIdx.x])) {
                bmag[threadIdx.x] = a;
                bidx[threadIdx.x] = ai;
            }
        }
        __syncthreads();
    }
    const double sign = (bmag[0] >= 0.0 && v[bidx[0]] < 0.0) ? -1.0 : 1.0;
    for (uint32_t i = threadIdx.x; i < dim; i += 256) matrix[(size_t)blockIdx.x * dim + i] = (float)(sign * v[i]);
}

// ---- driver --------------------------------------------------------------------------------------------------------
int pca_check(const BfIndexDev &src, uint32_t out_dim) {
    if (src.fmt || !src.rows) return fail(SCANN_HIP_INVALID_ARGUMENT, "pca_train: the index holds quantized rows, not f32 rows");
    if (src.n == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "pca_train: cannot train on an empty dataset");
    if (out_dim == 0 || out_dim > src.dim)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "pca_train: out_dim " + std::to_string(out_dim) + " must be in 1.." + std::to_string(src.dim));
    if (src.dim > kPcaMaxDim)
        return fail(SCANN_HIP_RESOURCE_EXHAUSTED, "pca_train: in_dim " + std::to_string(src.dim) + " is above the limit of " +
                                                      std::to_string(kPcaMaxDim) + " (the Jacobi solve is O(d^3) per sweep)");
    return SCANN_HIP_OK;
}

static thread_local float g_pca_stage_ms[4] = {};

void pca_last_stage_ms(float *out4) { std::memcpy(out4, g_pca_stage_ms, sizeof(g_pca_stage_ms)); }

static float ms_since(std::chrono::steady_clock::time_point &t) {
    const auto now = std::chrono::steady_clock::now();
    const float ms = std::chrono::duration<float, std::milli>(now - t).count();
    t = now;
    return ms;
}

int pca_train_device(scann_hip_ctx *ctx, const BfIndexDev &src, uint32_t out_dim, uint64_t max_samples, uint64_t seed,
                     hipStream_t st, scann_hip_projection **out, double *out_eigenvalues, double *out_covariance,
                     uint32_t *out_sweeps, int *out_converged) {
    SCANN_TRY(pca_check(src, out_dim));
    const uint64_t n = src.n;
    const uint32_t d = src.dim, stride = src.stride, m = (d + 1u) & ~1u;
    const bool sampled = max_samples != 0 && max_samples < n;
    const uint64_t ns = sampled ? max_samples : n;
    float ms[4] = {};
    auto t = std::chrono::steady_clock::now();

    // ---- 1 sample, 2 mean ----
    DevBuf d_sel, d_runs, d_mean64, d_mean32;
    const uint32_t *sel = nullptr;
    if (sampled) {
        SCANN_TRY(d_sel.ensure(ns * 4));
        SCANN_TRY(launch(pca_sample_kernel, dim3((uint32_t)ceil_div_u64(ns, 256)), dim3(256), 0, st, seed ^ 0x9CAull, ns, n,
                         d_sel.as<uint32_t>()));
        sel = d_sel.as<uint32_t>();
    }
    const uint64_t mean_per = ceil_div_u64(ns, kPcaMeanChunks);
    const uint32_t mean_runs = (uint32_t)ceil_div_u64(ns, mean_per);
    SCANN_TRY(d_runs.ensure((size_t)mean_runs * d * 8));
    SCANN_TRY(d_mean64.ensure((size_t)d * 8));
    SCANN_TRY(d_mean32.ensure((size_t)d * 4));
    SCANN_TRY(launch(pca_mean_runs_kernel, dim3(ceil_div_u32(d, 256), mean_runs), dim3(256), 0, st, src.rows, sel, ns, d, stride,
                     mean_per, d_runs.as<double>()));
    SCANN_TRY(launch(pca_mean_final_kernel, dim3(ceil_div_u32(d, 256)), dim3(256), 0, st, (const double *)d_runs.as<double>(),
                     mean_runs, d, ns, d_mean64.as<double>(), d_mean32.as<float>()));
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    d_runs.release();
    ms[0] = ms_since(t);

    // ---- 3 covariance ----
    const uint32_t npanels = ceil_div_u32(d, kPcaPanel), npairs = npanels * (npanels + 1) / 2;
    const size_t panel_bytes = (size_t)kPcaPanel * kPcaPanel * 8;
    uint64_t cov_runs = std::min<uint64_t>(kPcaCovMaxRuns, ceil_div_u64(ns, kPcaCovMinRun));
    cov_runs = std::max<uint64_t>(1, std::min<uint64_t>(cov_runs, kPcaCovWorkspaceBytes / (npairs * panel_bytes)));
    const uint64_t cov_per = ceil_div_u64(ceil_div_u64(ns, cov_runs), kPcaCovStage) * kPcaCovStage;
    cov_runs = ceil_div_u64(ns, cov_per);
    DevBuf d_partial, d_a0, d_a1, d_vt;
    SCANN_TRY(d_partial.ensure((size_t)cov_runs * npairs * panel_bytes));
    const size_t mm_bytes = (size_t)m * m * 8;
    SCANN_TRY(d_a0.ensure(mm_bytes));
    SCANN_HIP_CHECK(hipMemsetAsync(d_a0.p, 0, mm_bytes, st));
    SCANN_TRY(launch(pca_cov_kernel, dim3(npairs, (uint32_t)cov_runs), dim3(256), 0, st, src.rows, sel, ns, d, stride,
                     (const double *)d_mean64.as<double>(), cov_per, npanels, d_partial.as<double>()));
    SCANN_TRY(launch(pca_cov_reduce_kernel, dim3(npairs), dim3(256), 0, st, (const double *)d_partial.as<double>(),
                     (uint32_t)cov_runs, npairs, npanels, d, m, (double)std::max<uint64_t>(1, ns - 1), d_a0.as<double>()));
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    d_partial.release();
    d_sel.release();
    if (out_covariance)
        SCANN_HIP_CHECK(hipMemcpy2D(out_covariance, (size_t)d * 8, d_a0.p, (size_t)m * 8, (size_t)d * 8, d, hipMemcpyDeviceToHost));
    ms[1] = ms_since(t);

    // ---- 4 eigen-solve ----
    DevBuf d_rowsum, d_norm;
    SCANN_TRY(d_a1.ensure(mm_bytes));
    SCANN_TRY(d_vt.ensure(mm_bytes));
    SCANN_TRY(d_rowsum.ensure((size_t)m * 8));
    SCANN_TRY(d_norm.ensure(8));
    SCANN_HIP_CHECK(hipMemsetAsync(d_a1.p, 0, mm_bytes, st));
    SCANN_HIP_CHECK(hipMemsetAsync(d_vt.p, 0, mm_bytes, st));
    SCANN_TRY(launch(pca_identity_kernel, dim3(ceil_div_u32(m, 256)), dim3(256), 0, st, d_vt.as<double>(), m));
    double *cur = d_a0.as<double>(), *nxt = d_a1.as<double>();
    auto sumsq = [&](const double *A, int strict, double *host) -> int {
        SCANN_TRY(launch(pca_sumsq_rows_kernel, dim3(m), dim3(256), 0, st, A, m, strict, d_rowsum.as<double>()));
        SCANN_TRY(launch(pca_sumsq_final_kernel, dim3(1), dim3(256), 0, st, (const double *)d_rowsum.as<double>(), m,
                         d_norm.as<double>()));
        SCANN_HIP_CHECK(hipMemcpyAsync(host, d_norm.p, 8, hipMemcpyDeviceToHost, st));
        SCANN_HIP_CHECK(hipStreamSynchronize(st));
        return SCANN_HIP_OK;
    };
    double all2 = 0.0, off2 = 0.0;
    SCANN_TRY(sumsq(cur, 0, &all2));
    SCANN_TRY(sumsq(cur, 1, &off2));
    const double tol = std::ldexp(std::sqrt(all2), -46);   // 2^-46 ||C||_F
    auto done = [&] { return std::sqrt(2.0 * off2) <= tol; };
    uint32_t sweeps = 0;
    int converged = done() ? 1 : 0;
    while (!converged && sweeps < kPcaMaxSweeps) {
        for (uint32_t round = 0; round + 1 < m; ++round) {
            SCANN_TRY(launch(pca_jacobi_round_kernel, dim3(ceil_div_u32(m / 2, 128), m / 2), dim3(128), 0, st, (const double *)cur,
                             nxt, d_vt.as<double>(), m, round));
            std::swap(cur, nxt);
        }
        ++sweeps;
        SCANN_TRY(sumsq(cur, 1, &off2));
        converged = done() ? 1 : 0;
    }
    ms[2] = ms_since(t);

    // ---- 5 components ----
    DevBuf d_order, d_eig, d_matrix;
    SCANN_TRY(d_order.ensure((size_t)d * 4));
    SCANN_TRY(d_eig.ensure((size_t)d * 8));
    SCANN_TRY(d_matrix.ensure((size_t)out_dim * d * 4));
    SCANN_HIP_CHECK(hipMemsetAsync(d_order.p, 0, (size_t)d * 4, st));
    SCANN_HIP_CHECK(hipMemsetAsync(d_eig.p, 0, (size_t)d * 8, st));
    SCANN_TRY(launch(pca_rank_kernel, dim3(ceil_div_u32(d, 256)), dim3(256), 0, st, (const double *)cur, m, d,
                     d_order.as<uint32_t>(), d_eig.as<double>()));
    SCANN_TRY(launch(pca_components_kernel, dim3(out_dim), dim3(256), 0, st, (const double *)d_vt.as<double>(), m, d,
                     (const uint32_t *)d_order.as<uint32_t>(), d_matrix.as<float>()));
    std::vector<float> matrix((size_t)out_dim * d), mean(d);
    SCANN_HIP_CHECK(hipMemcpyAsync(matrix.data(), d_matrix.p, matrix.size() * 4, hipMemcpyDeviceToHost, st));
    SCANN_HIP_CHECK(hipMemcpyAsync(mean.data(), d_mean32.p, mean.size() * 4, hipMemcpyDeviceToHost, st));
    if (out_eigenvalues) SCANN_HIP_CHECK(hipMemcpyAsync(out_eigenvalues, d_eig.p, (size_t)d * 8, hipMemcpyDeviceToHost, st));
    SCANN_HIP_CHECK(hipStreamSynchronize(st));
    SCANN_TRY(scann_hip_projection_create(ctx, SCANN_HIP_PROJ_PCA, d, out_dim, matrix.data(), mean.data(), 0, out));
    ms[3] = ms_since(t);
    if (out_sweeps) *out_sweeps = sweeps;
    if (out_converged) *out_converged = converged;
    std::memcpy(g_pca_stage_ms, ms, sizeof(ms));
    return SCANN_HIP_OK;
}

}  // namespace scann

using namespace scann;

extern "C" {

int scann_hip_projection_arrays(const scann_hip_projection *p, float *out_matrix, float *out_mean) {
    if (!p) return fail(SCANN_HIP_INVALID_ARGUMENT, "projection is null");
    if (out_matrix && !p->matrix.empty()) std::memcpy(out_matrix, p->matrix.data(), p->matrix.size() * 4);
    if (out_mean && !p->mean.empty()) std::memcpy(out_mean, p->mean.data(), p->mean.size() * 4);
    return SCANN_HIP_OK;
}

void scann_hip_pca_last_stage_ms(float *out4) {
    if (out4) pca_last_stage_ms(out4);
}

}  // extern "C"

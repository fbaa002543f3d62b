// project.hip -- dense projections on the device (project.h): project_kernel, the window copy of
// TruncateProjection, and the entry points scann_hip_projection_create / _destroy / _info, scann_hip_project and
// scann_hip_project_device.  (The handles that search through a projection are in api.hip.)
#include "project.h"

#include <algorithm>

#include "comm.h"   // ctx_device
#include "launch.h"

namespace scann {

// A register-tiled sequential-k GEMM.  Workgroup (bx, by) owns rows [64 bx, 64 bx + 64) x outputs [64 by, 64 by + 64);
// thread (ty, tx) = (tid / 16, tid % 16) owns rows 4 ty .. 4 ty + 3 x outputs 4 tx .. 4 tx + 3 of them.  The i range is
// walked in ascending chunks of 32: the chunk of the 64 rows (centred once, here, for PCA) and of the 64 matrix rows is
// staged in LDS transposed ([i][row], [i][output], pitch 68 floats so that a thread's four values are one 16-byte
// read), then every thread walks the chunk's elements in ascending i: acc = acc + x * m, a multiply and an add
// (the library is compiled with -ffp-contract=off).  Every output's chain is therefore the reference's own: no FMA, no
// split of the i range, no tree.  LDS: 2 x 32 x 68 x 4 = 17 408 bytes, whatever in_dim is.  Rows past n and outputs
// past out_dim are neither read nor written (their LDS slots hold zeros, their accumulators are dropped).
constexpr uint32_t kProjPitch = kProjRows + 4;
static_assert(kProjRows == 64 && kProjOuts == 64 && kProjChunk == 32, "project_kernel's thread map is written for 64 x 64 x 32");

template <bool PCA>
__global__ __launch_bounds__(256) void project_kernel(ProjDev p, const float *__restrict__ rows, uint64_t n,
                                                      uint32_t row_stride, float *__restrict__ out, uint32_t out_stride) {
    __shared__ __attribute__((aligned(16))) float xs[kProjChunk][kProjPitch];
    __shared__ __attribute__((aligned(16))) float ms[kProjChunk][kProjPitch];
    const uint32_t tid = threadIdx.x, tx = tid & 15u, ty = tid >> 4;
    const uint64_t r0 = (uint64_t)blockIdx.x * kProjRows;
    const uint32_t j0 = blockIdx.y * kProjOuts;
    const uint32_t nr = (uint32_t)std::min<uint64_t>(kProjRows, n - r0), nj = std::min(kProjOuts, p.out_dim - j0);
    const uint32_t in_dim = p.in_dim;
    const uint32_t sc = tid & 31u, sr = tid >> 5;   // staging: element (row sr + 8 u, column sc) of the chunk
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0f;
    for (uint32_t i0 = 0; i0 < in_dim; i0 += kProjChunk) {
        const uint32_t kc = std::min(kProjChunk, in_dim - i0);
#pragma unroll
        for (uint32_t u = 0; u < kProjRows / 8; ++u) {
            const uint32_t r = sr + 8u * u;
            float x = 0.0f, m = 0.0f;
            if (sc < kc) {
                if (r < nr) {
                    x = rows[(size_t)(r0 + r) * row_stride + i0 + sc];
                    if (PCA) x = x - p.mean[i0 + sc];
                }
                if (r < nj) m = p.matrix[(size_t)(j0 + r) * in_dim + i0 + sc];
            }
            xs[sc][r] = x;
            ms[sc][r] = m;
        }
        __syncthreads();
#pragma unroll 8
        for (uint32_t k = 0; k < kc; ++k) {
            const float4 xv = *reinterpret_cast<const float4 *>(&xs[k][4u * ty]);
            const float4 mv = *reinterpret_cast<const float4 *>(&ms[k][4u * tx]);
            const float x[4] = {xv.x, xv.y, xv.z, xv.w}, m[4] = {mv.x, mv.y, mv.z, mv.w};
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const float t = x[a] * m[b];
                    acc[a][b] = acc[a][b] + t;
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (uint32_t a = 0; a < 4; ++a) {
        const uint32_t r = 4u * ty + a;
        if (r < nr) {
            float *o = out + (size_t)(r0 + r) * out_stride + j0;
#pragma unroll
            for (uint32_t b = 0; b < 4; ++b)
                if (4u * tx + b < nj) o[4u * tx + b] = acc[a][b];
        }
    }
}

// TruncateProjection (and an untrained PcaProjection): out = in[start .. start + out_dim)
__global__ __launch_bounds__(256) void project_window_kernel(const float *__restrict__ rows, uint64_t n, uint32_t row_stride,
                                                             uint32_t start, uint32_t out_dim, float *__restrict__ out,
                                                             uint32_t out_stride) {
    const uint64_t total = n * out_dim;
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (uint64_t)gridDim.x * 256) {
        const uint64_t r = e / out_dim;
        const uint32_t j = (uint32_t)(e - r * out_dim);
        out[r * out_stride + j] = rows[r * row_stride + start + j];
    }
}

int launch_project(const ProjDev &p, const float *d_rows, uint64_t n, uint32_t row_stride, float *d_out,
                   uint32_t out_stride, hipStream_t st) {
    if (n == 0) return SCANN_HIP_OK;
    if (!d_rows || !d_out) return fail(SCANN_HIP_INVALID_ARGUMENT, "projection: null rows/output");
    if (row_stride < p.in_dim || out_stride < p.out_dim)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "projection: a stride is below its dim");
    if (n > UINT64_MAX / std::max(row_stride, out_stride)) return fail(SCANN_HIP_OUT_OF_RANGE, "projection: n * stride overflows");
    if (p.kind == SCANN_HIP_PROJ_TRUNCATE) {
        const uint32_t grid = (uint32_t)std::min<uint64_t>(ceil_div_u64(n * p.out_dim, 256), (uint64_t)num_cus() * 8);
        return launch(project_window_kernel, dim3(grid), dim3(256), 0, st, d_rows, n, row_stride, p.start, p.out_dim, d_out,
                      out_stride);
    }
    const uint64_t gx = ceil_div_u64(n, kProjRows);
    if (gx > 0x7FFFFFFFull) return fail(SCANN_HIP_OUT_OF_RANGE, "projection: more than 2^31 - 1 row tiles");
    if (ceil_div_u64(p.out_dim, kProjOuts) > 65535u) return fail(SCANN_HIP_OUT_OF_RANGE, "projection: more than 65535 output tiles");
    const dim3 grid((uint32_t)gx, ceil_div_u32(p.out_dim, kProjOuts));
    if (p.kind == SCANN_HIP_PROJ_PCA)
        return launch(project_kernel<true>, grid, dim3(256), 0, st, p, d_rows, n, row_stride, d_out, out_stride);
    if (p.kind == SCANN_HIP_PROJ_MATRIX)
        return launch(project_kernel<false>, grid, dim3(256), 0, st, p, d_rows, n, row_stride, d_out, out_stride);
    return fail(SCANN_HIP_INVALID_ARGUMENT, "projection: unknown kind " + std::to_string(p.kind));
}

int projection_args(int kind, uint32_t in_dim, uint32_t out_dim, const float *matrix, const float *mean, uint32_t start) {
    if (kind != SCANN_HIP_PROJ_MATRIX && kind != SCANN_HIP_PROJ_PCA && kind != SCANN_HIP_PROJ_TRUNCATE)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "projection: unknown kind " + std::to_string(kind));
    if (in_dim == 0 || out_dim == 0) return fail(SCANN_HIP_INVALID_ARGUMENT, "projection: in_dim and out_dim must be > 0");
    if (kind == SCANN_HIP_PROJ_TRUNCATE) {
        if ((uint64_t)start + out_dim > in_dim)
            return fail(SCANN_HIP_INVALID_ARGUMENT, "projection: start + out_dim exceeds in_dim");
        return SCANN_HIP_OK;
    }
    if (!matrix) return fail(SCANN_HIP_INVALID_ARGUMENT, "projection: matrix is null");
    if (kind == SCANN_HIP_PROJ_PCA && !mean) return fail(SCANN_HIP_INVALID_ARGUMENT, "projection: mean is null (PCA)");
    return SCANN_HIP_OK;
}

}  // namespace scann

using namespace scann;

extern "C" {

int scann_hip_projection_create(scann_hip_ctx *ctx, int kind, uint32_t in_dim, uint32_t out_dim, const float *matrix,
                                const float *mean, uint32_t start, scann_hip_projection **out) {
    if (!ctx || !out) return fail(SCANN_HIP_INVALID_ARGUMENT, "null ctx/out_projection");
    SCANN_TRY(projection_args(kind, in_dim, out_dim, matrix, mean, start));
    SCANN_HIP_CHECK(hipSetDevice(ctx_device(ctx)));
    auto *p = new scann_hip_projection();
    p->ctx = ctx;
    p->dev.kind = kind;
    p->dev.in_dim = in_dim;
    p->dev.out_dim = out_dim;
    p->dev.start = kind == SCANN_HIP_PROJ_TRUNCATE ? start : 0u;
    int s = SCANN_HIP_OK;
    if (kind != SCANN_HIP_PROJ_TRUNCATE) {
        p->matrix.assign(matrix, matrix + (size_t)out_dim * in_dim);
        s = upload(p->d_matrix, p->matrix.data(), p->matrix.size() * 4);
        p->dev.matrix = p->d_matrix.as<float>();
    }
    if (s == SCANN_HIP_OK && kind == SCANN_HIP_PROJ_PCA) {
        p->mean.assign(mean, mean + in_dim);
        s = upload(p->d_mean, p->mean.data(), p->mean.size() * 4);
        p->dev.mean = p->d_mean.as<float>();
    }
    if (s != SCANN_HIP_OK) {
        delete p;
        return s;
    }
    *out = p;
    return SCANN_HIP_OK;
}

void scann_hip_projection_destroy(scann_hip_projection *p) { delete p; }

int scann_hip_projection_info(const scann_hip_projection *p, uint32_t *out4) {
    if (!p || !out4) return fail(SCANN_HIP_INVALID_ARGUMENT, "null projection/output");
    out4[0] = (uint32_t)p->dev.kind;
    out4[1] = p->dev.in_dim;
    out4[2] = p->dev.out_dim;
    out4[3] = p->dev.start;
    return SCANN_HIP_OK;
}

int scann_hip_project_device(const scann_hip_projection *p, const float *d_rows, uint64_t n, uint32_t row_stride,
                             float *d_out, uint32_t out_stride, void *hip_stream) {
    if (!p) return fail(SCANN_HIP_INVALID_ARGUMENT, "projection is null");
    SCANN_HIP_CHECK(hipSetDevice(ctx_device(p->ctx)));
    return launch_project(p->dev, d_rows, n, row_stride, d_out, out_stride, static_cast<hipStream_t>(hip_stream));
}

int scann_hip_project(const scann_hip_projection *p, const float *rows, uint64_t n, uint32_t row_stride, uint32_t row_dim,
                      float *out, uint32_t out_stride) {
    if (!p) return fail(SCANN_HIP_INVALID_ARGUMENT, "projection is null");
    if (row_dim != p->dev.in_dim)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "projection: row_dim " + std::to_string(row_dim) + " is not in_dim " +
                                                    std::to_string(p->dev.in_dim));
    if (row_stride < row_dim || out_stride < p->dev.out_dim)
        return fail(SCANN_HIP_INVALID_ARGUMENT, "projection: a stride is below its dim");
    if (n == 0) return SCANN_HIP_OK;
    if (!rows || !out) return fail(SCANN_HIP_INVALID_ARGUMENT, "projection: null rows/output");
    if (n > UINT64_MAX / 4 / std::max(row_stride, out_stride)) return fail(SCANN_HIP_OUT_OF_RANGE, "projection: n * stride overflows");
    SCANN_HIP_CHECK(hipSetDevice(ctx_device(p->ctx)));
    // the last row is dim wide, not stride wide: the caller's arrays may end there
    const size_t in_elems = (size_t)(n - 1) * row_stride + row_dim, out_elems = (size_t)(n - 1) * out_stride + p->dev.out_dim;
    DevBuf d_in, d_out;
    SCANN_TRY(upload(d_in, rows, in_elems * 4));
    SCANN_TRY(d_out.ensure(out_elems * 4));
    SCANN_TRY(launch_project(p->dev, d_in.as<float>(), n, row_stride, d_out.as<float>(), out_stride, nullptr));
    // only the out_dim columns come back: the caller's elements between out_dim and out_stride stay as they are
    SCANN_HIP_CHECK(hipMemcpy2D(out, (size_t)out_stride * 4, d_out.p, (size_t)out_stride * 4, (size_t)p->dev.out_dim * 4, n,
                                hipMemcpyDeviceToHost));
    return SCANN_HIP_OK;
}

}  // extern "C"

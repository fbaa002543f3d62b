// project.h -- the reference's dense projections on the device: PcaProjection, RandomOrthogonalProjection,
// GaussianRandomProjection and OpqProjection are one loop (pca.rs:156-180, random.rs:82-92, 157-167, opq.rs:179-194),
//     out[j] = 0.0f;  for i in 0..in_dim (ascending):  out[j] += (in[i] - mean[i]) * M[(i, j)]
// an f32 sum whose every step is a multiply and then an add (Rust never contracts), the subtraction PCA's alone;
// TruncateProjection and an untrained PcaProjection are a window copy.  project_kernel keeps exactly that chain per
// output, so a projected row is the reference's bit for bit.
#pragma once
#include <vector>

#include "common.h"

namespace scann {

// A projection on the device.  matrix: [out_dim][in_dim] (row j = column j of the reference's column-major DMatrix),
// nullptr for TRUNCATE; mean: [in_dim], PCA only.
struct ProjDev {
    int kind = 0;   // SCANN_HIP_PROJ_*; 0 = none
    uint32_t in_dim = 0, out_dim = 0, start = 0;
    const float *matrix = nullptr;
    const float *mean = nullptr;
};

// the tile of project_kernel: a workgroup of 256 threads owns kProjRows rows x kProjOuts outputs (4 x 4 per thread) and
// walks the i range in chunks of kProjChunk staged in LDS
constexpr uint32_t kProjRows = 64, kProjOuts = 64, kProjChunk = 32;

// n rows of p.in_dim floats at row_stride -> n rows of p.out_dim floats at out_stride; enqueue only, no allocation.
// Elements of `out` past out_dim are not written.
int launch_project(const ProjDev &p, const float *d_rows, uint64_t n, uint32_t row_stride, float *d_out,
                   uint32_t out_stride, hipStream_t st);

// kind / dims / pointers of a create call (InvalidArgument on a bad one)
int projection_args(int kind, uint32_t in_dim, uint32_t out_dim, const float *matrix, const float *mean, uint32_t start);

}  // namespace scann

// The opaque type of the C ABI: immutable after create.  The host copies serve handles that copy the projection
// (scann_hip_txh_create_projected) and the index-file writer.
struct scann_hip_projection {
    scann_hip_ctx *ctx = nullptr;
    scann::ProjDev dev;
    std::vector<float> matrix, mean;
    scann::DevBuf d_matrix, d_mean;
};

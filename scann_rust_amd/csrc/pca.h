// pca.h -- scann_hip_pca_train (scann_hip.h "PCA training on the device"): PcaProjection::train
// (projection/pca.rs:71-129, utils/linear_algebra.rs:89-120) from the resident rows of an f32 brute-force handle.  The
// rule is the project's own, the one trainer.pca_projection states (the reference's shuffle and nalgebra SVD are not
// reproducible: SURVEY F2, F4, F10):
//   1 sample      max_samples == 0 or >= n: every row in order; else ns = max_samples rows, row t =
//                 splitmix64(seed ^ 0x9CA, 0, ns)[t] % n (with replacement, counter based), computed on the device.
//   2 mean        per column in f64: the ns rows are cut into at most kPcaMeanChunks runs of consecutive sample
//                 positions, every run is summed in ascending order by one thread, the runs are added in ascending order
//                 by one thread.  No floating-point atomics; the order depends on ns alone.  mean_f32 is its rounding.
//   3 covariance  C = sum (x - mean64)(x - mean64)^T / max(1, ns - 1): rows widened to f64 and centred with the UNROUNDED
//                 mean before the product, two passes, never E[xx^T] - mu mu^T.  Computed on v_mfma_f64_16x16x4_f64 in
//                 panels of kPcaPanel columns, upper-triangle panel pairs only, split over row runs into a bounded
//                 workspace and reduced in ascending run order; the lower triangle is the mirror of the upper.
//                 Elements between dim and stride are never read.
//   4 eigen-solve cyclic Jacobi on C in f64: a fixed round-robin pairing (m - 1 rounds of m / 2 disjoint rotations, m =
//                 dim rounded up to even; the odd dim's bye is a rotation against a zero row), one kernel per round, so
//                 the result is a function of C alone.  Converged when the Frobenius norm of the strict off-diagonal,
//                 summed from the off-diagonal entries themselves, is <= 2^-46 ||C||_F; at most kPcaMaxSweeps sweeps.
//   5 components  eigenvalues descending (ties: lower column first); each component's sign makes its largest-magnitude
//                 entry positive (ties: lowest index); cast to f32; matrix [out_dim][in_dim].
// Device memory while training (all released on return), d = in_dim, m = d rounded up to even:
//   ns * 4 (sample indices, only when sampling) + kPcaMeanChunks * d * 8 (mean runs) + at most kPcaCovWorkspaceBytes
//   (covariance runs) + 3 * m * m * 8 (two copies of the rotated matrix, the eigenvectors) + O(d) words.
#pragma once
#include "bf.h"
#include "common.h"

namespace scann {

constexpr uint32_t kPcaMaxDim = 2048;          // Jacobi is O(d^3) per sweep; DESIGN.md 7
constexpr uint32_t kPcaMaxSweeps = 30;
constexpr uint32_t kPcaMeanChunks = 1024;      // runs of the mean's first pass
constexpr uint32_t kPcaPanel = 64;             // columns of one covariance panel (4 x 4 MFMA tiles per panel pair)
constexpr uint32_t kPcaCovStage = 32;          // rows staged in LDS per step of the covariance kernel
constexpr uint32_t kPcaCovMinRun = 1024;       // fewest rows worth a covariance run of their own
constexpr uint32_t kPcaCovMaxRuns = 256;
constexpr size_t kPcaCovWorkspaceBytes = (size_t)128 << 20;   // ceiling of the covariance runs' partial panels

// Every refusal of scann_hip_pca_train that depends on the rows' shape; launches nothing.
int pca_check(const BfIndexDev &src, uint32_t out_dim);
// Trains on `stream` (complete on return) and creates the projection object as scann_hip_projection_create does from
// the matrix and mean read back.  out_eigenvalues [dim], out_covariance [dim][dim], out_sweeps, out_converged: optional.
int pca_train_device(scann_hip_ctx *ctx, const BfIndexDev &src, uint32_t out_dim, uint64_t max_samples, uint64_t seed,
                     hipStream_t stream, scann_hip_projection **out, double *out_eigenvalues, double *out_covariance,
                     uint32_t *out_sweeps, int *out_converged);
// host-clock milliseconds of the calling thread's last pca_train_device: sample + mean, covariance, eigen-solve,
// components + read-back (tools/time_pca_build.py)
void pca_last_stage_ms(float *out4);

}  // namespace scann

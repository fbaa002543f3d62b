// opq.h -- scann_hip_opq_train (scann_hip.h "OPQ training on the device"): the non-parametric
// alternation of Ge et al. that OpqProjection::train_on_vecs (projection/opq.rs:91-157) calls "full OPQ", from the
// resident rows of an f32 brute-force handle.  The rule is the project's own, the one trainer.opq_rotation states:
//   1 sample      scann_hip_pca_train's step 1 with salt seed ^ 0x0B9; the sampled rows are gathered once into a device
//                 buffer X [ns][d] (max_samples == 0: the handle's rows in place).
//   2 for t = 0 .. T - 1
//     a project   Y = X R_t by project_kernel (f32, sequential, no FMA): the rows a projected build will see.
//     b codebook  t == 0: step 3 of scann_hip_txh_build on Y (flat, seed + s, training_iterations Lloyd steps);
//                 t >= 1: no seeding, inner_iterations Lloyd steps from the previous codebook (build.h, warm).
//     c encode    scann_hip_encode's rule on Y; distortion[t] = ||Y - decode(codes)||_F^2 / ns in f64, fixed order.
//     d cross     M = X^T Yhat in f64 (X widened, no centring), Yhat decoded from the codes while staging:
//                 opq_cross_kernel on v_mfma_f64_16x16x4_f64, every panel pair, row runs reduced in ascending order.
//     e polar     M = U S V^T by one-sided (Hestenes) Jacobi in f64, R_{t+1} = U V^T cast to f32.  sigma_min <=
//                 2^-40 sigma_max: M is singular, training stops and R_t is returned.
//   3 R_T, stored as a SCANN_HIP_PROJ_MATRIX projection [out][in] = R^T.
// Device memory while training (released on return): ns * d * 4 (X, only when sampling) + ns * d * 4 (Y) + ns * S (codes)
// + ns * 8 (row errors) + the codebook trainer's buffers + at most kOpqCrossWorkspaceBytes (cross-covariance runs)
// + 2 * d * d * 8 (M^T, V^T) + 2 * d * d * 4 (R_t^T, R_{t+1}^T) + O(d) words.
#pragma once
#include "bf.h"
#include "common.h"

namespace scann {

constexpr uint32_t kOpqMaxDim = 2048;          // a row pair of the Hestenes round is 8 doubles per lane at 256 lanes
constexpr uint32_t kOpqMaxIterations = 64;     // the report's arrays
constexpr uint32_t kOpqMaxSweeps = 30;
constexpr uint32_t kOpqPanel = 64;             // columns of one panel (4 x 4 MFMA tiles per panel pair)
constexpr uint32_t kOpqStage = 32;             // rows staged in LDS per step
constexpr uint32_t kOpqMinRun = 1024;          // fewest rows worth a run of their own
constexpr uint32_t kOpqMaxRuns = 256;
constexpr size_t kOpqCrossWorkspaceBytes = (size_t)128 << 20;   // ceiling of the runs' partial panels
constexpr int kOpqSingularExp = -40;           // sigma_min <= 2^-40 sigma_max: singular (the solve converges to ~2^-46)

// Every refusal of scann_hip_opq_train; launches nothing.
int opq_check(const BfIndexDev &src, const scann_hip_opq_config &cfg, const scann_hip_projection *init);

// M = X^T Yhat, X the n rows of d floats at `stride` on the device, Yhat[r][j] = codebook[s][code[r][s]][j - s dsub]
// (d_codebook [S][K][dsub]; d_codes [n][S] bytes, or [n][ceil(S / 2)] with subspace s in nibble s & 1 of byte s >> 1).
// d_out [d][d] f64 on the device: M[i][j] at i * d + j, or at j * d + i when transposed.  Enqueue only; d_partial is
// the caller's workspace (grown as needed).
int opq_cross_device(const float *d_rows, uint64_t n, uint32_t d, uint32_t stride, const float *d_codebook, uint32_t S,
                     uint32_t K, uint32_t dsub, const uint8_t *d_codes, int packed4, double *d_out, bool transposed,
                     DevBuf &d_partial, hipStream_t stream);

// Polar factor of the M whose transpose d_mt [d][d] holds (destroyed): d_r [d][d] f32 = U V^T, R[i][j] at i * d + j, or
// at j * d + i when transposed (the projection's [out][in]).  sigma [d] (host, unsorted: column order) is always
// written; d_r only when assemble.  Complete on return.
int opq_polar_device(double *d_mt, uint32_t d, float *d_r, bool transposed, bool assemble_singular, double *sigma,
                     uint32_t *out_sweeps, int *out_converged, double *out_min_over_max, int *out_singular,
                     hipStream_t stream);

int opq_train_device(scann_hip_ctx *ctx, const BfIndexDev &src, const scann_hip_opq_config &cfg,
                     const scann_hip_projection *init, hipStream_t stream, scann_hip_projection **out,
                     scann_hip_opq_report *rep);

}  // namespace scann

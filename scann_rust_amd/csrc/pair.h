// pair.h -- exact distance of one pair of f32 rows by one thread, in the reference's own arithmetic: shared by the
// exact scans and finishes of txh.hip and by the MMR stage of mmr.hip (similarity of two stored rows).
#pragma once
#include "common.h"

namespace scann {

// Exact distance of one (query, row) pair by ONE thread: the 8 AVX2 lane chains in registers, combined as
// the reference combines them (exact_pair_8lanes spreads the same chains over 8 lanes).  DistanceMeasure::
// distance (distance_measures/mod.rs:70-81) = the one-to-many kernels' per-row arithmetic (simd/x86.rs).
__device__ __forceinline__ float exact_pair_thread(int measure, uint32_t dim, const float *sq, const float *row) {
    const uint32_t chunks = dim >> 3;
    float ac[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, aa[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f},
          bb[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    // rows are 16-byte aligned when their stride is a multiple of 4 floats (compute_stride: always): 16-byte
    // loads, four 8-dim chunks (eight loads) in flight -- a 4-byte load per element costs the L1 as many line
    // requests as a 16-byte one
    const bool vec = (reinterpret_cast<uintptr_t>(row) & 15u) == 0;
    for (uint32_t c0 = 0; c0 < chunks; c0 += 4) {
        float xs[4][8];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (c0 + u < chunks) {
                if (vec) {
                    const float4 lo4 = *reinterpret_cast<const float4 *>(row + 8 * (c0 + u));
                    const float4 hi4 = *reinterpret_cast<const float4 *>(row + 8 * (c0 + u) + 4);
                    xs[u][0] = lo4.x; xs[u][1] = lo4.y; xs[u][2] = lo4.z; xs[u][3] = lo4.w;
                    xs[u][4] = hi4.x; xs[u][5] = hi4.y; xs[u][6] = hi4.z; xs[u][7] = hi4.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) xs[u][j] = row[8 * (c0 + u) + j];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
        if (c0 + u >= chunks) break;
        const uint32_t c = c0 + u;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float qv = sq[8 * c + j], x = xs[u][j];
            if (measure == SCANN_HIP_DOT_PRODUCT) {
                ac[j] = fmaf(qv, x, ac[j]);
            } else if (measure == SCANN_HIP_L1) {
                ac[j] = ac[j] + fabsf(qv - x);
            } else if (measure == SCANN_HIP_COSINE) {
                ac[j] = ac[j] + qv * x;
                aa[j] = aa[j] + qv * qv;
                bb[j] = bb[j] + x * x;
            } else {
                const float d = qv - x;
                ac[j] = fmaf(d, d, ac[j]);
            }
        }
        }
    }
    float r, saa = 0.0f, sbb = 0.0f;
    if (measure == SCANN_HIP_COSINE) {   // wide 0.7 reduce_add, non-AVX build
        r = (((ac[0] + ac[1]) + ac[2]) + ac[3]) + (((ac[4] + ac[5]) + ac[6]) + ac[7]);
        saa = (((aa[0] + aa[1]) + aa[2]) + aa[3]) + (((aa[4] + aa[5]) + aa[6]) + aa[7]);
        sbb = (((bb[0] + bb[1]) + bb[2]) + bb[3]) + (((bb[4] + bb[5]) + bb[6]) + bb[7]);
    } else {                             // horizontal_sum_f32_avx2
        r = ((ac[0] + ac[4]) + (ac[1] + ac[5])) + ((ac[2] + ac[6]) + (ac[3] + ac[7]));
    }
    for (uint32_t j = chunks * 8; j < dim; ++j) {   // scalar tail, not fused
        const float qv = sq[j], x = row[j];
        if (measure == SCANN_HIP_DOT_PRODUCT) {
            r = r + qv * x;
        } else if (measure == SCANN_HIP_L1) {
            r = r + fabsf(qv - x);
        } else if (measure == SCANN_HIP_COSINE) {
            r = r + qv * x;
            saa = saa + qv * qv;
            sbb = sbb + x * x;
        } else {
            const float d = qv - x;
            r = r + d * d;
        }
    }
    if (measure == SCANN_HIP_DOT_PRODUCT) r = -r;
    if (measure == SCANN_HIP_L2) r = sqrtf(r);
    if (measure == SCANN_HIP_COSINE) {
        const float na = sqrtf(saa), nb = sqrtf(sbb);
        r = 1.0f - ((na == 0.0f || nb == 0.0f) ? 0.0f : r / (na * nb));
    }
    return r;
}

}  // namespace scann

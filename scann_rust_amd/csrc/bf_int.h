// bf_int.h -- the integer-MFMA shortlist pass of brute force over integer-coded rows (bf_int.hip).
#pragma once
#include "bf.h"

namespace scann {

// int8 digit planes per query (2 or 3): the smaller count with which every query of the 1M x 128 timing workload
// verifies (DESIGN.md 3.3b-i has both measurements)
#ifndef SCANN_BF_INT_DIGITS
#define SCANN_BF_INT_DIGITS 2
#endif
constexpr int kBfIntDigits = SCANN_BF_INT_DIGITS;
static_assert(kBfIntDigits == 2 || kBfIntDigits == 3, "two or three digit planes");

// rows this kernel can read: INT4, dim in {32, 64, 96, 128, 192, 256}, a row of whole 16-byte words on an aligned base
bool bf_int_eligible(const BfIndexDev &ix);
// |score - q.x| <= shortlist_int_err(dim, D) |q||x| for every row; D = 0: without the dropped query residual, which
// the pass carries per query (q_err of bf_int_q_prep: |e_q.x| <= q_err |x|)
float shortlist_int_err(uint32_t dim, int digits);
// bytes of the digit planes / weights of nq queries
size_t bf_int_digit_bytes(uint32_t nq, uint32_t dim);
size_t bf_int_weight_bytes(uint32_t nq);
// queries -> kBfIntDigits int8 planes [D][nq][dim], weights [nq][D] (digit scale * inv_mult), squared-norm upper
// bounds (as bf_q_prep_kernel) and q_err [nq] = an upper bound of the dropped residual's 2-norm.  Enqueue only.
int bf_int_q_prep(const BfIndexDev &ix, const float *d_queries, uint32_t nq, uint32_t q_stride, int8_t *q_digits,
                  float *q_weights, float *q_n2, float *q_err, hipStream_t st);
// (a shortlist pass is never filtered by an allow-list: p.ids / p.allow are not read)
int bf_int_pass(const BfIndexDev &ix, const BfPass &p, const int8_t *q_digits, const float *q_weights,
                const float *q_n2, hipStream_t st);

}  // namespace scann

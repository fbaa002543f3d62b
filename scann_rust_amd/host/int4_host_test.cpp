// int4_host_test.cpp -- the host arithmetic that packed int4 rows added, in a program of its own that needs no GPU and
// is meant to run under the host sanitizers: the 4-bit signed calibration (sq_calibrate's signed4 path) and its
// refusals, the 4-bit codes, the eligibility rule and the bound of the integer shortlist pass.  It compiles the two
// units it calls and supplies the two library functions they reference:
//
//   hipcc -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -x hip \
//       host/int4_host_test.cpp csrc/scalarq.hip csrc/bf_int.hip -o int4_host_test && ./int4_host_test
//
// (The stride and format checks of scann_hip_bf_create_quantized / scann_hip_index_quantize_rows sit behind a device
// context and are covered by tests/test_gpu_int4_rows.py::test_refusals instead.)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../csrc/bf_int.h"
#include "../csrc/comm.h"
#include "../csrc/scalarq.h"

namespace scann {
static std::string g_last;
int fail(int status, const std::string &msg) {
    g_last = msg;
    return status;
}
int ctx_device(const scann_hip_ctx *) { return 0; }
}  // namespace scann

using namespace scann;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

int main() {
    // signed 4-bit calibration: s = (float)(m / 7), params {-m, m, s, 1 / s}, zero point 0; 8-bit stays m / 127
    const float stats[4] = {-0.25f, 3.5f, 0.1f, 1.0f};
    SqParams p{};
    int32_t zp = -1;
    CHECK(sq_calibrate(stats, 4, SCANN_HIP_SQ_SIGNED, 0.0f, 0.0f, &p, &zp, true) == SCANN_HIP_OK);
    CHECK(p.levels == 7 && p.mn == -3.5f && p.mx == 3.5f && p.scale == (float)(3.5 / 7.0) && p.inv_scale == 1.0f / p.scale && zp == 0);
    CHECK(sq_calibrate(stats, 8, SCANN_HIP_SQ_SIGNED, 0.0f, 0.0f, &p, &zp) == SCANN_HIP_OK && p.levels == 127);
    const float zeros[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    CHECK(sq_calibrate(zeros, 4, SCANN_HIP_SQ_SIGNED, 0.0f, 0.0f, &p, &zp, true) == SCANN_HIP_OK && p.scale == 1.0f);
    // refusals: 4 bits without the int4 format, 8 bits with it, non-finite stats; nothing is written
    SqParams keep{1.0f, 2.0f, 3.0f, 4.0f, 5};
    p = keep;
    CHECK(sq_calibrate(stats, 4, SCANN_HIP_SQ_SIGNED, 0.0f, 0.0f, &p, &zp, false) == SCANN_HIP_INVALID_ARGUMENT);
    CHECK(sq_calibrate(stats, 8, SCANN_HIP_SQ_SIGNED, 0.0f, 0.0f, &p, &zp, true) == SCANN_HIP_INVALID_ARGUMENT);
    const float bad[4] = {-1.0f, INFINITY, 0.0f, 1.0f};
    CHECK(sq_calibrate(bad, 4, SCANN_HIP_SQ_SIGNED, 0.0f, 0.0f, &p, &zp, true) == SCANN_HIP_INVALID_ARGUMENT);
    CHECK(p.mn == keep.mn && p.scale == keep.scale && p.levels == keep.levels);
    float out4[4];
    CHECK(scann_hip_scalar_quantizer_calibrate(stats, 4, SCANN_HIP_SQ_SIGNED, 0.0f, 0.0f, out4, &zp) == SCANN_HIP_INVALID_ARGUMENT);
    CHECK(scann_hip_scalar_quantizer_calibrate(stats, 4, SCANN_HIP_SQ_SYMMETRIC, 0.0f, 0.0f, out4, &zp) == SCANN_HIP_OK);
    // 4-bit codes: clip to [-7, 7], ties to even, NaN -> 0; the reference levels wrap into nibbles elsewhere
    CHECK(sq_signed_code(3.5f, 0.5f, 7.0f) == 7 && sq_signed_code(-100.0f, 0.5f, 7.0f) == -7);
    CHECK(sq_signed_code(0.25f, 0.5f, 7.0f) == 0 && sq_signed_code(0.75f, 0.5f, 7.0f) == 2 && sq_signed_code(NAN, 0.5f, 7.0f) == 0);
    CHECK(sq_signed_code(100.0f, 0.5f) == 127);
    // eligibility of the integer pass: INT4, whole 16-byte words on an aligned base, the shortlist's dims
    alignas(16) static unsigned char rows[64];
    BfIndexDev ix{};
    ix.fmt = SCANN_HIP_ROWS_INT4;
    ix.qrows = rows;
    ix.dim = 128;
    ix.stride = 128;
    CHECK(bf_int_eligible(ix));
    ix.stride = 144;
    CHECK(!bf_int_eligible(ix));
    ix.stride = 128;
    ix.qrows = rows + 8;
    CHECK(!bf_int_eligible(ix));
    ix.qrows = rows;
    ix.dim = 48;
    CHECK(!bf_int_eligible(ix));
    ix.dim = 32;
    ix.stride = 32;
    CHECK(bf_int_eligible(ix));
    ix.fmt = SCANN_HIP_ROWS_INT8;
    CHECK(!bf_int_eligible(ix));
    BfPass pass{};
    CHECK(bf_int_pass(ix, pass, nullptr, nullptr, nullptr, nullptr) == SCANN_HIP_INTERNAL);
    // the bound: the residual term shrinks by 254 per digit and vanishes in the per-query form (digits = 0)
    const float e0 = shortlist_int_err(128, 0), e2 = shortlist_int_err(128, 2), e3 = shortlist_int_err(128, 3);
    CHECK(e0 > 0.0f && e0 < e3 && e3 < e2);
    CHECK(std::fabs((e2 - e0) / (e3 - e0) - 254.0f) < 1.0f);
    CHECK(bf_int_digit_bytes(3, 128) == (size_t)kBfIntDigits * 3 * 128 && bf_int_weight_bytes(3) == (size_t)kBfIntDigits * 3 * 4);
    std::printf("int4_host_test ok\n");
    return 0;
}

// projection_test -- scann::Projection's CPU project() (scann.hpp) against hand-computed values: the reference's loop
// (pca.rs:156-180, random.rs:82-92, opq.rs:179-194), out[j] = sum over ascending i of (in[i] - mean[i]) * M[(i, j)] with
// an f32 multiply and then an f32 add per step, and the window copy of TruncateProjection.  Uses no GPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "scann.hpp"

static int g_failed = 0;

#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++g_failed;                                                     \
        }                                                                   \
    } while (0)

static uint32_t bits(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}

template <typename F>
static bool throws_invalid(F f) {
    try {
        f();
    } catch (const scann::ScannError &) {
        return true;
    }
    return false;
}

int main() {
    using scann::Projection;
    {   // matrix: row j of `m` is column j of the reference's DMatrix
        const Projection p = Projection::matrix(3, 2, {1.0f, 0.5f, 0.25f, 2.0f, -1.0f, 0.0f});
        const auto out = p.project({1.0f, 2.0f, 3.0f});
        EXPECT(out.size() == 2 && out[0] == 2.75f && out[1] == 0.0f);
        EXPECT(p.input_dim() == 3 && p.output_dim() == 2 && p.kind() == scann::ProjectionKind::Matrix);
    }
    {   // PCA subtracts the mean first; MATRIX reads none
        const Projection p = Projection::pca(2, 2, {1.0f, 1.0f, 1.0f, -1.0f}, {1.0f, 2.0f});
        auto out = p.project({3.0f, 5.0f});
        EXPECT(out[0] == 5.0f && out[1] == -1.0f);
        out = p.project({1.0f, 1.0f});
        EXPECT(out[0] == -1.0f && out[1] == 1.0f);
        out = Projection::matrix(2, 2, {1.0f, 1.0f, 1.0f, -1.0f}).project({3.0f, 5.0f});
        EXPECT(out[0] == 8.0f && out[1] == -2.0f);
    }
    {   // every step rounds once, in ascending i: ((0 + 2^24) + 1) + 1 stays at 2^24
        const Projection p = Projection::matrix(3, 2, {1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f});
        auto out = p.project({16777216.0f, 1.0f, 1.0f});
        EXPECT(out[0] == 16777216.0f && out[1] == 16777216.0f);
        out = p.project({1.0f, 1.0f, 16777216.0f});   // (1 + 1) + 2^24 is exact
        EXPECT(out[0] == 16777218.0f);
    }
    {   // no fused multiply-add: a * a rounds to 1 + 2^-11 before the add, so the sum is 0, not 2^-24
        const float a = 1.0f + std::ldexp(1.0f, -12), b = 1.0f + std::ldexp(1.0f, -11);
        const auto out = Projection::matrix(2, 1, {a, -1.0f}).project({a, b});
        EXPECT(bits(out[0]) == bits(0.0f));
    }
    {   // identity: the input, with -0.0 becoming +0.0 (0.0 + -0.0 * 1.0) and subnormals kept
        const float sub = std::numeric_limits<float>::denorm_min() * 7.0f;
        std::vector<float> eye(25, 0.0f);
        for (int i = 0; i < 5; ++i) eye[i * 5 + i] = 1.0f;
        const auto out = Projection::matrix(5, 5, eye).project({1.5f, -0.0f, 0.0f, -2.25f, sub});
        EXPECT(out[0] == 1.5f && bits(out[1]) == bits(0.0f) && bits(out[2]) == bits(0.0f) && out[3] == -2.25f);
        EXPECT(bits(out[4]) == bits(sub) && sub > 0.0f);
    }
    {   // an infinite input poisons the other outputs of the row (inf * 0 = NaN); its own output stays infinite
        const auto out = Projection::matrix(2, 2, {1.0f, 0.0f, 0.0f, 1.0f}).project({INFINITY, 2.0f});
        EXPECT(std::isinf(out[0]) && std::isnan(out[1]));
    }
    {   // truncate windows; an untrained PCA is the window from 0
        const std::vector<float> x = {0.0f, 1.0f, 2.0f, 3.0f, 4.0f, 5.0f};
        auto out = Projection::truncate(6, 3, 2).project(x);
        EXPECT(out.size() == 3 && out[0] == 2.0f && out[1] == 3.0f && out[2] == 4.0f);
        out = Projection::truncate(6, 6).project(x);
        EXPECT(out == x);
        out = Projection::truncate(6, 1, 5).project(x);
        EXPECT(out.size() == 1 && out[0] == 5.0f);
        out = Projection::truncate(6, 4).project(x);
        EXPECT(out.size() == 4 && out[3] == 3.0f);
    }
    {   // a dataset, row by row
        const Projection p = Projection::pca(3, 2, {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 2.0f}, {0.5f, 0.0f, -1.0f});
        const auto ds = scann::DenseDataset::from_flat({1.0f, 9.0f, 1.0f, 2.5f, 9.0f, 0.0f}, 3);
        const auto pd = p.project_dataset(ds);
        EXPECT(pd.size() == 2 && pd.dimensionality() == 2);
        EXPECT(pd.get(0)[0] == 0.5f && pd.get(0)[1] == 4.0f && pd.get(1)[0] == 2.0f && pd.get(1)[1] == 2.0f);
    }
    // argument errors
    EXPECT(throws_invalid([] { Projection::matrix(0, 2, {}); }));
    EXPECT(throws_invalid([] { Projection::matrix(2, 0, {}); }));
    EXPECT(throws_invalid([] { Projection::matrix(2, 2, {1.0f, 2.0f, 3.0f}); }));
    EXPECT(throws_invalid([] { Projection::pca(2, 1, {1.0f, 2.0f}, {1.0f}); }));
    EXPECT(throws_invalid([] { Projection::truncate(4, 3, 2); }));
    EXPECT(throws_invalid([] { Projection::truncate(4, 2, 1).project({1.0f, 2.0f, 3.0f}); }));
    if (g_failed) {
        std::printf("projection_test: %d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("projection_test ok\n");
    return 0;
}

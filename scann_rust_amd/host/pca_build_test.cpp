// pca_build_test.cpp -- Projection::train_pca_on_device and build_projected_on_device of the C++ mirror (scann.hpp)
// through scann_hip_pca_train and scann_hip_txh_build_projected.
//   training   the components are orthonormal and carry the variance the data was given; a second training gives the
//              same bits; the trained object projects as a Projection made from its arrays does on the host
//   building   a projected tree and a projected hasher built in one call search like a second build and like the
//              chained route (project on the device, brute-force handle, scann_hip_txh_build without rows: its
//              approximate search of projected queries), bit for bit; bad shapes are refused and the source still searches
// Needs a GPU: without one the first handle fails Unavailable and the program exits 2.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "scann.hpp"

using namespace scann;

static int g_fail = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

template <typename F>
static bool throws(ErrorCode code, F f) {
    try {
        f();
    } catch (const ScannError &e) {
        return e.code == code;
    }
    return false;
}

static uint64_t g_rng = 29;
static float uniform() {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((g_rng >> 40) & 0xFFFF) / 32768.0f - 1.0f;
}
// rows whose column i has amplitude 4 * 0.8^i for i < strong and 0.05 after, mixed pairwise so that no axis is a component
static std::vector<std::vector<float>> spectrum(size_t n, uint32_t dim, uint32_t strong) {
    std::vector<std::vector<float>> rows(n, std::vector<float>(dim));
    for (auto &r : rows) {
        for (uint32_t j = 0; j < dim; ++j) r[j] = (j < strong ? 4.0f * std::pow(0.8f, (float)j) : 0.05f) * uniform();
        for (uint32_t j = 0; j + 1 < dim; j += 2) {
            const float a = r[j], b = r[j + 1];
            r[j] = 0.6f * a - 0.8f * b + 1.5f;
            r[j + 1] = 0.8f * a + 0.6f * b - 0.5f;
        }
    }
    return rows;
}

static bool same(const NNResultsVector &a, const NNResultsVector &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].first != b[i].first || std::memcmp(&a[i].second, &b[i].second, 4)) return false;
    return true;
}

static const uint32_t kDim = 48, kOut = 16;
static const size_t kRows = 3000;

static void training(const std::vector<std::vector<float>> &rows, const BruteForceSearcher &source) {
    uint32_t sweeps = 0;
    bool converged = false;
    std::vector<double> eig;
    DeviceProjection dev = Projection::train_pca_on_device(source, kOut, 0, 42, &sweeps, &converged, &eig);
    EXPECT(converged && sweeps >= 1 && sweeps <= 30);
    EXPECT(eig.size() == kDim);
    for (size_t i = 1; i < eig.size(); ++i) EXPECT(eig[i] <= eig[i - 1]);
    const Projection p = Projection::from_device(dev);
    EXPECT(p.kind() == ProjectionKind::Pca && p.input_dim() == kDim && p.output_dim() == kOut);
    const std::vector<float> &m = p.matrix_rows();
    for (uint32_t a = 0; a < kOut; ++a)
        for (uint32_t b = a; b < kOut; ++b) {
            double dot = 0.0;
            for (uint32_t i = 0; i < kDim; ++i) dot += (double)m[a * kDim + i] * m[b * kDim + i];
            EXPECT(std::fabs(dot - (a == b ? 1.0 : 0.0)) <= std::ldexp(1.0, -22));
        }
    // the variance of the rows along component j is eigenvalue j (f32 projection, f64 sums: a loose 1e-3 relative)
    for (uint32_t j = 0; j < 4; ++j) {
        double s = 0.0, s2 = 0.0;
        for (const auto &r : rows) {
            const double v = p.project(r)[j];
            s += v;
            s2 += v * v;
        }
        const double var = (s2 - s * s / (double)kRows) / (double)(kRows - 1);
        EXPECT(std::fabs(var - eig[j]) <= 1e-3 * eig[0]);
    }
    // a second training: the same bits; the device object projects as the host loop over its arrays does
    DeviceProjection again = Projection::train_pca_on_device(source, kOut);
    const Projection p2 = Projection::from_device(again);
    EXPECT(p2.matrix_rows().size() == m.size() && !std::memcmp(p2.matrix_rows().data(), m.data(), m.size() * 4));
    EXPECT(!std::memcmp(p2.mean().data(), p.mean().data(), kDim * 4));
    const std::vector<float> on_dev = dev.project(rows[7].data(), 1, kDim, kDim), on_host = p.project(rows[7]);
    EXPECT(!std::memcmp(on_dev.data(), on_host.data(), kOut * 4));
    EXPECT(throws(ErrorCode::InvalidArgument, [&] { Projection::train_pca_on_device(source, kDim + 1); }));
    EXPECT(throws(ErrorCode::InvalidArgument, [&] { Projection::train_pca_on_device(source, 0); }));
}

static std::vector<float> flat_rows(const std::vector<std::vector<float>> &rows) {
    std::vector<float> flat(kRows * kDim);
    for (size_t i = 0; i < kRows; ++i) std::memcpy(flat.data() + i * kDim, rows[i].data(), kDim * 4);
    return flat;
}

// Steps 1-3 of the chained route of scann_hip.h "projected device build" through the C ABI: the rows projected by the
// device kernel, a brute-force handle over them, scann_hip_txh_build without rows.  (Step 4 needs the arrays on the host;
// tests/test_gpu_projected_build.py runs it.)  Its approximate search of a projected query is, bit for bit, what the
// projected handle returns for the query itself without exact re-ordering.
static void against_the_chain(const std::vector<std::vector<float>> &rows, const BruteForceSearcher &source,
                              const DeviceProjection &dev, const Projection &host, scann_hip_build_config c) {
    detail::IndexHandle one, bf, plain;
    check(scann_hip_txh_build_projected(source.handle(), dev.handle(), &c, &one.h, nullptr));
    const std::vector<float> projected = dev.project(flat_rows(rows).data(), kRows, kDim, kDim);
    check(scann_hip_bf_create(context(0), projected.data(), kRows, kOut, kOut, SCANN_HIP_SQUARED_L2, &bf.h));
    c.store_rows = 0;
    check(scann_hip_txh_build(bf.h, &c, &plain.h, nullptr));
    scann_hip_search_opts o;
    scann_hip_search_opts_default(&o);
    o.exact_reorder = 0;
    for (size_t q = 0; q < 16; ++q) {
        std::vector<float> query = rows[q * 180];
        query[1] += 0.01f;
        const std::vector<float> qp = host.project(query);
        const auto a = detail::run_search(one.h, query.data(), 1, kDim, kDim, 10, &o)[0];
        const auto b = detail::run_search(plain.h, qp.data(), 1, kOut, kOut, 10, &o)[0];
        EXPECT(a.size() == 10 && same(a, b));
    }
}

static void building(const std::vector<std::vector<float>> &rows, const BruteForceSearcher &source) {
    DeviceProjection dev = Projection::train_pca_on_device(source, kOut, 1000, 7);
    const Projection host = Projection::from_device(dev);
    // a projected tree: two builds agree, rows of the dataset find themselves through the exact re-rank
    TreeXHybridConfig cfg(8, 3);
    cfg.hash_config = AsymmetricHasherConfig(16, 8);
    cfg.hash_config.training_iterations = 6;
    cfg.kmeans_iterations = 15;
    TreeXHybridSearcher a(cfg), b(cfg);
    scann_hip_build_report rep;
    a.build_projected_on_device(source, dev, &rep);
    b.build_projected_on_device(source, dev);
    EXPECT(a.num_partitions() == 8 && a.num_datapoints() == kRows && a.dimensionality() == kDim);
    EXPECT(rep.partition_iterations >= 1 && rep.partition_iterations <= 15);
    size_t hits = 0;
    for (size_t q = 0; q < 16; ++q) {
        const std::vector<float> &query = rows[q * 180];
        const auto ra = a.search(query, 10);
        EXPECT(ra.size() == 10 && same(ra, b.search(query, 10)));
        hits += !ra.empty() && ra[0].first == q * 180 && ra[0].second == 0.0f;
    }
    EXPECT(hits >= 8);    // a sanity bound, not the parity check (tests/test_gpu_projected_build.py)
    scann_hip_build_config c;
    scann_hip_build_config_default(&c);
    c.num_partitions = 8; c.kmeans_iterations = 15; c.num_subspaces = 8; c.num_codes = 16; c.training_iterations = 6;
    c.partitions_to_search = 3;
    against_the_chain(rows, source, dev, host, c);
    // a projected hasher, with and without rows
    AsymmetricHasherConfig hcfg(16, 8);
    hcfg.training_iterations = 6;
    AsymmetricHasher h1(hcfg), h2(hcfg), bare(hcfg);
    h1.build_projected_on_device(source, dev);
    h2.build_projected_on_device(source, dev);
    bare.build_projected_on_device(source, dev, false);
    for (size_t q = 0; q < 12; ++q) {
        std::vector<float> query = rows[q * 150];
        query[0] += 0.01f;
        EXPECT(same(h1.search(query, 10), h2.search(query, 10)));
        EXPECT(same(h1.search(query, 10), bare.search(query, 10)));
        EXPECT(same(h1.search_with_reordering(query, 10, 40), h2.search_with_reordering(query, 10, 40)));
    }
    EXPECT(throws(ErrorCode::FailedPrecondition, [&] { bare.search_with_reordering(rows[0], 5, 20); }));
    c.num_partitions = 0;
    c.partitions_to_search = 1;
    against_the_chain(rows, source, dev, host, c);
    // refusals are judged on out_dim, and the source still searches
    TreeXHybridConfig bad(8, 3);
    bad.hash_config = AsymmetricHasherConfig(16, 24);   // 48 % 24 == 0, 16 % 24 != 0
    TreeXHybridSearcher r(bad);
    EXPECT(throws(ErrorCode::InvalidArgument, [&] { r.build_projected_on_device(source, dev); }));
    DeviceProjection narrow = Projection::truncate(kDim / 2, kOut).to_device();
    EXPECT(throws(ErrorCode::InvalidArgument, [&] { a.build_projected_on_device(source, narrow); }));
    EXPECT(same(source.search(rows[3], 5), BruteForceSearcher(DenseDataset::from_vecs(rows), DistanceMeasure::SquaredL2)
                                               .search(rows[3], 5)));
}

int main() {
    try {
        auto rows = spectrum(kRows, kDim, 12);
        BruteForceSearcher source(DenseDataset::from_vecs(rows), DistanceMeasure::SquaredL2);
        training(rows, source);
        building(rows, source);
    } catch (const ScannError &e) {
        std::printf("ScannError %d: %s\n", (int)e.code, e.what());
        return 2;
    }
    if (g_fail) return 1;
    std::printf("pca_build_test ok\n");
    return 0;
}

// device_build_test.cpp -- build_on_device of the C++ mirror (scann.hpp) through scann_hip_txh_build.
//   AsymmetricHasher      trains what build() trains (same rows, same seeds), so every search of the device-built
//                         hasher equals the host-built one bit for bit; without stored rows the approximate search still
//                         does and the exact reordering is refused (FailedPrecondition)
//   TreeXHybridSearcher   another training order than build(), so it is compared with itself: two builds from the same
//                         source give the same results, the source still searches, both codebook routes
//                         (batched_codebook 1 / 0) give one index, the report counts iterations, bad shapes are refused
// Needs a GPU: without one the first handle fails Unavailable and the program exits 2.
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

static uint64_t g_rng = 23;
static float uniform() {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((g_rng >> 40) & 0xFFFF) / 32768.0f - 1.0f;
}
// `clusters` centres, rows scattered around them
static std::vector<std::vector<float>> clustered(size_t n, uint32_t dim, uint32_t clusters) {
    std::vector<std::vector<float>> cen(clusters, std::vector<float>(dim)), rows(n, std::vector<float>(dim));
    for (auto &c : cen)
        for (auto &v : c) v = 4.0f * uniform();
    for (size_t i = 0; i < n; ++i)
        for (uint32_t j = 0; j < dim; ++j) rows[i][j] = cen[i % clusters][j] + 0.25f * uniform();
    return rows;
}

static bool same(const NNResultsVector &a, const NNResultsVector &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].first != b[i].first || std::memcmp(&a[i].second, &b[i].second, 4)) return false;
    return true;
}

static void hasher() {
    const uint32_t dim = 16;
    auto rows = clustered(2000, dim, 7);
    BruteForceSearcher source(DenseDataset::from_vecs(rows), DistanceMeasure::SquaredL2);
    AsymmetricHasherConfig cfg(16, 8);
    cfg.training_iterations = 6;
    AsymmetricHasher host(cfg), dev(cfg), bare(cfg);
    host.build(DenseDataset::from_vecs(rows));
    scann_hip_build_report rep;
    dev.build_on_device(source, true, &rep);
    bare.build_on_device(source, false);
    EXPECT(dev.num_datapoints() == 2000 && dev.dimensionality() == dim);
    for (uint32_t s = 0; s < 8; ++s) EXPECT(rep.subspace_iterations[s] >= 1 && rep.subspace_iterations[s] <= 6);
    for (size_t q = 0; q < 12; ++q) {
        std::vector<float> query = rows[q * 150];
        query[0] += 0.01f;
        EXPECT(same(dev.search(query, 10), host.search(query, 10)));
        EXPECT(same(dev.search_with_reordering(query, 10, 40), host.search_with_reordering(query, 10, 40)));
        EXPECT(same(bare.search(query, 10), host.search(query, 10)));
    }
    EXPECT(throws(ErrorCode::FailedPrecondition, [&] { bare.search_with_reordering(rows[0], 5, 20); }));
    EXPECT(same(source.search(rows[3], 5), BruteForceSearcher(DenseDataset::from_vecs(rows), DistanceMeasure::SquaredL2)
                                               .search(rows[3], 5)));
}

static void tree() {
    const uint32_t dim = 32;
    auto rows = clustered(3000, dim, 9);
    BruteForceSearcher source(DenseDataset::from_vecs(rows), DistanceMeasure::SquaredL2);
    TreeXHybridConfig cfg(8, 3);
    cfg.hash_config = AsymmetricHasherConfig(16, 8);
    cfg.hash_config.training_iterations = 6;
    cfg.kmeans_iterations = 15;
    TreeXHybridSearcher a(cfg), b(cfg);
    scann_hip_build_report rep;
    a.build_on_device(source, &rep);
    b.build_on_device(source);
    EXPECT(a.num_partitions() == 8 && a.num_datapoints() == 3000 && a.dimensionality() == dim);
    EXPECT(rep.partition_iterations >= 1 && rep.partition_iterations <= 15);
    // the per-subspace codebook route through the C ABI: the same index, so the same results
    scann_hip_build_config c;
    scann_hip_build_config_default(&c);
    c.num_partitions = 8; c.kmeans_iterations = 15; c.num_subspaces = 8; c.num_codes = 16; c.training_iterations = 6;
    c.partitions_to_search = 3; c.batched_codebook = 0;
    detail::IndexHandle per;
    check(scann_hip_txh_build(source.handle(), &c, &per.h, nullptr));
    size_t hits = 0;
    for (size_t q = 0; q < 16; ++q) {
        const std::vector<float> &query = rows[q * 180];
        auto ra = a.search(query, 10);
        EXPECT(ra.size() == 10 && same(ra, b.search(query, 10)));
        EXPECT(same(ra, detail::run_search(per.h, query.data(), 1, dim, dim, 10, nullptr)[0]));
        hits += !ra.empty() && ra[0].first == q * 180 && ra[0].second == 0.0f;
    }
    EXPECT(hits >= 8);    // a row of the dataset finds itself (a sanity bound, not the parity check: tests/test_gpu_device_build.py)
    EXPECT(same(source.search(rows[3], 5), BruteForceSearcher(DenseDataset::from_vecs(rows), DistanceMeasure::SquaredL2)
                                               .search(rows[3], 5)));
    TreeXHybridConfig bad(8, 3);
    bad.hash_config = AsymmetricHasherConfig(16, 24);   // 32 % 24 != 0
    TreeXHybridSearcher r(bad);
    EXPECT(throws(ErrorCode::InvalidArgument, [&] { r.build_on_device(source); }));
    EXPECT(source.search(rows[0], 3).size() == 3);
}

int main() {
    try {
        hasher();
        tree();
    } catch (const ScannError &e) {
        std::printf("ScannError %d: %s\n", (int)e.code, e.what());
        return 2;
    }
    if (g_fail) return 1;
    std::printf("device_build_test ok\n");
    return 0;
}

// hier_build_test.cpp -- build_hierarchical_on_device of the C++ mirror (scann.hpp) through
// scann_hip_txh_build_hierarchical: a tree of 4 children and depth 2 over clustered rows.  The handle searches bit for
// bit like a second build of the same data and like a handle built through the C ABI with the same two configurations;
// the tree report counts what was built, the source still searches, a bad tree configuration is refused.
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

static uint64_t g_rng = 29;
static float uniform() {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((g_rng >> 40) & 0xFFFF) / 32768.0f - 1.0f;
}
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

int main() {
    try {
        const uint32_t dim = 32;
        auto rows = clustered(3000, dim, 16);
        BruteForceSearcher source(DenseDataset::from_vecs(rows), DistanceMeasure::SquaredL2);
        TreeXHybridConfig cfg(8, 3);   // (num_partitions is replaced by the tree's leaves)
        cfg.hash_config = AsymmetricHasherConfig(16, 8);
        cfg.hash_config.training_iterations = 6;
        scann_hip_tree_config tree;
        scann_hip_tree_config_default(&tree);
        EXPECT(tree.num_children == 100 && tree.max_depth == 1 && tree.min_leaf_size == 1 && tree.seed == 42);
        tree.num_children = 4;
        tree.max_depth = 2;
        tree.kmeans_iterations = 15;
        TreeXHybridSearcher a(cfg), b(cfg);
        scann_hip_build_report rep;
        scann_hip_tree_report trep;
        a.build_hierarchical_on_device(source, tree, &rep, &trep);
        b.build_hierarchical_on_device(source, tree);
        EXPECT(a.num_datapoints() == 3000 && a.dimensionality() == dim);
        EXPECT(trep.num_leaves >= 2 && trep.num_leaves <= 16 && a.num_partitions() == trep.num_leaves);
        EXPECT(trep.depth_reached == 2 && trep.level_nodes[0] == 1 && trep.level_nodes[1] >= 2 && trep.level_nodes[1] <= 4);
        EXPECT(trep.level_leaves[0] + trep.level_leaves[1] + trep.level_leaves[2] == trep.num_leaves);
        EXPECT(rep.partition_iterations >= 1 && rep.partition_iterations <= 15);
        EXPECT(trep.level_iterations[0] == rep.partition_iterations);
        // the same two configurations through the C ABI
        scann_hip_build_config c;
        scann_hip_build_config_default(&c);
        c.num_subspaces = 8; c.num_codes = 16; c.training_iterations = 6; c.partitions_to_search = 3;
        detail::IndexHandle abi;
        check(scann_hip_txh_build_hierarchical(source.handle(), &tree, &c, &abi.h, nullptr, nullptr));
        size_t hits = 0;
        for (size_t q = 0; q < 16; ++q) {
            const std::vector<float> &query = rows[q * 180];
            auto ra = a.search(query, 10);
            EXPECT(ra.size() == 10 && same(ra, b.search(query, 10)));
            EXPECT(same(ra, detail::run_search(abi.h, query.data(), 1, dim, dim, 10, nullptr)[0]));
            hits += !ra.empty() && ra[0].first == q * 180 && ra[0].second == 0.0f;
        }
        EXPECT(hits >= 8);   // a row of the dataset finds itself (a sanity bound; the parity check is tests/test_gpu_hier_build.py)
        EXPECT(same(source.search(rows[3], 5),
                    BruteForceSearcher(DenseDataset::from_vecs(rows), DistanceMeasure::SquaredL2).search(rows[3], 5)));
        scann_hip_tree_config bad = tree;
        bad.num_children = 0;
        TreeXHybridSearcher r(cfg);
        EXPECT(throws(ErrorCode::InvalidArgument, [&] { r.build_hierarchical_on_device(source, bad); }));
        bad = tree;
        bad.max_depth = 5;
        EXPECT(throws(ErrorCode::Unimplemented, [&] { r.build_hierarchical_on_device(source, bad); }));
        EXPECT(source.search(rows[0], 3).size() == 3);
    } catch (const ScannError &e) {
        std::printf("ScannError %d: %s\n", (int)e.code, e.what());
        return 2;
    }
    if (g_fail) return 1;
    std::printf("hier_build_test ok\n");
    return 0;
}

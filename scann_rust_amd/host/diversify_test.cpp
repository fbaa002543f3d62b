// diversify_test.cpp -- CrowdingMultidimensional / MmrDiversifier of the C++ mirror (scann.hpp) against the
// reference's own unit-test data (restricts/crowding.rs:313-374).  Host only by default; with the argument "gpu" the
// same vectors also go through BruteForceSearcher::search_with_crowding_md and search_with_mmr on the device.
#include <cstdio>
#include <cstring>

#include "scann.hpp"

using namespace scann;

static int g_fail = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

// test_multidimensional_crowding's attributes (:315-333): category and region of six datapoints, limits [2, 2]
static CrowdingMultidimensional reference_md() {
    CrowdingMultidimensional c(2, 6);
    const uint64_t category[6] = {1, 1, 2, 2, 3, 3}, region[6] = {10, 10, 10, 20, 20, 30};
    for (uint32_t i = 0; i < 6; ++i) {
        c.set_attribute(0, i, category[i]);
        c.set_attribute(1, i, region[i]);
    }
    c.set_limits({2, 2});
    return c;
}

static bool indices_are(const NNResultsVector &r, std::initializer_list<uint32_t> want) {
    if (r.size() != want.size()) return false;
    size_t i = 0;
    for (uint32_t w : want)
        if (r[i++].first != w) return false;
    return true;
}

static void host_checks() {
    const NNResultsVector results = {{0, 0.1f}, {1, 0.2f}, {2, 0.3f}, {3, 0.4f}, {4, 0.5f}, {5, 0.6f}};
    CrowdingMultidimensional c = reference_md();
    // 0, 1 fill category 1 and region 10; 2 is rejected by region 10; 3, 4 fill category 2 / 3 and region 20; 5 is kept
    NNResultsVector f = c.apply(results, 6);
    EXPECT(indices_are(f, {0, 1, 3, 4, 5}));
    for (const auto &r : f) EXPECT(r.second == results[r.first].second);
    EXPECT(indices_are(c.apply(results, 3), {0, 1, 3}));   // stops at k kept
    // defaults: no limit; out-of-range set_attribute is ignored; a missing datapoint has attribute 0 in every dimension
    CrowdingMultidimensional d(2, 3);
    EXPECT(d.limits().size() == 2 && d.limits()[0] == std::numeric_limits<size_t>::max());
    d.set_attribute(2, 0, 9);
    d.set_attribute(0, 3, 9);
    EXPECT(d.get_attributes(0) == std::vector<uint64_t>({0, 0}) && d.get_attributes(7) == std::vector<uint64_t>({0, 0}));
    EXPECT(d.apply(results, 6).size() == 6);
    d.set_limits({1, 100});
    EXPECT(indices_are(d.apply(results, 6), {0}));          // everything shares attribute 0 in dimension 0
    d.set_limits({0, 100});
    EXPECT(d.apply(results, 6).empty());
    d.set_limits({1});                                      // the reference panics on limits[1]
    bool threw = false;
    try {
        d.apply(results, 6);
    } catch (const ScannError &) {
        threw = true;
    }
    EXPECT(threw);
    // the chain: dimension 0 = p / 2, dimension 1 = (p + 1) / 2, limits (1, 1): exactly the even positions are kept --
    // each decision depends on the previous REJECTION (a count of earlier entries would keep only entry 0)
    CrowdingMultidimensional chain(2, 10);
    NNResultsVector row;
    for (uint32_t p = 0; p < 10; ++p) {
        chain.set_attribute(0, p, p / 2);
        chain.set_attribute(1, p, (p + 1) / 2);
        row.emplace_back(p, 0.5f * (float)p);
    }
    chain.set_limits({1, 1});
    EXPECT(indices_are(chain.apply(row, 10), {0, 2, 4, 6, 8}));

    // test_mmr_diversifier (:353-374): lambda 0.5, identity similarity, k = 3
    const NNResultsVector cand = {{0, 0.1f}, {1, 0.2f}, {2, 0.3f}, {3, 0.4f}};
    auto ident = [](DatapointIndex a, DatapointIndex b) { return a == b ? 1.0f : 0.0f; };
    EXPECT(indices_are(MmrDiversifier(0.5f).apply(cand, 3, ident), {0, 1, 2}));
    EXPECT(MmrDiversifier(0.5f).apply(cand, 0, ident).empty() && MmrDiversifier(0.5f).apply({}, 3, ident).empty());
    EXPECT(MmrDiversifier(-1.0f).lambda == 0.0f && MmrDiversifier(7.0f).lambda == 1.0f);
    // lambda = 1 on finite similarities: the first k of the row
    EXPECT(indices_are(MmrDiversifier(1.0f).apply(cand, 4, [](DatapointIndex a, DatapointIndex b) { return (float)(a * b); }),
                       {0, 1, 2, 3}));
    // lambda = 0: pure diversity; 1 and 0 are similar, 3 is the least similar to 0
    auto sim = [](DatapointIndex a, DatapointIndex b) { return -std::fabs((float)a - (float)b); };
    EXPECT(indices_are(MmrDiversifier(0.0f).apply(cand, 2, sim), {0, 3}));
    // every similarity NaN: max_sim stays f32::MIN; the scores tie at -(1 - lambda) * MIN and the lowest position wins
    auto nan_sim = [](DatapointIndex, DatapointIndex) { return std::numeric_limits<float>::quiet_NaN(); };
    EXPECT(indices_are(MmrDiversifier(0.5f).apply(cand, 4, nan_sim), {0, 1, 2, 3}));
    // every score NaN (inf - inf): no score exceeds f32::MIN, best_idx stays 0 -> row order
    const NNResultsVector infs = {{0, -INFINITY}, {1, -INFINITY}, {2, -INFINITY}};
    auto inf_sim = [](DatapointIndex, DatapointIndex) { return INFINITY; };
    EXPECT(indices_are(MmrDiversifier(0.5f).apply(infs, 3, inf_sim), {0, 1, 2}));
}

static void gpu_checks() {
    // rows (i + 1, 0, 0, 0), query 0 -> the plain row is 0..5 with distances (i + 1)^2
    std::vector<std::vector<float>> rows;
    for (int i = 0; i < 6; ++i) rows.push_back({(float)(i + 1), 0, 0, 0});
    BruteForceSearcher bf(DenseDataset::from_vecs(rows), DistanceMeasure::SquaredL2);
    const std::vector<float> q = {0, 0, 0, 0};
    CrowdingMultidimensional c = reference_md();
    NNResultsVector r = bf.search_with_crowding_md(q, 6, 6, c);
    EXPECT(indices_are(r, {0, 1, 3, 4, 5}));
    EXPECT(r == c.apply(bf.search(q, 6), 6));
    EXPECT(indices_are(bf.search_with_crowding_md(q, 3, 0, c), {0, 1}));   // depth 0 = k = 3: 2 is rejected
    c.set_attribute(1, 2, 40);                                             // the change is attached again
    EXPECT(indices_are(bf.search_with_crowding_md(q, 6, 6, c), {0, 1, 2, 3, 4, 5}));
    // MMR through the handle against the host walk with sim = -SquaredL2 of the stored rows
    auto sim = [&](DatapointIndex a, DatapointIndex b) {
        const float d = rows[a][0] - rows[b][0];
        return -(d * d);
    };
    for (float lambda : {0.0f, 0.3f, 0.5f, 1.0f}) {
        const MmrDiversifier mmr(lambda);
        r = bf.search_with_mmr(q, 4, 6, mmr);
        EXPECT(r == mmr.apply(bf.search(q, 6), 4, sim));
        EXPECT(r.size() == 4 && r[0].first == 0);
    }
    EXPECT(bf.search_with_mmr(q, 2, 6, MmrDiversifier(0.0f))[1].first == 5);   // pure diversity: the farthest from row 0
}

int main(int argc, char **argv) {
    try {
        host_checks();
        if (argc > 1 && !std::strcmp(argv[1], "gpu")) gpu_checks();
    } catch (const ScannError &e) {
        std::printf("ScannError %d: %s\n", (int)e.code, e.what());
        return 2;
    }
    if (g_fail) return 1;
    std::printf("diversify_test ok\n");
    return 0;
}

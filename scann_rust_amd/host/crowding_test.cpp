// crowding_test.cpp -- CrowdingConfig / CrowdingConstraint of the C++ mirror (scann.hpp) against the reference's own
// unit tests (restricts/crowding.rs:274-311) and set_attribute's resize-with-0 (:69-75).  Host only by default; with
// the argument "gpu" the same vector also goes through BruteForceSearcher::search_with_crowding and
// search_crowded_exact on the device.
#include <cstdio>
#include <cstring>

#include "scann.hpp"

using namespace scann;

static int g_fail = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

static void host_checks() {
    // test_crowding_constraint (:275-299)
    CrowdingConstraint c({0, 0, 0, 1, 1, 2}, CrowdingConfig(2));
    const NNResultsVector results = {{0, 0.1f}, {1, 0.2f}, {2, 0.3f}, {3, 0.4f}, {4, 0.5f}, {5, 0.6f}};
    NNResultsVector f = c.apply(results, 6);
    EXPECT(f.size() == 5);
    const uint32_t want[5] = {0, 1, 3, 4, 5};
    for (size_t i = 0; i < f.size() && i < 5; ++i) EXPECT(f[i].first == want[i] && f[i].second == results[want[i]].second);
    f = c.apply(results, 3);                      // stops at k kept
    EXPECT(f.size() == 3 && f[2].first == 3);
    // test_crowding_disabled (:301-311)
    CrowdingConstraint d({0, 0, 0}, CrowdingConfig::disabled());
    EXPECT(!d.config().enabled && d.config().per_crowd_limit == std::numeric_limits<size_t>::max());
    EXPECT(d.apply({{0, 0.1f}, {1, 0.2f}, {2, 0.3f}}, 3).size() == 3);
    EXPECT(d.apply({{0, 0.1f}, {1, 0.2f}, {2, 0.3f}}, 2).size() == 2);
    EXPECT(!d.would_violate(0, {{1, 0.2f}, {2, 0.3f}}));
    // defaults and limit 0
    EXPECT(CrowdingConfig().per_crowd_limit == 3 && CrowdingConfig().enabled);
    EXPECT(CrowdingConstraint({0, 1, 2}, CrowdingConfig(0)).apply(results, 6).empty());
    // an index past the array has attribute 0 and crowds with the real zeros
    CrowdingConstraint s({7, 0}, CrowdingConfig(1));
    uint64_t a = 99;
    EXPECT(s.get_attribute(1, &a) && a == 0);
    EXPECT(!s.get_attribute(2, &a));
    f = s.apply({{5, 0.1f}, {1, 0.2f}, {0, 0.3f}, {9, 0.4f}}, 4);
    EXPECT(f.size() == 2 && f[0].first == 5 && f[1].first == 0);
    // set_attribute: resize with 0, then the value
    const uint64_t stamp = s.stamp();
    s.set_attribute(5, 7);
    EXPECT(s.attributes().size() == 6 && s.attributes()[2] == 0 && s.attributes()[4] == 0 && s.attributes()[5] == 7);
    EXPECT(s.stamp() != stamp);
    f = s.apply({{5, 0.1f}, {1, 0.2f}, {0, 0.3f}, {9, 0.4f}}, 4);   // 5 and 0 now share attribute 7
    EXPECT(f.size() == 2 && f[0].first == 5 && f[1].first == 1);
    s.set_attribute(1, 3);
    EXPECT(s.attributes().size() == 6 && s.attributes()[1] == 3);
    // would_violate (:107-119)
    EXPECT(c.would_violate(2, {{0, 0.1f}, {1, 0.2f}}));
    EXPECT(!c.would_violate(3, {{0, 0.1f}, {1, 0.2f}}));
    EXPECT(c.would_violate(100, {{0, 0.1f}, {1, 0.2f}}));   // missing attribute = 0
}

static void gpu_checks() {
    // the reference's vector through a handle: rows (i + 1, 0, 0, 0), query 0 -> distances (i + 1)^2 ascending in i
    std::vector<std::vector<float>> rows;
    for (int i = 0; i < 6; ++i) rows.push_back({(float)(i + 1), 0, 0, 0});
    BruteForceSearcher bf(DenseDataset::from_vecs(rows), DistanceMeasure::SquaredL2);
    CrowdingConstraint c({0, 0, 0, 1, 1, 2}, CrowdingConfig(2));
    const std::vector<float> q = {0, 0, 0, 0};
    NNResultsVector r = bf.search_with_crowding(q, 6, 6, c);
    const uint32_t want[5] = {0, 1, 3, 4, 5};
    EXPECT(r.size() == 5);
    for (size_t i = 0; i < r.size() && i < 5; ++i) EXPECT(r[i].first == want[i] && r[i].second == (float)((want[i] + 1) * (want[i] + 1)));
    EXPECT(r == c.apply(bf.search(q, 6), 6));
    // depth 0 = k; a disabled constraint is the plain search
    r = bf.search_with_crowding(q, 3, 0, c);
    EXPECT(r.size() == 2 && r[1].first == 1);
    EXPECT(bf.search_with_crowding(q, 3, 0, CrowdingConstraint({0, 0, 0}, CrowdingConfig::disabled())) == bf.search(q, 3));
    // exact: deepens from 3 to 6 to find the third attribute
    CrowdingConstraint one({0, 0, 0, 1, 1, 2}, CrowdingConfig(1));
    auto e = bf.search_crowded_exact(q, 3, one);
    EXPECT(e.second && e.first.size() == 3 && e.first[0].first == 0 && e.first[1].first == 3 && e.first[2].first == 5);
    e = bf.search_crowded_exact(q, 5, one);   // only three attributes exist: the whole index was walked
    EXPECT(e.second && e.first.size() == 3);
    // the attributes follow the constraint: a changed constraint is attached again
    one.set_attribute(1, 9);
    e = bf.search_crowded_exact(q, 3, one);
    EXPECT(e.second && e.first.size() == 3 && e.first[1].first == 1 && e.first[2].first == 3);
    Scann sc = Scann::brute_force(DenseDataset::from_vecs(rows));
    EXPECT(sc.search_with_crowding(q, 6, 6, c).size() == 5);
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
    std::printf("crowding_test ok\n");
    return 0;
}

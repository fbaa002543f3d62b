// bf_filter_test.cpp -- filtered brute force through the C++ mirror (scann.hpp) on the 5-point cube set of the
// reference's searcher tests (brute_force/searcher.rs:280-376).  The reference's BruteForceSearcher has no filter
// argument; the contract is the search over the allowed rows alone (include/scann_hip.h, allow_bitmap).
#include <cmath>
#include <cstdio>

#include "scann.hpp"

using namespace scann;

static int g_fail = 0;
#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
    } while (0)

static DenseDataset cube() {
    return DenseDataset::from_vecs({{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 1}});
}

static void filtered_searches(DistanceMeasure measure) {
    BruteForceSearcher s(cube(), measure);
    const float one = 1.0f, three = measure == DistanceMeasure::L2 ? std::sqrt(3.0f) : 3.0f;
    // the exact match is denied: it must not come back, and the three unit points (distance 1) lead
    RestrictDenylist deny = RestrictDenylist::from_indices({0}, 5);
    auto r = s.search_with_filter({0, 0, 0}, 3, &deny);
    EXPECT(r.size() == 3);
    for (auto &p : r) EXPECT(p.first != 0 && p.second == one);
    EXPECT(r.size() == 3 && r[0].first == 1 && r[1].first == 2 && r[2].first == 3);   // (distance, index) order
    // k beyond the allowed rows: all four of them, sorted
    r = s.search_with_filter({0, 0, 0}, 5, &deny);
    EXPECT(r.size() == 4 && r[3].first == 4 && r[3].second == three);
    // an allow-list of two rows, one of them past the capacity of a short list
    RestrictAllowlist allow = RestrictAllowlist::from_indices({4, 2}, 5);
    r = s.search_with_filter({0, 0, 0}, 3, &allow);
    EXPECT(r.size() == 2 && r[0].first == 2 && r[1].first == 4);
    RestrictAllowlist short_list = RestrictAllowlist::from_indices({1, 4}, 3);   // 4 >= capacity: not allowed
    r = s.search_with_filter({0, 0, 0}, 3, &short_list);
    EXPECT(r.size() == 1 && r[0].first == 1);
    // nothing allowed, no filter
    RestrictAllowlist none(5);
    EXPECT(s.search_with_filter({0, 0, 0}, 3, &none).empty());
    r = s.search_with_filter({0, 0, 0}, 3, nullptr);
    EXPECT(r.size() == 3 && r[0].first == 0);
    // radius: origin + 3 unit points within 1.5 (test_brute_force_radius); without the origin, three
    auto rr = s.search_radius_with_filter({0, 0, 0}, 1.5f, &deny);
    EXPECT(rr.size() == 3 && rr[0].first == 1 && rr[2].first == 3);
    rr = s.search_radius_with_filter({0, 0, 0}, 1.5f, &none);
    EXPECT(rr.empty());
    rr = s.search_radius_with_filter({0, 0, 0}, 1.5f, nullptr);
    EXPECT(rr.size() == 4 && rr[0].first == 0);
    // the filter of one call does not stick to the next
    r = s.search({0, 0, 0}, 1);
    EXPECT(r.size() == 1 && r[0].first == 0);
}

int main() {
    try {
        filtered_searches(DistanceMeasure::SquaredL2);
        filtered_searches(DistanceMeasure::L2);
    } catch (const ScannError &e) {
        std::printf("ScannError %d: %s\n", (int)e.code, e.what());
        return 2;
    }
    if (g_fail) return 1;
    std::printf("bf_filter_test ok\n");
    return 0;
}

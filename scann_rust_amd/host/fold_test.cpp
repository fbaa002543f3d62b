// fold_test.cpp -- MutableIndex::compact of the C++ mirror (scann.hpp) on the device: scann_hip_fold_mutable over a
// brute-force base.  After every compact the expected answer of a search is a BruteForceSearcher built from the live
// rows in ascending id order, indices mapped back, compared bit for bit; ids, rows and the id sequence survive; the
// new base holds its rows on the device only.  Needs a GPU: without one the first handle fails Unavailable and the
// program exits 2.
#include <cstdio>
#include <cstring>
#include <map>

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

static uint64_t g_rng = 11;
static uint32_t rnd(uint32_t n) {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_rng >> 33) % n);
}
// small integers: many exact ties, in every measure
static std::vector<float> small_row(uint32_t dim) {
    std::vector<float> r(dim);
    for (auto &v : r) v = (float)rnd(3) - 1.0f;
    return r;
}

using Live = std::map<DatapointIndex, std::vector<float>>;   // the model: id -> row, ascending

static void check_search(const MutableIndex &m, const Live &live, DistanceMeasure measure,
                         const std::vector<std::vector<float>> &queries, size_t k, const char *what) {
    std::vector<std::vector<float>> rows;
    std::vector<DatapointIndex> ids;
    for (auto &kv : live) {
        ids.push_back(kv.first);
        rows.push_back(kv.second);
    }
    EXPECT(m.size() == live.size());
    auto got = m.search_batched(queries, k);
    BruteForceSearcher ref(DenseDataset::from_vecs(rows), measure);
    auto want = ref.search_batched(queries, k);
    for (size_t q = 0; q < queries.size(); ++q) {
        bool same = got[q].size() == want[q].size();
        for (size_t i = 0; same && i < want[q].size(); ++i)
            same = got[q][i].first == ids[want[q][i].first] && !std::memcmp(&got[q][i].second, &want[q][i].second, 4);
        if (!same) {
            std::printf("FAIL %s: query %zu differs from the search over the live rows\n", what, q);
            ++g_fail;
        }
    }
}

// the ids compact() returned, the rows behind them and the state of the handle
static void check_compacted(const MutableIndex &m, const Live &live, const std::vector<DatapointIndex> &ids) {
    EXPECT(ids.size() == live.size() && m.pending() == 0 && m.size() == live.size());
    EXPECT(m.base().dataset_size() == live.size() && m.base().dataset().size() == 0);   // rows on the device only
    size_t i = 0;
    for (auto &kv : live) {
        EXPECT(i < ids.size() && ids[i] == kv.first);
        ++i;
    }
    auto ex = m.export_live();
    EXPECT(ex.second == ids);
    i = 0;
    for (auto &kv : live) {
        EXPECT(!std::memcmp(ex.first.get(i), kv.second.data(), kv.second.size() * 4));
        std::vector<float> r;
        EXPECT(m.get(kv.first, &r) && r == kv.second);
        ++i;
    }
}

static void script(DistanceMeasure measure, uint32_t dim) {
    const uint32_t n = 700, k = 10;
    std::vector<std::vector<float>> rows(n), queries(9);
    for (auto &r : rows) r = small_row(dim);
    for (auto &q : queries) q = small_row(dim);
    Live live;
    for (uint32_t i = 0; i < n; ++i) live[i] = rows[i];
    MutableIndex m(std::make_shared<BruteForceSearcher>(DenseDataset::from_vecs(rows), measure), 256);
    // nothing mutated: the ids are 0 .. n - 1 and the answers those of the base
    auto before = m.search_batched(queries, k);
    auto ids = m.compact();
    check_compacted(m, live, ids);
    EXPECT(m.search_batched(queries, k) == before);
    // adds (high ids), updates of low ids, removes across a bitmap word boundary
    std::vector<std::vector<float>> add(90);
    for (uint32_t i = 0; i < 90; ++i) add[i] = i % 7 == 0 ? rows[rnd(n)] : small_row(dim);
    auto added = m.add_batch(add);
    EXPECT(added.size() == 90 && added[0] == n);
    for (uint32_t i = 0; i < 90; ++i) live[added[i]] = add[i];
    for (uint32_t i = 0; i < 40; ++i) {
        const DatapointIndex id = 1 + i * 5;
        auto r = i % 4 == 0 ? rows[400 + i] : small_row(dim);
        m.update(id, r);
        live[id] = r;
    }
    std::vector<DatapointIndex> rm;
    for (uint32_t id = 58; id < 70; ++id) rm.push_back(id);
    for (uint32_t i = 0; i < 10; ++i) rm.push_back(n + i * 6);
    m.remove_batch(rm);
    for (auto id : rm) live.erase(id);
    check_search(m, live, measure, queries, k, "before compact");
    before = m.search_batched(queries, k);
    ids = m.compact();
    check_compacted(m, live, ids);
    EXPECT(m.search_batched(queries, k) == before);
    check_search(m, live, measure, queries, k, "after compact");
    EXPECT(throws(ErrorCode::NotFound, [&] { m.remove(rm[3]); }));
    // life after it: the id sequence goes on, mutations on non-dense ids, a filter over external ids, a second compact
    auto more = m.add(small_row(dim));
    EXPECT(more == n + 90);
    std::vector<float> mr;
    EXPECT(m.get(more, &mr));
    live[more] = mr;
    m.remove(ids[100]);
    live.erase(ids[100]);
    m.update(ids[3], rows[650]);
    live[ids[3]] = rows[650];
    check_search(m, live, measure, queries, k, "mutated again");
    RestrictAllowlist allow = RestrictAllowlist::from_indices({more, ids[3], ids[100]}, n + 200);
    auto fr = m.search(queries[0], k, &allow, n + 200);
    EXPECT(fr.size() == 2);
    for (auto &e : fr) EXPECT(e.first == more || e.first == ids[3]);
    ids = m.compact();
    check_compacted(m, live, ids);
    check_search(m, live, measure, queries, k, "after the second compact");
}

static void refusals() {
    const uint32_t dim = 8;
    std::vector<std::vector<float>> rows(20);
    for (auto &r : rows) r = small_row(dim);
    MutableIndex m(std::make_shared<BruteForceSearcher>(DenseDataset::from_vecs(rows), DistanceMeasure::SquaredL2), 4);
    std::vector<DatapointIndex> all(20);
    for (uint32_t i = 0; i < 20; ++i) all[i] = i;
    m.remove_batch(all);
    EXPECT(m.size() == 0 && m.pending() == 20);
    EXPECT(throws(ErrorCode::FailedPrecondition, [&] { m.compact(); }));
    EXPECT(m.size() == 0 && m.pending() == 20 && m.search(rows[0], 3).empty());
    auto id = m.add(rows[5]);                  // the delta alone becomes the base
    EXPECT(id == 20);
    auto ids = m.compact();
    EXPECT(ids.size() == 1 && ids[0] == 20 && m.size() == 1);
    auto r = m.search(rows[5], 3);
    EXPECT(r.size() == 1 && r[0].first == 20);
}

int main() {
    try {
        const DistanceMeasure all[5] = {DistanceMeasure::SquaredL2, DistanceMeasure::L2, DistanceMeasure::DotProduct,
                                        DistanceMeasure::L1, DistanceMeasure::Cosine};
        for (auto measure : all) script(measure, 24);
        script(DistanceMeasure::DotProduct, 19);
        refusals();
    } catch (const ScannError &e) {
        std::printf("ScannError %d: %s\n", (int)e.code, e.what());
        return 2;
    }
    if (g_fail) return 1;
    std::printf("fold_test ok\n");
    return 0;
}

// mutable_test.cpp -- MutableIndex of the C++ mirror (scann.hpp) on the device: the mutation script, export / compact
// and the host-side refusals of include/scann_hip.h "mutable indexes".  The expected answer of every search is the
// contract itself: a BruteForceSearcher built from the live rows in ascending id order, indices mapped back, compared
// bit for bit.  Needs a GPU: without one the first handle fails Unavailable and the program exits 2.
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

static uint64_t g_rng = 7;
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
    if (rows.empty()) {
        for (auto &r : got) EXPECT(r.empty());
        return;
    }
    BruteForceSearcher ref(DenseDataset::from_vecs(rows), measure);
    auto want = ref.search_batched(queries, k);
    for (size_t q = 0; q < queries.size(); ++q) {
        bool same = got[q].size() == want[q].size();
        for (size_t i = 0; same && i < want[q].size(); ++i)
            same = got[q][i].first == ids[want[q][i].first] &&
                   !std::memcmp(&got[q][i].second, &want[q][i].second, 4);
        if (!same) {
            std::printf("FAIL %s: query %zu differs from the search over the live rows\n", what, q);
            ++g_fail;
        }
    }
}

static void script(DistanceMeasure measure, uint32_t dim) {
    const uint32_t n = 600, k = 10;
    std::vector<std::vector<float>> rows(n), queries(9);
    for (auto &r : rows) r = small_row(dim);
    for (auto &q : queries) q = small_row(dim);
    Live live;
    for (uint32_t i = 0; i < n; ++i) live[i] = rows[i];
    auto base = std::make_shared<BruteForceSearcher>(DenseDataset::from_vecs(rows), measure);
    MutableIndex m(base, 128);
    check_search(m, live, measure, queries, k, "no mutation");
    // add 70 rows, some of them copies of base rows
    std::vector<std::vector<float>> add(70);
    for (uint32_t i = 0; i < 70; ++i) add[i] = i % 7 == 0 ? rows[rnd(n)] : small_row(dim);
    auto ids = m.add_batch(add);
    EXPECT(ids.size() == 70 && ids[0] == n && ids[69] == n + 69);
    for (uint32_t i = 0; i < 70; ++i) live[ids[i]] = add[i];
    check_search(m, live, measure, queries, k, "add");
    // remove 40 base and 10 delta ids
    std::vector<DatapointIndex> rm;
    for (uint32_t i = 0; i < 40; ++i) rm.push_back(i * 13 % n);
    for (uint32_t i = 0; i < 10; ++i) rm.push_back(n + i * 6);
    m.remove_batch(rm);
    for (auto id : rm) live.erase(id);
    check_search(m, live, measure, queries, k, "remove");
    // update 15 base and 5 delta ids; a LOW id becomes a copy of a higher base row (it must win that tie from a late slot)
    std::vector<DatapointIndex> up;
    std::vector<std::vector<float>> upr;
    for (uint32_t i = 0; i < 15; ++i) {
        up.push_back(1 + i * 2);
        upr.push_back(rows[300 + i * 17 % 300]);
    }
    for (uint32_t i = 0; i < 5; ++i) {
        up.push_back(n + 1 + i * 6);
        upr.push_back(small_row(dim));
    }
    m.update_batch(up, upr);
    for (size_t i = 0; i < up.size(); ++i) live[up[i]] = upr[i];
    check_search(m, live, measure, queries, k, "update");
    // revive 3 removed ids (two base, one delta); remove one id twice
    const DatapointIndex rev[3] = {rm[0], rm[5], rm[41]};
    for (auto id : rev) {
        EXPECT(!m.exists(id));
        auto r = small_row(dim);
        m.update(id, r);
        live[id] = r;
        EXPECT(m.exists(id));
    }
    m.remove(rm[7]);
    m.remove(rm[7]);
    check_search(m, live, measure, queries, k, "revive");
    for (auto &kv : live) {
        std::vector<float> r;
        EXPECT(m.get(kv.first, &r) && r == kv.second);
    }
    EXPECT(!m.get(rm[7], nullptr));
    EXPECT(m.pending() == 70 + 50 + 20 + 3 + 2 && m.needs_rebuild(145) && !m.needs_rebuild(146));

    // export / compact: the same rows, the same answers, the delta empty, dropped ids forgotten
    auto ex = m.export_live();
    EXPECT(ex.second.size() == live.size());
    size_t i = 0;
    for (auto &kv : live) {
        EXPECT(i < ex.second.size() && ex.second[i] == kv.first &&
               !std::memcmp(ex.first.get(i), kv.second.data(), (size_t)dim * 4));
        ++i;
    }
    auto before = m.search_batched(queries, k);
    m.compact();
    EXPECT(m.pending() == 0 && m.size() == live.size());
    EXPECT(m.search_batched(queries, k) == before);
    EXPECT(throws(ErrorCode::NotFound, [&] { m.remove(rm[7]); }));
    EXPECT(throws(ErrorCode::NotFound, [&] { m.update(rm[7], small_row(dim)); }));
    // mutations on the now non-dense ids
    auto more = m.add(small_row(dim));
    EXPECT(more == n + 70);
    std::vector<float> got;
    EXPECT(m.get(more, &got));
    live[more] = got;
    auto first = live.begin()->first;
    m.remove(first);
    live.erase(first);
    auto moved = std::next(live.begin(), 5)->first;
    m.update(moved, rows[599]);
    live[moved] = rows[599];
    check_search(m, live, measure, queries, k, "after compact");
    RestrictAllowlist allow = RestrictAllowlist::from_indices({moved, more, 3, rm[7]}, n + 200);
    auto fr = m.search(queries[0], k, &allow, n + 200);
    for (auto &e : fr) EXPECT(e.first == moved || e.first == more || (e.first == 3 && live.count(3)));
    EXPECT(fr.size() == 2 + (live.count(3) ? 1 : 0));
    std::vector<DatapointIndex> bad = ex.second;
    std::swap(bad[0], bad[1]);
    auto nb = std::make_shared<BruteForceSearcher>(ex.first, measure);
    EXPECT(throws(ErrorCode::InvalidArgument, [&] { m.rebase(nb, &bad); }));
}

static void refusals() {
    const uint32_t dim = 8;
    std::vector<std::vector<float>> rows(20);
    for (auto &r : rows) r = small_row(dim);
    auto base = std::make_shared<BruteForceSearcher>(DenseDataset::from_vecs(rows), DistanceMeasure::SquaredL2);
    EXPECT(throws(ErrorCode::InvalidArgument, [&] { MutableIndex z(base, 0); }));
    EXPECT(throws(ErrorCode::InvalidArgument, [&] { MutableIndex z(base, SCANN_HIP_MUTABLE_MAX_CAPACITY + 1); }));
    MutableIndex m(base, 4);
    const std::vector<std::vector<float>> q = {small_row(dim)};
    EXPECT(throws(ErrorCode::InvalidArgument, [&] { m.add(small_row(dim + 1)); }));
    EXPECT(throws(ErrorCode::InvalidArgument, [&] { m.update(0, small_row(dim - 1)); }));
    EXPECT(throws(ErrorCode::InvalidArgument, [&] { m.search(small_row(dim + 1), 3); }));
    EXPECT(throws(ErrorCode::InvalidArgument, [&] { m.search(q[0], SCANN_HIP_MUTABLE_MAX_K + 1); }));
    EXPECT(throws(ErrorCode::NotFound, [&] { m.remove(20); }));
    EXPECT(m.pending() == 0 && m.size() == 20);
    // a full delta changes nothing
    auto ids = m.add_batch({small_row(dim), small_row(dim), small_row(dim), small_row(dim)});
    auto before = m.search_batched(q, 24);
    EXPECT(before[0].size() == 24);
    EXPECT(throws(ErrorCode::ResourceExhausted, [&] { m.add(small_row(dim)); }));
    EXPECT(throws(ErrorCode::ResourceExhausted, [&] { m.update(0, small_row(dim)); }));
    EXPECT(m.pending() == 4 && m.size() == 24 && m.search_batched(q, 24) == before);
    EXPECT(m.add_batch({}).empty());
    // all or nothing: the third element is unknown
    EXPECT(throws(ErrorCode::NotFound, [&] { m.remove_batch({1, 2, 999}); }));
    EXPECT(throws(ErrorCode::NotFound, [&] { m.update_batch({ids[0], ids[1], 999}, {rows[0], rows[1], rows[2]}); }));
    EXPECT(m.pending() == 4 && m.exists(1) && m.exists(2) && m.search_batched(q, 24) == before);
    m.update(ids[0], rows[3]);   // in place: needs no slot
    EXPECT(m.pending() == 5);
}

int main() {
    try {
        const DistanceMeasure all[5] = {DistanceMeasure::SquaredL2, DistanceMeasure::L2, DistanceMeasure::DotProduct,
                                        DistanceMeasure::L1, DistanceMeasure::Cosine};
        for (auto measure : all) script(measure, 24);
        script(DistanceMeasure::SquaredL2, 19);
        script(DistanceMeasure::DotProduct, 19);
        refusals();
    } catch (const ScannError &e) {
        std::printf("ScannError %d: %s\n", (int)e.code, e.what());
        return 2;
    }
    if (g_fail) return 1;
    std::printf("mutable_test ok\n");
    return 0;
}

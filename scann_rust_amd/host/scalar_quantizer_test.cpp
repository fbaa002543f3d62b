// scalar_quantizer_test.cpp -- the scalar quantizer of the C++ mirror (scann.hpp): the reference's own unit tests of
// quantization/mod.rs:150-163, quantization/scalar.rs:411-454 and brute_force/scalar_quantized.rs:424-513 replayed,
// then the device route (ScalarQuantizedBruteForceSearcher::create = scann_hip_index_quantize_rows) against the host
// route (QuantizedDataset::from_dataset + from_quantized) bit for bit.  The quantizer arithmetic needs no GPU; the
// searchers do: without one the first handle fails Unavailable and the program exits 2.
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

// ---- no GPU needed ---------------------------------------------------------------------------------
static void test_quantization_stats() {   // mod.rs:150-163
    auto stats = QuantizationStats::from_vecs({{1.0f, 2.0f, 3.0f}, {4.0f, 5.0f, 6.0f}});
    EXPECT(stats.min_value == 1.0f);
    EXPECT(stats.max_value == 6.0f);
    EXPECT(std::fabs(stats.mean - 3.5f) < 0.01f);
}

static void test_scalar_quantizer_basic() {   // scalar.rs:411-431
    ScalarQuantizer quantizer(ScalarQuantizerConfig::int8());
    QuantizationStats stats;
    stats.min_value = -1.0f; stats.max_value = 1.0f; stats.mean = 0.0f; stats.std_dev = 0.5f;
    quantizer.calibrate(stats);
    EXPECT(quantizer.min_value() == -1.0f && quantizer.max_value() == 1.0f && quantizer.zero_point() == 128);
    const float original = 0.5f;
    const float dequantized = quantizer.dequantize_value(quantizer.quantize_value(original));
    EXPECT(std::fabs(original - dequantized) < 0.02f);
    // int4, an explicit range, the symmetric config, refusals
    ScalarQuantizer q4(ScalarQuantizerConfig::int4().with_range(0.0f, 15.0f));
    q4.calibrate(stats);
    EXPECT(q4.scale() == 1.0f && q4.quantize_value(7.5f) == 8 && q4.quantize_value(99.0f) == 15);
    ScalarQuantizer qs(ScalarQuantizerConfig::int8().symmetric());
    stats.min_value = -0.25f;
    qs.calibrate(stats);
    EXPECT(qs.min_value() == -1.0f && qs.max_value() == 1.0f);
    ScalarQuantizer bad(ScalarQuantizerConfig::int8().with_range(2.0f, 1.0f));
    EXPECT(throws(ErrorCode::InvalidArgument, [&] { bad.calibrate(stats); }));
    ScalarQuantizerConfig c5;
    c5.bits = 5;
    ScalarQuantizer q5(c5);
    EXPECT(throws(ErrorCode::InvalidArgument, [&] { q5.calibrate(stats); }));
    // the wrap: 128 .. 255 are stored as -128 .. -1 and come back as 128 .. 255
    ScalarQuantizer q8(ScalarQuantizerConfig::int8().with_range(0.0f, 255.0f));
    q8.calibrate(stats);
    EXPECT(q8.quantize_value(127.0f) == 127 && q8.quantize_value(127.5f) == -128 && q8.quantize_value(255.0f) == -1);
    EXPECT(q8.dequantize_value(-128) == 128.0f && q8.dequantize_value(-1) == 255.0f);
}

static void test_quantized_dataset() {   // scalar.rs:433-454
    auto dataset = DenseDataset::from_vecs({{1.0f, 2.0f, 3.0f}, {4.0f, 5.0f, 6.0f}, {-1.0f, 0.0f, 1.0f}});
    auto qdata = QuantizedDataset::from_dataset(dataset, ScalarQuantizer(ScalarQuantizerConfig::int8()));
    EXPECT(qdata.size() == 3 && qdata.dimensionality() == 3);
    auto dequant = qdata.get_dequantized(1);
    EXPECT(std::fabs(dequant[0] - 4.0f) < 1.0f && std::fabs(dequant[1] - 5.0f) < 1.0f && std::fabs(dequant[2] - 6.0f) < 1.0f);
    EXPECT(throws(ErrorCode::InvalidArgument,
                  [&] { QuantizedDataset::from_dataset(DenseDataset(), ScalarQuantizer(ScalarQuantizerConfig::int8())); }));
}

// ---- on the device -----------------------------------------------------------------------------------
static DenseDataset create_test_dataset() {
    return DenseDataset::from_vecs({{0.0f, 0.0f, 0.0f}, {10.0f, 0.0f, 0.0f}, {0.0f, 10.0f, 0.0f}, {0.0f, 0.0f, 10.0f},
                                    {10.0f, 10.0f, 10.0f}});
}

static bool same(const NNResultsVector &a, const NNResultsVector &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].first != b[i].first || std::memcmp(&a[i].second, &b[i].second, 4)) return false;
    return true;
}

// the device route against the host route: the same quantizer, the same answers
static void check_routes(const DenseDataset &ds, const ScalarQuantizedConfig &config,
                         const std::vector<std::vector<float>> &queries, size_t k) {
    auto dev = ScalarQuantizedBruteForceSearcher::create(ds, config);
    auto qdata = QuantizedDataset::from_dataset(ds, ScalarQuantizer(config.quantizer_config));
    auto host = ScalarQuantizedBruteForceSearcher::from_quantized(qdata, config.distance_measure);
    const ScalarQuantizer &a = dev.quantizer(), &b = qdata.quantizer();
    EXPECT(a.min_value() == b.min_value() && a.max_value() == b.max_value() && a.scale() == b.scale() &&
           a.zero_point() == b.zero_point());
    auto ra = dev.search_batched(queries, k), rb = host.search_batched(queries, k);
    EXPECT(ra.size() == rb.size());
    for (size_t q = 0; q < ra.size() && q < rb.size(); ++q) {
        EXPECT(same(ra[q], rb[q]));
        EXPECT(same(dev.search(queries[q], k), rb[q]));
        EXPECT(same(dev.search_radius(queries[q], 60.0f), host.search_radius(queries[q], 60.0f)));
    }
}

static void test_scalar_quantized_search() {   // scalar_quantized.rs:424-435
    auto searcher = ScalarQuantizedBruteForceSearcher::create(create_test_dataset(), ScalarQuantizedConfig::squared_l2());
    auto results = searcher.search({0.0f, 0.0f, 0.0f}, 3);
    EXPECT(results.size() == 3);
    EXPECT(!results.empty() && results[0].first == 0);
    EXPECT(searcher.dataset_size() == 5 && searcher.dimensionality() == 3);
    EXPECT(throws(ErrorCode::InvalidArgument, [&] { searcher.search({0.0f, 0.0f}, 3); }));
    EXPECT(throws(ErrorCode::InvalidArgument,
                  [&] { ScalarQuantizedBruteForceSearcher::create(DenseDataset(), ScalarQuantizedConfig::squared_l2()); }));
}

static void test_scalar_quantized_search_dot_product() {   // :437-451
    auto dataset = DenseDataset::from_vecs({{10.0f, 0.0f}, {0.0f, 10.0f}, {10.0f, 10.0f}});
    auto searcher = ScalarQuantizedBruteForceSearcher::create(dataset, ScalarQuantizedConfig::dot_product());
    EXPECT(searcher.search({1.0f, 0.0f}, 3).size() == 3);
}

static void test_scalar_quantized_batched() {   // :453-468
    auto searcher = ScalarQuantizedBruteForceSearcher::create(create_test_dataset(),
                                                              ScalarQuantizedConfig::squared_l2().with_parallel(false));
    auto results = searcher.search_batched({{0.0f, 0.0f, 0.0f}, {10.0f, 10.0f, 10.0f}}, 2);
    EXPECT(results.size() == 2 && results[0].size() == 2 && results[1].size() == 2);
}

static void test_compression_ratio() {   // :470-483
    auto dataset = DenseDataset::from_vecs({std::vector<float>(128, 1.0f), std::vector<float>(128, 2.0f),
                                            std::vector<float>(128, 3.0f)});
    auto searcher = ScalarQuantizedBruteForceSearcher::create(dataset, ScalarQuantizedConfig::squared_l2());
    const float ratio = searcher.compression_ratio();
    EXPECT(ratio > 3.0f && ratio < 5.0f);
    EXPECT(searcher.memory_usage() >= 3 * 128);
}

static void test_accuracy_vs_float() {   // :485-513
    auto dataset = DenseDataset::from_vecs({{1.0f, 2.0f, 3.0f}, {4.0f, 5.0f, 6.0f}, {7.0f, 8.0f, 9.0f}, {1.1f, 2.1f, 3.1f},
                                            {10.0f, 0.0f, 0.0f}});
    BruteForceSearcher float_searcher(dataset, DistanceMeasure::SquaredL2);
    auto quantized_searcher = ScalarQuantizedBruteForceSearcher::create(dataset, ScalarQuantizedConfig::squared_l2());
    const std::vector<float> query = {1.0f, 2.0f, 3.0f};
    auto float_results = float_searcher.search(query, 3);
    auto quant_results = quantized_searcher.search(query, 3);
    EXPECT(!quant_results.empty() && float_results[0].first == quant_results[0].first);
    // the device's statistics of the resident rows are the reference's
    auto host = QuantizationStats::from_dataset(dataset);
    auto dev = QuantizationStats::from_index(float_searcher.handle());
    EXPECT(host.min_value == dev.min_value && host.max_value == dev.max_value && host.mean == dev.mean &&
           host.std_dev == dev.std_dev);
}

static void test_routes() {
    const std::vector<std::vector<float>> q3 = {{0.0f, 0.0f, 0.0f}, {10.0f, 10.0f, 10.0f}, {3.0f, -1.0f, 7.5f}};
    for (auto measure : {DistanceMeasure::SquaredL2, DistanceMeasure::L2, DistanceMeasure::DotProduct}) {
        ScalarQuantizedConfig c = ScalarQuantizedConfig::squared_l2().with_distance(measure);
        check_routes(create_test_dataset(), c, q3, 4);
        c.quantizer_config = ScalarQuantizerConfig::int8().symmetric();
        check_routes(create_test_dataset(), c, q3, 4);
        c.quantizer_config = ScalarQuantizerConfig::int4().with_range(-1.0f, 6.0f);
        check_routes(create_test_dataset(), c, q3, 5);
    }
    EXPECT(throws(ErrorCode::Unimplemented, [&] {
        ScalarQuantizedBruteForceSearcher::create(create_test_dataset(), ScalarQuantizedConfig::squared_l2().with_distance(DistanceMeasure::L1));
    }));
}

int main() {
    test_quantization_stats();
    test_scalar_quantizer_basic();
    test_quantized_dataset();
    try {
        test_scalar_quantized_search();
        test_scalar_quantized_search_dot_product();
        test_scalar_quantized_batched();
        test_compression_ratio();
        test_accuracy_vs_float();
        test_routes();
    } catch (const ScannError &e) {
        std::printf("ScannError %d: %s\n", (int)e.code, e.what());
        return 2;
    }
    if (g_fail) return 1;
    std::printf("scalar_quantizer_test ok\n");
    return 0;
}

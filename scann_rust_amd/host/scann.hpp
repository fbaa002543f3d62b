// scann.hpp -- C++ host-side mirror of the reference crate's API for the hot path, on top
// of the C ABI (include/scann_hip.h).  The reference is Rust; the build image has no Rust
// toolchain, so this header plays the role of the Rust wrappers shown in INTEGRATION.md:
// same type / method names, argument meaning and error behaviour.
//
//   scann::DenseDataset                 data_format/dataset.rs:46-280
//   scann::BruteForceSearcher           brute_force/searcher.rs:18-208
//   scann::QuantizationStats, ScalarQuantizer(+Config), QuantizedDataset   quantization/mod.rs:62-145, scalar.rs:10-300
//   scann::ScalarQuantizedBruteForceSearcher(+Config)   brute_force/scalar_quantized.rs:24-348 (`create` is its `new`)
//   scann::AsymmetricHasher(+Config)    hashes/hasher.rs:19-258
//   scann::TreeXHybridSearcher(+Config) tree_x_hybrid/mod.rs:23-418
//   scann::ScannBuilder / scann::Scann  scann.rs:35-56, 364-426
//   scann::MutableIndex                 mutator/mod.rs:233-490 (MutableDataset), 492-560 (IncrementalUpdater's counter)
//   scann::ScannError / ErrorCode       error.rs:10-147
//
// All distance computation and top-k selection runs in libscann_hip.so on the GPU.  Index
// TRAINING (k-means, PQ codebooks) is host-side C++ here with its own RNG: the reference's
// StdRng streams are not reproducible and the trained index is an input to
// the search path.  Encoding uses the GPU (scann_hip_encode, bit-exact with Codebook::encode).
#pragma once

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/scann_hip.h"

namespace scann {

enum class ErrorCode : int {   // error.rs:10-45, declaration order
    Ok = 0, Cancelled, Unknown, InvalidArgument, DeadlineExceeded, NotFound, AlreadyExists,
    PermissionDenied, ResourceExhausted, FailedPrecondition, Aborted, OutOfRange, Unimplemented,
    Internal, Unavailable, DataLoss, Unauthenticated
};

struct ScannError : std::runtime_error {   // error.rs:73-147
    ErrorCode code;
    ScannError(ErrorCode c, const std::string &m) : std::runtime_error(m), code(c) {}
    static ScannError invalid_argument(const std::string &m) { return {ErrorCode::InvalidArgument, m}; }
    static ScannError failed_precondition(const std::string &m) { return {ErrorCode::FailedPrecondition, m}; }
};

inline void check(int status) {
    if (status != SCANN_HIP_OK) throw ScannError(static_cast<ErrorCode>(status), scann_hip_last_error());
}

enum class DistanceMeasure : int { SquaredL2 = 0, L2 = 1, DotProduct = 2, L1 = 3, Cosine = 4 };  // distance_measures/mod.rs:32-66 (the dense measures of the hot path)

using DatapointIndex = uint32_t;                                   // types.rs:10
using NNResultsVector = std::vector<std::pair<DatapointIndex, float>>;  // types.rs:17-20

// One context per device, shared by every searcher of the process.
inline scann_hip_ctx *context(int device = 0) {
    static scann_hip_ctx *ctxs[64] = {};
    if (device < 0 || device >= 64) throw ScannError::invalid_argument("device id");
    if (!ctxs[device]) check(scann_hip_init(device, &ctxs[device]));
    return ctxs[device];
}

// quantization/fp8.rs: the reference's FP8 codec and quantizer on the device (its own bit-level conversion,
// restated bit for bit by scann_hip_fp8_quantize / _dequantize; see include/scann_hip.h).
enum class Fp8Format : int { E4M3 = 0, E5M2 = 1 };               // fp8.rs:8-19

struct Fp8Config {                                               // fp8.rs:22-62
    Fp8Format format = Fp8Format::E4M3;
    float scale = 1.0f;
    static Fp8Config e4m3() { return Fp8Config{}; }
    static Fp8Config e5m2() { return Fp8Config{Fp8Format::E5M2, 1.0f}; }
    Fp8Config with_scale(float s) const { return Fp8Config{format, s}; }
};

class Fp8Quantizer {                                             // fp8.rs:206-273
public:
    explicit Fp8Quantizer(Fp8Config config = Fp8Config{}, int device = 0) : config_(config), device_(device) {}
    static Fp8Quantizer e4m3() { return Fp8Quantizer(Fp8Config::e4m3()); }
    static Fp8Quantizer e5m2() { return Fp8Quantizer(Fp8Config::e5m2()); }
    Fp8Format format() const { return config_.format; }
    float scale() const { return config_.scale; }
    size_t bits() const { return 8; }
    void calibrate_scale(float max_abs_value) {                  // :238-244
        const float fp8_max = config_.format == Fp8Format::E4M3 ? 448.0f : 57344.0f;
        config_.scale = fp8_max / std::max(max_abs_value, 1e-10f);
    }
    std::vector<uint8_t> quantize(const std::vector<float> &values) const {      // Quantizer::quantize
        std::vector<uint8_t> out(values.size());
        check(scann_hip_fp8_quantize(context(device_), values.data(), values.size(), config_.scale, (int)config_.format,
                                     out.data()));
        return out;
    }
    std::vector<float> dequantize(const std::vector<uint8_t> &bits) const {      // Quantizer::dequantize
        std::vector<float> out(bits.size());
        check(scann_hip_fp8_dequantize(context(device_), bits.data(), bits.size(), config_.scale, (int)config_.format,
                                       out.data()));
        return out;
    }

private:
    Fp8Config config_;
    int device_;
};

// one_to_many_fp8_float_{squared_l2,dot_product} (distance_measures/one_to_many_asymmetric.rs:327-377)
inline std::vector<float> one_to_many_fp8(const std::vector<float> &query, const std::vector<uint8_t> &database,
                                          size_t stride, size_t num_points, DistanceMeasure measure, int device = 0) {
    std::vector<float> out(num_points);
    check(scann_hip_fp8_distances(context(device), query.data(), (uint32_t)query.size(), database.data(), stride,
                                  num_points, (int)measure, out.data()));
    return out;
}

// data_format/dataset.rs: one row-major buffer, stride = align_up(dim, 16 floats).
class DenseDataset {
public:
    DenseDataset() = default;
    static DenseDataset from_vecs(const std::vector<std::vector<float>> &vecs) {  // :99-123
        DenseDataset d;
        if (vecs.empty()) return d;
        d.dim_ = static_cast<uint32_t>(vecs[0].size());
        d.n_ = vecs.size();
        d.stride_ = scann_hip_compute_stride(d.dim_);
        d.data_.assign(d.n_ * d.stride_, 0.0f);
        for (size_t i = 0; i < d.n_; ++i)
            std::memcpy(&d.data_[i * d.stride_], vecs[i].data(), std::min<size_t>(vecs[i].size(), d.dim_) * 4);
        return d;
    }
    static DenseDataset from_flat(const std::vector<float> &flat, uint32_t dim) {  // :126-174
        if (dim == 0) throw ScannError::invalid_argument("Dimensionality cannot be 0");
        if (flat.size() % dim) throw ScannError::invalid_argument("Data length is not a multiple of dimensionality");
        DenseDataset d;
        d.dim_ = dim;
        d.n_ = flat.size() / dim;
        d.stride_ = scann_hip_compute_stride(dim);
        d.data_.assign(d.n_ * d.stride_, 0.0f);
        for (size_t i = 0; i < d.n_; ++i) std::memcpy(&d.data_[i * d.stride_], &flat[i * dim], dim * 4);
        return d;
    }
    bool is_empty() const { return n_ == 0; }
    size_t size() const { return n_; }
    uint32_t dimensionality() const { return dim_; }
    uint32_t stride() const { return stride_; }
    const float *raw_data() const { return data_.data(); }
    const float *get(size_t i) const { return &data_[i * stride_]; }

private:
    std::vector<float> data_;
    size_t n_ = 0;
    uint32_t dim_ = 0, stride_ = 0;
};

// ---- restricts (restricts/mod.rs:16-45, restricts/allowlist.rs:8-187) ----------------------------
struct RestrictFilter {
    virtual ~RestrictFilter() = default;
    virtual bool is_allowed(DatapointIndex index) const = 0;
    // Words of an allow-bitmap covering datapoints [0, n): bit i = is_allowed(i).
    virtual std::vector<uint64_t> to_bitmap(size_t n) const {
        std::vector<uint64_t> w((n + 63) / 64, 0);
        for (size_t i = 0; i < n; ++i)
            if (is_allowed((DatapointIndex)i)) w[i >> 6] |= 1ull << (i & 63);
        return w;
    }
};

class RestrictAllowlist : public RestrictFilter {   // allowlist.rs:8-105
public:
    explicit RestrictAllowlist(size_t capacity) : bits_((capacity + 63) / 64, 0), capacity_(capacity) {}
    static RestrictAllowlist from_indices(const std::vector<DatapointIndex> &indices, size_t capacity) {
        RestrictAllowlist a(capacity);
        for (auto i : indices) a.add(i);
        return a;
    }
    void add(DatapointIndex i) {
        if (i < capacity_ && !get(i)) { bits_[i >> 6] |= 1ull << (i & 63); ++count_; }
    }
    void remove(DatapointIndex i) {
        if (i < capacity_ && get(i)) { bits_[i >> 6] &= ~(1ull << (i & 63)); --count_; }
    }
    void clear() { std::fill(bits_.begin(), bits_.end(), 0); count_ = 0; }
    size_t capacity() const { return capacity_; }
    size_t num_allowed() const { return count_; }
    bool is_allowed(DatapointIndex i) const override { return i < capacity_ && get(i); }
    std::vector<uint64_t> to_bitmap(size_t n) const override {
        std::vector<uint64_t> w = bits_;
        w.resize((n + 63) / 64, 0);
        if (n & 63) w.back() &= (1ull << (n & 63)) - 1;
        return w;
    }

private:
    bool get(DatapointIndex i) const { return (bits_[i >> 6] >> (i & 63)) & 1ull; }
    std::vector<uint64_t> bits_;
    size_t capacity_, count_ = 0;
};

class RestrictDenylist : public RestrictFilter {    // allowlist.rs:107-187
public:
    explicit RestrictDenylist(size_t capacity) : deny_(capacity) {}
    static RestrictDenylist from_indices(const std::vector<DatapointIndex> &indices, size_t capacity) {
        RestrictDenylist d(capacity);
        for (auto i : indices) d.deny(i);
        return d;
    }
    void deny(DatapointIndex i) { deny_.add(i); }
    void allow(DatapointIndex i) { deny_.remove(i); }
    void clear() { deny_.clear(); }
    bool is_allowed(DatapointIndex i) const override { return !deny_.is_allowed(i); }

private:
    RestrictAllowlist deny_;
};

// Range-based filter (restricts/mod.rs:73-95): allows indices in [start, end).  num_allowed is end - start where the
// range is well formed and 0 where it is not (start > end: the reference's subtraction underflows there).
class RangeFilter : public RestrictFilter {
public:
    RangeFilter(DatapointIndex start, DatapointIndex end) : start_(start), end_(end) {}
    bool is_allowed(DatapointIndex index) const override { return index >= start_ && index < end_; }
    size_t num_allowed() const { return end_ > start_ ? (size_t)(end_ - start_) : 0; }
    DatapointIndex start() const { return start_; }
    DatapointIndex end() const { return end_; }
    // the same filter as a clause on an AttributeTable's row-index column: lo = start, hi = end - 1 as i64
    scann_hip_range_bound lo_bound() const { scann_hip_range_bound b; b.i64 = (int64_t)start_; return b; }
    scann_hip_range_bound hi_bound() const { scann_hip_range_bound b; b.i64 = (int64_t)end_ - 1; return b; }

private:
    DatapointIndex start_, end_;
};

// Typed attribute columns resident on the device (scann_hip_attr_table): int64 and float columns of one value per
// datapoint, uploaded once; a batch names clause columns and gives one inclusive range per (query, clause).  The
// table is a snapshot: build a new one to change a value.
class AttributeTable {
public:
    static constexpr uint32_t kRowIndex = SCANN_HIP_ATTR_ROW_INDEX;   // the clause column of RangeFilter
    AttributeTable() = default;
    explicit AttributeTable(scann_hip_attr_table *h) : h_(h) {}
    // columns of num_datapoints values each; types[c] is SCANN_HIP_ATTR_I64 (int64_t) or SCANN_HIP_ATTR_F32 (float)
    AttributeTable(scann_hip_ctx *ctx, size_t num_datapoints, const std::vector<int32_t> &types,
                   const std::vector<const void *> &columns) {
        if (types.size() != columns.size()) throw ScannError::invalid_argument("one type per column");
        check(scann_hip_attr_table_create(ctx, num_datapoints, (uint32_t)types.size(), types.data(), columns.data(), &h_));
    }
    AttributeTable(const AttributeTable &) = delete;
    AttributeTable &operator=(const AttributeTable &) = delete;
    AttributeTable(AttributeTable &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    AttributeTable &operator=(AttributeTable &&o) noexcept {
        if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; }
        return *this;
    }
    ~AttributeTable() { reset(); }
    void reset() { if (h_) scann_hip_attr_table_destroy(h_); h_ = nullptr; }
    scann_hip_attr_table *handle() const { return h_; }
    size_t num_datapoints() const { return h_ ? (size_t)scann_hip_attr_table_num_datapoints(h_) : 0; }
    size_t num_columns() const { return h_ ? (size_t)scann_hip_attr_table_num_columns(h_) : 0; }
    int column_type(uint32_t column) const { return h_ ? scann_hip_attr_table_column_type(h_, column) : 0; }
    static scann_hip_range_bound i64_bound(int64_t v) { scann_hip_range_bound b; b.i64 = v; return b; }
    static scann_hip_range_bound f32_bound(float v) { scann_hip_range_bound b; b.bits = 0; b.f32 = v; return b; }
    // one bitmap per query ([nq][ceil(n / 64)] words): bounds[q * cols.size() * 2 + c * 2 + {0, 1}] = lo, hi
    std::vector<uint64_t> allow_bitmaps(const std::vector<uint32_t> &cols, const std::vector<scann_hip_range_bound> &bounds,
                                        size_t nq) const {
        if (!h_) throw ScannError::failed_precondition("the attribute table is not on the device");
        if (bounds.size() != nq * cols.size() * 2) throw ScannError::invalid_argument("two bounds per query and clause");
        const size_t words = (num_datapoints() + 63) / 64;
        std::vector<uint64_t> out(nq * words);
        check(scann_hip_attr_table_allow_bitmaps(h_, cols.data(), (uint32_t)cols.size(), bounds.data(), (uint32_t)nq, 0, words,
                                                 out.data()));
        return out;
    }

private:
    scann_hip_attr_table *h_ = nullptr;
};

// A RestrictTokenMap resident on the device (scann_hip_token_map): what RestrictTokenMap::to_device returns.  The
// map is a snapshot: tokens added to the host map afterwards are not in it (build a new one).
class DeviceTokenMap {
public:
    DeviceTokenMap() = default;
    explicit DeviceTokenMap(scann_hip_token_map *h) : h_(h) {}
    DeviceTokenMap(const DeviceTokenMap &) = delete;
    DeviceTokenMap &operator=(const DeviceTokenMap &) = delete;
    DeviceTokenMap(DeviceTokenMap &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    DeviceTokenMap &operator=(DeviceTokenMap &&o) noexcept {
        if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; }
        return *this;
    }
    ~DeviceTokenMap() { reset(); }
    void reset() { if (h_) scann_hip_token_map_destroy(h_); h_ = nullptr; }
    scann_hip_token_map *handle() const { return h_; }
    size_t num_tokens() const { return h_ ? (size_t)scann_hip_token_map_num_tokens(h_) : 0; }
    size_t num_datapoints() const { return h_ ? (size_t)scann_hip_token_map_num_datapoints(h_) : 0; }

private:
    scann_hip_token_map *h_ = nullptr;
};

// Token-based filtering for multi-valued attributes (allowlist.rs:184-244): each datapoint carries any number of
// tokens; the filter allows datapoints that have at least one of the query's tokens.  The host type is the
// reference's: get_indices keeps insertion order, duplicates and out-of-range indices.
class RestrictTokenMap {
public:
    explicit RestrictTokenMap(size_t num_datapoints) : num_datapoints_(num_datapoints) {}                    // :198-203
    void add_token(DatapointIndex index, uint64_t token) { token_to_indices_[token].push_back(index); }      // :206-211
    void set_tokens(DatapointIndex index, const std::vector<uint64_t> &tokens) {                              // :214-218
        for (uint64_t t : tokens) add_token(index, t);
    }
    // nullptr for an unknown token (the reference's None)
    const std::vector<DatapointIndex> *get_indices(uint64_t token) const {                                    // :221-223
        const auto it = token_to_indices_.find(token);
        return it == token_to_indices_.end() ? nullptr : &it->second;
    }
    RestrictAllowlist create_allowlist(const std::vector<uint64_t> &tokens) const {                           // :226-238
        RestrictAllowlist a(num_datapoints_);
        for (uint64_t t : tokens)
            if (const auto *ix = get_indices(t))
                for (DatapointIndex i : *ix) a.add(i);
        return a;
    }
    size_t num_tokens() const { return token_to_indices_.size(); }                                            // :241-243
    size_t num_datapoints() const { return num_datapoints_; }
    // The map as it stands, uploaded once: scann_hip_token_map_create over every (index, token) pair.
    DeviceTokenMap to_device(scann_hip_ctx *ctx) const {
        std::vector<uint32_t> idx;
        std::vector<uint64_t> tok;
        for (const auto &kv : token_to_indices_)
            for (DatapointIndex i : kv.second) { idx.push_back(i); tok.push_back(kv.first); }
        scann_hip_token_map *h = nullptr;
        check(scann_hip_token_map_create(ctx, num_datapoints_, idx.data(), tok.data(), idx.size(), &h));
        return DeviceTokenMap(h);
    }

private:
    std::unordered_map<uint64_t, std::vector<DatapointIndex>> token_to_indices_;
    size_t num_datapoints_;
};

// ---- crowding (restricts/crowding.rs:10-120) --------------------------------------------------------
struct CrowdingConfig {              // crowding.rs:10-44
    size_t per_crowd_limit = 3;
    bool enabled = true;
    CrowdingConfig() = default;
    explicit CrowdingConfig(size_t limit) : per_crowd_limit(limit), enabled(true) {}
    static CrowdingConfig disabled() {
        CrowdingConfig c(std::numeric_limits<size_t>::max());
        c.enabled = false;
        return c;
    }
};

class CrowdingConstraint {           // crowding.rs:46-120
public:
    CrowdingConstraint(std::vector<uint64_t> crowding_attributes, CrowdingConfig config)
        : attrs_(std::move(crowding_attributes)), config_(config), stamp_(next_stamp()) {}
    bool get_attribute(DatapointIndex index, uint64_t *out) const {   // Option<u64>: false = None
        if ((size_t)index >= attrs_.size()) return false;
        *out = attrs_[index];
        return true;
    }
    uint64_t attribute_or_zero(DatapointIndex index) const {          // get_attribute(idx).unwrap_or(0), :90
        return (size_t)index < attrs_.size() ? attrs_[index] : 0;
    }
    void set_attribute(DatapointIndex index, uint64_t attribute) {    // :69-75: resize with 0
        if ((size_t)index >= attrs_.size()) attrs_.resize((size_t)index + 1, 0);
        attrs_[index] = attribute;
        stamp_ = next_stamp();
    }
    // The plain host walk (:81-104), statement for statement -- including that it tests `len >= k` only after a push.
    NNResultsVector apply(const NNResultsVector &results, size_t k) const {
        if (!config_.enabled) return NNResultsVector(results.begin(), results.begin() + std::min(k, results.size()));
        std::unordered_map<uint64_t, size_t> crowd_counts;
        NNResultsVector filtered;
        filtered.reserve(std::min(k, results.size()));
        for (const auto &r : results) {
            size_t &count = crowd_counts[attribute_or_zero(r.first)];
            if (count < config_.per_crowd_limit) {
                filtered.push_back(r);
                ++count;
                if (filtered.size() >= k) break;
            }
        }
        return filtered;
    }
    bool would_violate(DatapointIndex index, const NNResultsVector &current_results) const {   // :107-119
        if (!config_.enabled) return false;
        const uint64_t attribute = attribute_or_zero(index);
        size_t count = 0;
        for (const auto &r : current_results) count += attribute_or_zero(r.first) == attribute ? 1 : 0;
        return count >= config_.per_crowd_limit;
    }
    const CrowdingConfig &config() const { return config_; }
    const std::vector<uint64_t> &attributes() const { return attrs_; }
    // changes whenever the attributes do (and differs between constraints): what a searcher remembers having attached
    uint64_t stamp() const { return stamp_; }

private:
    static uint64_t next_stamp() {
        static std::atomic<uint64_t> s{0};
        return ++s;
    }
    std::vector<uint64_t> attrs_;
    CrowdingConfig config_;
    uint64_t stamp_;
};

class CrowdingMultidimensional {     // crowding.rs:122-201
public:
    CrowdingMultidimensional(size_t num_dimensions, size_t num_datapoints)      // new (:134-140)
        : attrs_(num_dimensions, std::vector<uint64_t>(num_datapoints, 0)),
          limits_(num_dimensions, std::numeric_limits<size_t>::max()), num_datapoints_(num_datapoints), stamp_(next_stamp()) {}
    void set_limits(std::vector<size_t> limits) { limits_ = std::move(limits); }   // :143-145
    void set_attribute(size_t dim, DatapointIndex index, uint64_t attribute) {     // :148-155: out of range is ignored
        if (dim < attrs_.size() && (size_t)index < attrs_[dim].size()) {
            attrs_[dim][index] = attribute;
            stamp_ = next_stamp();
        }
    }
    std::vector<uint64_t> get_attributes(DatapointIndex index) const {             // :158-164: missing = 0
        std::vector<uint64_t> out;
        out.reserve(attrs_.size());
        for (const auto &d : attrs_) out.push_back((size_t)index < d.size() ? d[index] : 0);
        return out;
    }
    // The plain host walk (:167-200), statement for statement -- including that it tests `len >= k` only after a push.
    // The reference indexes limits[dim] and panics on a short vector; here that is InvalidArgument.
    NNResultsVector apply(const NNResultsVector &results, size_t k) const {
        const size_t num_dims = attrs_.size();
        if (limits_.size() < num_dims) throw ScannError::invalid_argument("fewer limits than crowding dimensions");
        std::vector<std::unordered_map<uint64_t, size_t>> crowd_counts(num_dims);
        NNResultsVector filtered;
        filtered.reserve(std::min(k, results.size()));
        for (const auto &r : results) {
            const std::vector<uint64_t> attrs = get_attributes(r.first);
            bool allowed = true;
            for (size_t dim = 0; dim < num_dims; ++dim) {
                auto it = crowd_counts[dim].find(attrs[dim]);
                const size_t count = it == crowd_counts[dim].end() ? 0 : it->second;
                if (count >= limits_[dim]) {
                    allowed = false;
                    break;
                }
            }
            if (allowed) {
                for (size_t dim = 0; dim < num_dims; ++dim) ++crowd_counts[dim][attrs[dim]];
                filtered.push_back(r);
                if (filtered.size() >= k) break;
            }
        }
        return filtered;
    }
    size_t num_dimensions() const { return attrs_.size(); }
    size_t num_datapoints() const { return num_datapoints_; }
    const std::vector<size_t> &limits() const { return limits_; }
    // [num_dimensions][num_datapoints], dimension-major: what scann_hip_index_set_crowding_attributes_md takes
    std::vector<uint64_t> flat_attributes() const {
        std::vector<uint64_t> flat;
        flat.reserve(attrs_.size() * num_datapoints_);
        for (const auto &d : attrs_) flat.insert(flat.end(), d.begin(), d.end());
        return flat;
    }
    uint64_t stamp() const { return stamp_; }

private:
    static uint64_t next_stamp() {
        static std::atomic<uint64_t> s{0};
        return ++s;
    }
    std::vector<std::vector<uint64_t>> attrs_;
    std::vector<size_t> limits_;
    size_t num_datapoints_;
    uint64_t stamp_;
};

struct MmrDiversifier {              // crowding.rs:203-268
    float lambda;
    explicit MmrDiversifier(float l) : lambda(l < 0.0f ? 0.0f : (l > 1.0f ? 1.0f : l)) {}   // f32::clamp (NaN stays NaN)
    // :220-267, statement for statement; similarity_fn(a, b) -> f32
    template <typename F>
    NNResultsVector apply(const NNResultsVector &candidates, size_t k, F similarity_fn) const {
        if (candidates.empty() || k == 0) return {};
        NNResultsVector selected, remaining(candidates);
        selected.reserve(std::min(k, candidates.size()));
        selected.push_back(remaining.front());
        remaining.erase(remaining.begin());
        const float f32_min = std::numeric_limits<float>::lowest();
        while (selected.size() < k && !remaining.empty()) {
            size_t best_idx = 0;
            float best_score = f32_min;
            for (size_t i = 0; i < remaining.size(); ++i) {
                const float rel_score = -remaining[i].second;
                float max_sim = f32_min;
                for (const auto &sel : selected) max_sim = std::fmax(max_sim, (float)similarity_fn(remaining[i].first, sel.first));
                // (volatile: each product is rounded to f32 before the subtraction, whatever the compiler's contraction)
                volatile float a = lambda * rel_score, b = (1.0f - lambda) * max_sim;
                const float mmr_score = a - b;
                if (mmr_score > best_score) {
                    best_score = mmr_score;
                    best_idx = i;
                }
            }
            selected.push_back(remaining[best_idx]);
            remaining.erase(remaining.begin() + (std::ptrdiff_t)best_idx);
        }
        return selected;
    }
};

namespace detail {

struct IndexHandle {
    scann_hip_index *h = nullptr;
    IndexHandle() = default;
    IndexHandle(const IndexHandle &) = delete;
    IndexHandle &operator=(const IndexHandle &) = delete;
    IndexHandle(IndexHandle &&o) noexcept : h(o.h) { o.h = nullptr; }
    ~IndexHandle() { if (h) scann_hip_index_destroy(h); }
};

inline std::vector<NNResultsVector> run_search(scann_hip_index *h, const float *q, uint32_t nq,
                                               uint32_t q_stride, uint32_t q_dim, uint32_t k,
                                               const scann_hip_search_opts *opts) {
    std::vector<uint32_t> idx((size_t)nq * std::max(1u, k)), cnt(nq);
    std::vector<float> dist((size_t)nq * std::max(1u, k));
    check(scann_hip_search_batched(h, q, nq, q_stride, q_dim, k, opts, idx.data(), dist.data(), cnt.data()));
    std::vector<NNResultsVector> out(nq);
    for (uint32_t i = 0; i < nq; ++i)
        for (uint32_t j = 0; j < cnt[i]; ++j) out[i].emplace_back(idx[(size_t)i * k + j], dist[(size_t)i * k + j]);
    return out;
}

// Searcher::search_batched_with_params (searcher.rs:148-186): one num_neighbors per query
inline std::vector<NNResultsVector> run_search_params(scann_hip_index *h, const float *q, uint32_t nq,
                                                      uint32_t q_stride, uint32_t q_dim, const std::vector<uint32_t> &ks,
                                                      const scann_hip_search_opts *opts) {
    uint32_t pitch = 1;
    for (uint32_t k : ks) pitch = std::max(pitch, k);
    std::vector<uint32_t> idx((size_t)nq * pitch), cnt(nq);
    std::vector<float> dist((size_t)nq * pitch);
    check(scann_hip_search_batched_params(h, q, nq, q_stride, q_dim, ks.data(), opts, pitch, idx.data(), dist.data(), cnt.data()));
    std::vector<NNResultsVector> out(nq);
    for (uint32_t i = 0; i < nq; ++i)
        for (uint32_t j = 0; j < cnt[i]; ++j) out[i].emplace_back(idx[(size_t)i * pitch + j], dist[(size_t)i * pitch + j]);
    return out;
}

// search_with_crowding of every searcher: the constraint's attributes are copied to the handle once (again only when
// they changed), then scann_hip_search_crowded = CrowdingConstraint::apply(search(query, depth), k) on the device.
struct CrowdAttach {
    mutable uint64_t stamp = 0;   // (attaching needs the external synchronisation of create / destroy)
    void ensure(scann_hip_index *h, const CrowdingConstraint &c) const {
        if (stamp == c.stamp()) return;
        // (an empty attribute vector still attaches: every datapoint then has attribute 0)
        static const uint64_t zero = 0;
        const auto &a = c.attributes();
        check(scann_hip_index_set_crowding_attributes(h, a.empty() ? &zero : a.data(), a.empty() ? 1 : a.size()));
        stamp = c.stamp();
    }
};

inline NNResultsVector run_search_crowded(scann_hip_index *h, const CrowdAttach &at, const std::vector<float> &query,
                                          size_t k, size_t depth, const CrowdingConstraint &c,
                                          const scann_hip_search_opts *opts) {
    at.ensure(h, c);
    const uint32_t limit = (uint32_t)std::min<size_t>(c.config().per_crowd_limit, 0xFFFFFFFFu);
    std::vector<uint32_t> idx(std::max<size_t>(1, k));
    std::vector<float> dist(std::max<size_t>(1, k));
    uint32_t cnt = 0;
    check(scann_hip_search_crowded(h, query.data(), 1, (uint32_t)query.size(), (uint32_t)query.size(), (uint32_t)k,
                                   (uint32_t)depth, limit, opts, idx.data(), dist.data(), &cnt));
    NNResultsVector out;
    for (uint32_t j = 0; j < cnt; ++j) out.emplace_back(idx[j], dist[j]);
    return out;
}

// search_with_crowding_md: the attributes go to the handle once per change of the constraint, then
// scann_hip_search_crowded_md = CrowdingMultidimensional::apply(search(query, depth), k) on the device.
struct CrowdMdAttach {
    mutable uint64_t stamp = 0;
    void ensure(scann_hip_index *h, const CrowdingMultidimensional &c) const {
        if (stamp == c.stamp()) return;
        const std::vector<uint64_t> flat = c.flat_attributes();
        check(scann_hip_index_set_crowding_attributes_md(h, flat.data(), (uint32_t)c.num_dimensions(), c.num_datapoints()));
        stamp = c.stamp();
    }
};

inline NNResultsVector run_search_crowded_md(scann_hip_index *h, const CrowdMdAttach &at, const std::vector<float> &query,
                                             size_t k, size_t depth, const CrowdingMultidimensional &c,
                                             const scann_hip_search_opts *opts) {
    at.ensure(h, c);
    std::vector<uint32_t> limits;
    for (size_t l : c.limits()) limits.push_back((uint32_t)std::min<size_t>(l, 0xFFFFFFFFu));
    std::vector<uint32_t> idx(std::max<size_t>(1, k));
    std::vector<float> dist(std::max<size_t>(1, k));
    uint32_t cnt = 0;
    check(scann_hip_search_crowded_md(h, query.data(), 1, (uint32_t)query.size(), (uint32_t)query.size(), (uint32_t)k,
                                      (uint32_t)depth, limits.data(), (uint32_t)limits.size(), opts, idx.data(),
                                      dist.data(), &cnt));
    NNResultsVector out;
    for (uint32_t j = 0; j < cnt; ++j) out.emplace_back(idx[j], dist[j]);
    return out;
}

// MmrDiversifier::apply(search(query, depth), k, sim) on the device, sim = minus the handle's distance of two rows
inline NNResultsVector run_search_mmr(scann_hip_index *h, const std::vector<float> &query, size_t k, size_t depth,
                                      const MmrDiversifier &mmr, const scann_hip_search_opts *opts) {
    std::vector<uint32_t> idx(std::max<size_t>(1, k));
    std::vector<float> dist(std::max<size_t>(1, k));
    uint32_t cnt = 0;
    check(scann_hip_search_mmr(h, query.data(), 1, (uint32_t)query.size(), (uint32_t)query.size(), (uint32_t)k,
                               (uint32_t)depth, mmr.lambda, opts, idx.data(), dist.data(), &cnt));
    NNResultsVector out;
    for (uint32_t j = 0; j < cnt; ++j) out.emplace_back(idx[j], dist[j]);
    return out;
}

inline std::vector<float> flatten(const std::vector<std::vector<float>> &qs, uint32_t *dim_out) {
    uint32_t d = qs.empty() ? 0 : (uint32_t)qs[0].size();
    for (auto &q : qs)
        if (q.size() != d) throw ScannError::invalid_argument("Query dimensionality mismatch");
    std::vector<float> flat((size_t)qs.size() * std::max(1u, d));
    for (size_t i = 0; i < qs.size(); ++i) std::memcpy(&flat[i * d], qs[i].data(), d * 4);
    *dim_out = d;
    return flat;
}

// One allow-bitmap per query for scann_hip_search_opts.allow_bitmap_stride: row i = filters[i]->to_bitmap(n), a null
// entry = every datapoint below n; rows are ceil(n / 64) words apart (*stride_words).
inline std::vector<uint64_t> materialise_filters(const std::vector<const RestrictFilter *> &filters, size_t n,
                                                 uint64_t *stride_words) {
    const size_t words = (n + 63) / 64;
    std::vector<uint64_t> block(filters.size() * words, 0);
    for (size_t i = 0; i < filters.size(); ++i) {
        uint64_t *row = block.data() + i * words;
        if (filters[i]) {
            const auto w = filters[i]->to_bitmap(n);
            std::copy(w.begin(), w.begin() + std::min(w.size(), words), row);
        } else {
            std::fill(row, row + words, ~0ull);
            if (n & 63) row[words - 1] = (1ull << (n & 63)) - 1;
        }
    }
    *stride_words = words;
    return block;
}

// search_with_filter for a batch: query i under filters[i] (null = no filter for that query), one call
inline std::vector<NNResultsVector> run_search_filters(scann_hip_index *h, const std::vector<std::vector<float>> &queries,
                                                       size_t k, const std::vector<const RestrictFilter *> &filters,
                                                       size_t n, scann_hip_search_opts o) {
    if (queries.size() != filters.size()) throw ScannError::invalid_argument("one filter (or null) per query");
    if (queries.empty()) return {};
    uint32_t d;
    const auto flat = flatten(queries, &d);
    uint64_t stride = 0;
    const auto block = materialise_filters(filters, n, &stride);
    const uint64_t none = 0;   // (n = 0: capacity 0, a non-null pointer no row reads)
    o.allow_bitmap = block.empty() ? &none : block.data();
    o.allow_bitmap_bits = n;
    o.allow_bitmap_stride = stride;
    return run_search(h, flat.data(), (uint32_t)queries.size(), d, d, (uint32_t)k, &o);
}

// search_with_filter(map.create_allowlist(token_lists[i])) for a batch: the block is built on the device from the
// resident map and searched on the same stream (scann_hip_search_batched_tokens)
inline std::vector<NNResultsVector> run_search_tokens(scann_hip_index *h, const std::vector<std::vector<float>> &queries,
                                                      size_t k, const std::vector<std::vector<uint64_t>> &token_lists,
                                                      const DeviceTokenMap &map, const scann_hip_search_opts &o) {
    if (queries.size() != token_lists.size()) throw ScannError::invalid_argument("one token list per query");
    if (!map.handle()) throw ScannError::failed_precondition("the token map is not on the device");
    if (queries.empty()) return {};
    uint32_t d;
    const auto flat = flatten(queries, &d);
    const uint32_t nq = (uint32_t)queries.size(), kk = (uint32_t)k;
    std::vector<uint64_t> tok, off(1, 0);
    for (const auto &l : token_lists) {
        tok.insert(tok.end(), l.begin(), l.end());
        off.push_back(tok.size());
    }
    std::vector<uint32_t> idx((size_t)nq * std::max(1u, kk)), cnt(nq);
    std::vector<float> dist((size_t)nq * std::max(1u, kk));
    check(scann_hip_search_batched_tokens(h, map.handle(), flat.data(), nq, d, d, kk, &o, tok.data(), off.data(), idx.data(),
                                          dist.data(), cnt.data()));
    std::vector<NNResultsVector> out(nq);
    for (uint32_t i = 0; i < nq; ++i)
        for (uint32_t j = 0; j < cnt[i]; ++j) out[i].emplace_back(idx[(size_t)i * kk + j], dist[(size_t)i * kk + j]);
    return out;
}

// query i under the conjunction of ranges bounds[i * cols.size() * 2 + c * 2 + {0, 1}] over the table's clause columns
// `cols`: the block is built on the device from the resident columns and searched on the same stream
// (scann_hip_search_batched_ranges)
inline std::vector<NNResultsVector> run_search_ranges(scann_hip_index *h, const std::vector<std::vector<float>> &queries,
                                                      size_t k, const std::vector<uint32_t> &cols,
                                                      const std::vector<scann_hip_range_bound> &bounds,
                                                      const AttributeTable &table, const scann_hip_search_opts &o) {
    if (bounds.size() != queries.size() * cols.size() * 2) throw ScannError::invalid_argument("two bounds per query and clause");
    if (!table.handle()) throw ScannError::failed_precondition("the attribute table is not on the device");
    if (queries.empty()) return {};
    uint32_t d;
    const auto flat = flatten(queries, &d);
    const uint32_t nq = (uint32_t)queries.size(), kk = (uint32_t)k;
    std::vector<uint32_t> idx((size_t)nq * std::max(1u, kk)), cnt(nq);
    std::vector<float> dist((size_t)nq * std::max(1u, kk));
    check(scann_hip_search_batched_ranges(h, table.handle(), flat.data(), nq, d, d, kk, &o, cols.data(), (uint32_t)cols.size(),
                                          bounds.data(), idx.data(), dist.data(), cnt.data()));
    std::vector<NNResultsVector> out(nq);
    for (uint32_t i = 0; i < nq; ++i)
        for (uint32_t j = 0; j < cnt[i]; ++j) out[i].emplace_back(idx[(size_t)i * kk + j], dist[(size_t)i * kk + j]);
    return out;
}

// splitmix64: the documented counter-based generator of this build (not rand::StdRng).
inline uint64_t splitmix(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// KMeans::fit (trees/kmeans.rs:166-263) on the GPU over the rows of the brute-force index `bf`,
// restricted to columns [c0, c0 + d): k-means++ seeding (scann_hip_kmeans_init_pp, splitmix64 stream)
// then the Lloyd loop of fit_single (scann_hip_kmeans_lloyd: assignment with the lowest index on ties
// -- sequential-scalar distances below KMeansConfig.simd_threshold dims, the AVX2 order from there
// on -- f64 centre update in datapoint order, the reference's convergence test).
constexpr uint32_t kKMeansSimdThreshold = 128;   // KMeansConfig::default (trees/kmeans.rs:59)
inline void kmeans_gpu(scann_hip_index *bf, size_t n, size_t c0, size_t d, size_t k, size_t max_iterations,
                       double convergence_threshold, uint64_t seed, std::vector<float> &centers,
                       std::vector<uint32_t> &assign) {
    k = std::min(k, n);   // kmeans.rs:171-175: at most n clusters
    centers.assign(k * d, 0.0f);
    assign.assign(n, 0);
    check(scann_hip_kmeans_init_pp(bf, (uint32_t)c0, (uint32_t)d, (uint32_t)k, seed, kKMeansSimdThreshold,
                                   centers.data()));
    check(scann_hip_kmeans_lloyd(bf, (uint32_t)c0, (uint32_t)d, centers.data(), (uint32_t)k,
                                 (uint32_t)max_iterations, convergence_threshold, kKMeansSimdThreshold,
                                 assign.data(), nullptr, nullptr, nullptr, nullptr));
}

// Codebook::train (hashes/codebook.rs:146-202): per-subspace k-means with seed + s, on the GPU over
// the column windows of `bf` (an index holding the training rows).
inline std::vector<float> train_codebook(scann_hip_index *bf, size_t n, uint32_t dim, uint32_t S, uint32_t K,
                                         uint64_t seed, size_t max_iterations, double convergence_threshold) {
    if (n == 0) throw ScannError::invalid_argument("Cannot train on empty dataset");
    if (dim % S != 0)   // codebook.rs:154-159
        throw ScannError::invalid_argument("Dimensionality " + std::to_string(dim) +
                                           " must be divisible by num_subspaces " + std::to_string(S));
    const uint32_t dsub = dim / S;
    std::vector<float> cb((size_t)S * K * dsub, 0.0f), centers;
    std::vector<uint32_t> assign;
    for (uint32_t s = 0; s < S; ++s) {
        kmeans_gpu(bf, n, (size_t)s * dsub, dsub, K, max_iterations, convergence_threshold, seed + s, centers,
                   assign);
        const size_t got = centers.size() / dsub;
        for (uint32_t c = 0; c < K; ++c)
            std::memcpy(&cb[((size_t)s * K + c) * dsub], &centers[std::min<size_t>(c, got - 1) * dsub], dsub * 4);
    }
    return cb;
}

// TreePartitioner::build (tree_partitioner.rs:48-98): flat k-means with seed 42 on the GPU, then the
// CSR leaf lists (ascending datapoint index inside each leaf, :84-89).
inline void build_partition(const DenseDataset &ds, size_t num_partitions, size_t iterations, int device,
                            std::vector<float> &centers, std::vector<uint32_t> &leaf_off,
                            std::vector<uint32_t> &leaf_ids);

}  // namespace detail

// ---- BruteForceSearcher (brute_force/searcher.rs:18-208) --------------------------------
class BruteForceSearcher {
public:
    BruteForceSearcher(std::shared_ptr<DenseDataset> dataset, DistanceMeasure measure, int device = 0)
        : dataset_(std::move(dataset)), measure_(measure) {
        check(scann_hip_bf_create(context(device), dataset_->raw_data(), dataset_->size(),
                                  dataset_->dimensionality(), dataset_->stride(), (int)measure, &ix_.h));
    }
    BruteForceSearcher(DenseDataset dataset, DistanceMeasure measure, int device = 0)
        : BruteForceSearcher(std::make_shared<DenseDataset>(std::move(dataset)), measure, device) {}

    NNResultsVector search(const std::vector<float> &query, size_t k) const {   // :77-93
        return detail::run_search(ix_.h, query.data(), 1, (uint32_t)query.size(), (uint32_t)query.size(),
                                  (uint32_t)k, nullptr)[0];
    }
    std::vector<NNResultsVector> search_batched(const std::vector<std::vector<float>> &queries, size_t k) const {
        if (queries.empty()) return {};                                          // :175-177
        uint32_t d;
        auto flat = detail::flatten(queries, &d);
        return detail::run_search(ix_.h, flat.data(), (uint32_t)queries.size(), d, d, (uint32_t)k, nullptr);
    }
    // The reference's BruteForceSearcher takes no filter; the contract (include/scann_hip.h, allow_bitmap) is the
    // search over the allowed rows alone, as TreeXHybridSearcher::search_with_filter skips disallowed points before
    // scoring (tree_x_hybrid/mod.rs:327-332).  The filter is materialised once into an allow-bitmap.
    NNResultsVector search_with_filter(const std::vector<float> &query, size_t k, const RestrictFilter *filter) const {
        if (!filter) return search(query, k);
        const auto bits = filter->to_bitmap(dataset_size());
        scann_hip_search_opts o;
        scann_hip_search_opts_default(&o);
        o.allow_bitmap = bits.data();
        o.allow_bitmap_bits = bits.size() * 64;
        return detail::run_search(ix_.h, query.data(), 1, (uint32_t)query.size(), (uint32_t)query.size(),
                                  (uint32_t)k, &o)[0];
    }
    // CrowdingConstraint::apply(search(query, depth), k) on the device; a disabled constraint is the plain search.
    NNResultsVector search_with_crowding(const std::vector<float> &query, size_t k, size_t depth,
                                         const CrowdingConstraint &constraint) const {
        if (!constraint.config().enabled) return search(query, k);
        return detail::run_search_crowded(ix_.h, crowd_, query, k, depth, constraint, nullptr);
    }
    // CrowdingMultidimensional::apply(search(query, depth), k) on the device
    NNResultsVector search_with_crowding_md(const std::vector<float> &query, size_t k, size_t depth,
                                            const CrowdingMultidimensional &constraint) const {
        return detail::run_search_crowded_md(ix_.h, crowd_md_, query, k, depth, constraint, nullptr);
    }
    // MmrDiversifier::apply(search(query, depth), k, sim) on the device; sim(a, b) = -distance(row a, row b) under the
    // searcher's measure.  Rows come back in selection order.
    NNResultsVector search_with_mmr(const std::vector<float> &query, size_t k, size_t depth,
                                    const MmrDiversifier &mmr) const {
        return detail::run_search_mmr(ix_.h, query, k, depth, mmr, nullptr);
    }
    // The crowded k nearest neighbours over the WHOLE index: depth starts at k and doubles until the row holds k
    // entries or depth has reached min(N, 2048).  second = complete: k were kept, or the whole index was walked; by
    // the prefix property the rows then equal apply() over the full sorted database.
    std::pair<NNResultsVector, bool> search_crowded_exact(const std::vector<float> &query, size_t k,
                                                          const CrowdingConstraint &constraint) const {
        const size_t n = dataset_size(), cap = std::min<size_t>(n, 2048);
        if (!constraint.config().enabled) return {search(query, k), true};
        size_t depth = std::max<size_t>(1, std::min(k, cap));
        for (;;) {
            NNResultsVector r = search_with_crowding(query, std::min(k, depth), depth, constraint);
            if (r.size() >= k || depth >= cap) {
                const bool complete = r.size() >= k || depth >= n;
                return {std::move(r), complete};
            }
            depth = std::min(2 * depth, cap);
        }
    }
    NNResultsVector search_radius(const std::vector<float> &query, float radius) const {   // :142-167
        return search_radius_with_filter(query, radius, nullptr);
    }
    // every ALLOWED datapoint with distance <= radius
    NNResultsVector search_radius_with_filter(const std::vector<float> &query, float radius,
                                              const RestrictFilter *filter) const {
        if (dataset_size() == 0) return {};
        std::vector<uint64_t> bits;
        scann_hip_search_opts o;
        scann_hip_search_opts_default(&o);
        if (filter) {
            bits = filter->to_bitmap(dataset_size());
            o.allow_bitmap = bits.data();
            o.allow_bitmap_bits = bits.size() * 64;
        }
        std::vector<uint32_t> idx(256);
        std::vector<float> dist(256);
        uint64_t found = 0;
        for (;;) {
            check(scann_hip_bf_search_radius_opts(ix_.h, query.data(), (uint32_t)query.size(), radius,
                                                  filter ? &o : nullptr, idx.data(), dist.data(), idx.size(), &found));
            if (found <= idx.size()) break;
            idx.resize(found);
            dist.resize(found);
        }
        NNResultsVector r(found);
        for (size_t i = 0; i < found; ++i) r[i] = {idx[i], dist[i]};
        return r;
    }
    size_t dataset_size() const { return (size_t)scann_hip_index_size(ix_.h); }
    uint64_t dimensionality() const { return scann_hip_index_dimensionality(ix_.h); }
    DistanceMeasure distance_measure() const { return measure_; }
    // the host rows the searcher was built from; EMPTY for a base made on the device by MutableIndex::compact (its rows
    // never visited the host: MutableIndex::export_live reads them back)
    const DenseDataset &dataset() const { return *dataset_; }
    scann_hip_index *handle() const { return ix_.h; }   // (borrowed by MutableIndex)

private:
    friend class MutableIndex;
    // adopts a handle scann_hip_fold_mutable made
    BruteForceSearcher(scann_hip_index *adopted, DistanceMeasure measure)
        : dataset_(std::make_shared<DenseDataset>()), measure_(measure) {
        ix_.h = adopted;
    }
    std::shared_ptr<DenseDataset> dataset_;
    DistanceMeasure measure_;
    detail::IndexHandle ix_;
    detail::CrowdAttach crowd_;
    detail::CrowdMdAttach crowd_md_;
};

// ---- scalar quantizer (quantization/mod.rs:62-145, quantization/scalar.rs:10-177) ----------------------------
struct QuantizationStats {
    float min_value = 0.0f, max_value = 0.0f, mean = 0.0f, std_dev = 0.0f;
    // the reference's sequential f64 sums over the logical values, on the host
    static QuantizationStats from_dataset(const DenseDataset &ds) {
        float mn = std::numeric_limits<float>::max(), mx = std::numeric_limits<float>::lowest();
        double sum = 0.0, sum_sq = 0.0;
        uint64_t count = 0;
        for (size_t i = 0; i < ds.size(); ++i)
            for (uint32_t j = 0; j < ds.dimensionality(); ++j) {
                const float v = ds.get(i)[j];
                mn = std::fmin(mn, v);
                mx = std::fmax(mx, v);
                sum += (double)v;
                sum_sq += (double)v * (double)v;
                ++count;
            }
        QuantizationStats s;
        s.min_value = mn;
        s.max_value = mx;
        s.mean = count ? (float)(sum / (double)count) : 0.0f;
        const float var = count > 1 ? (float)((sum_sq - sum * sum / (double)count) / (double)(count - 1)) : 0.0f;
        s.std_dev = std::sqrt(var);
        return s;
    }
    static QuantizationStats from_vecs(const std::vector<std::vector<float>> &data) {
        return from_dataset(DenseDataset::from_vecs(data));
    }
    // the same statistics of the f32 rows resident in a handle, reduced on the device (scann_hip_index_quantization_stats)
    static QuantizationStats from_index(scann_hip_index *h) {
        float st[4];
        check(scann_hip_index_quantization_stats(h, st));
        QuantizationStats s;
        s.min_value = st[0]; s.max_value = st[1]; s.mean = st[2]; s.std_dev = st[3];
        return s;
    }
};

struct ScalarQuantizerConfig {       // scalar.rs:10-67
    size_t bits = 8;
    bool has_range = false;          // min_value / max_value: Some
    float min_value = 0.0f, max_value = 0.0f;
    bool is_symmetric = false;
    float num_std_devs = 3.0f;
    static ScalarQuantizerConfig int8() { return ScalarQuantizerConfig{}; }
    static ScalarQuantizerConfig int4() {
        ScalarQuantizerConfig c;
        c.bits = 4;
        return c;
    }
    ScalarQuantizerConfig with_range(float mn, float mx) const {
        ScalarQuantizerConfig c = *this;
        c.has_range = true;
        c.min_value = mn;
        c.max_value = mx;
        return c;
    }
    ScalarQuantizerConfig symmetric() const {
        ScalarQuantizerConfig c = *this;
        c.is_symmetric = true;
        return c;
    }
    // mode and (a, b) of the C entry points: an explicit range wins over symmetric, as in calibrate()
    int mode() const { return has_range ? SCANN_HIP_SQ_RANGE : (is_symmetric ? SCANN_HIP_SQ_SYMMETRIC : SCANN_HIP_SQ_STDDEV); }
    float a() const { return has_range ? min_value : num_std_devs; }
    float b() const { return has_range ? max_value : 0.0f; }
};

class ScalarQuantizer {              // scalar.rs:69-177, through the library's stateless host functions
public:
    explicit ScalarQuantizer(ScalarQuantizerConfig config = ScalarQuantizerConfig{}) : config_(config) {}
    void calibrate(const QuantizationStats &stats) {
        const float st[4] = {stats.min_value, stats.max_value, stats.mean, stats.std_dev};
        check(scann_hip_scalar_quantizer_calibrate(st, (uint32_t)config_.bits, config_.mode(), config_.a(), config_.b(),
                                                   params_, &zero_point_));
    }
    void calibrate_from_dataset(const DenseDataset &ds) { calibrate(QuantizationStats::from_dataset(ds)); }
    // adopts what scann_hip_index_quantize_rows calibrated on the device
    void set_params(const float *params4, int32_t zero_point) {
        std::memcpy(params_, params4, sizeof(params_));
        zero_point_ = zero_point;
    }
    float scale() const { return params_[2]; }
    int32_t zero_point() const { return zero_point_; }
    float min_value() const { return params_[0]; }
    float max_value() const { return params_[1]; }
    size_t bits() const { return config_.bits; }
    const ScalarQuantizerConfig &config() const { return config_; }
    int8_t quantize_value(float value) const { return quantize({value})[0]; }
    float dequantize_value(int8_t q) const { return dequantize({q})[0]; }
    std::vector<int8_t> quantize(const std::vector<float> &values) const {
        std::vector<int8_t> out(values.size());
        check(scann_hip_scalar_quantize(values.data(), values.size(), (uint32_t)config_.bits, config_.mode(), params_,
                                        out.data()));
        return out;
    }
    std::vector<float> dequantize(const std::vector<int8_t> &codes) const {
        std::vector<float> out(codes.size());
        check(scann_hip_scalar_dequantize(codes.data(), codes.size(), config_.mode(), params_, out.data()));
        return out;
    }

private:
    ScalarQuantizerConfig config_;
    float params_[4] = {0.0f, 1.0f, 1.0f, 1.0f};   // ScalarQuantizer::new: min 0, max 1, scale 1, inv_scale 1
    int32_t zero_point_ = 0;
};

class QuantizedDataset {             // scalar.rs:179-300: stride == dimensionality, codes on the host
public:
    static QuantizedDataset from_dataset(const DenseDataset &ds, ScalarQuantizer quantizer) {
        if (ds.is_empty()) throw ScannError::invalid_argument("Cannot quantize empty dataset");
        quantizer.calibrate_from_dataset(ds);
        QuantizedDataset q(std::move(quantizer));
        q.n_ = ds.size();
        q.dim_ = ds.dimensionality();
        std::vector<float> flat(q.n_ * q.dim_);
        for (size_t i = 0; i < q.n_; ++i) std::memcpy(&flat[i * q.dim_], ds.get(i), q.dim_ * 4);
        q.data_ = q.quantizer_.quantize(flat);
        return q;
    }
    size_t size() const { return n_; }
    size_t dimensionality() const { return dim_; }
    const std::vector<int8_t> &raw_data() const { return data_; }
    const ScalarQuantizer &quantizer() const { return quantizer_; }
    std::vector<float> get_dequantized(DatapointIndex i) const {
        return quantizer_.dequantize(std::vector<int8_t>(data_.begin() + (size_t)i * dim_, data_.begin() + ((size_t)i + 1) * dim_));
    }

private:
    explicit QuantizedDataset(ScalarQuantizer q) : quantizer_(std::move(q)) {}
    std::vector<int8_t> data_;
    size_t n_ = 0, dim_ = 0;
    ScalarQuantizer quantizer_;
};

// ---- ScalarQuantizedBruteForceSearcher (brute_force/scalar_quantized.rs:24-348) --------------------------------
struct ScalarQuantizedConfig {
    ScalarQuantizerConfig quantizer_config;
    DistanceMeasure distance_measure = DistanceMeasure::SquaredL2;
    bool parallel = true;                    // (the device runs every batch at once: kept for the signature)
    size_t parallel_batch_threshold = 100;
    static ScalarQuantizedConfig squared_l2() { return ScalarQuantizedConfig{}; }
    static ScalarQuantizedConfig dot_product() { return ScalarQuantizedConfig{}.with_distance(DistanceMeasure::DotProduct); }
    ScalarQuantizedConfig with_distance(DistanceMeasure d) const {
        ScalarQuantizedConfig c = *this;
        c.distance_measure = d;
        return c;
    }
    ScalarQuantizedConfig with_parallel(bool p) const {
        ScalarQuantizedConfig c = *this;
        c.parallel = p;
        return c;
    }
};

// The reference reads the quantizer's offset-binary bytes as SIGNED and ignores min_value (:198-225); so does the
// library (include/scann_hip.h "scalar quantizer"), and so does this class.
class ScalarQuantizedBruteForceSearcher {
public:
    // new(&dataset, config): the f32 rows are uploaded once, quantized ON THE DEVICE (scann_hip_index_quantize_rows:
    // stats, calibrate, quantize) and the f32 handle is released.
    static ScalarQuantizedBruteForceSearcher create(const DenseDataset &dataset, ScalarQuantizedConfig config, int device = 0) {
        if (dataset.is_empty()) throw ScannError::invalid_argument("Cannot quantize empty dataset");
        detail::IndexHandle f32;
        check(scann_hip_bf_create(context(device), dataset.raw_data(), dataset.size(), dataset.dimensionality(),
                                  dataset.stride(), (int)config.distance_measure, &f32.h));
        ScalarQuantizedBruteForceSearcher s(config.distance_measure, ScalarQuantizer(config.quantizer_config));
        const ScalarQuantizerConfig &qc = config.quantizer_config;
        float params[4];
        int32_t zp = 0;
        check(scann_hip_index_quantize_rows(f32.h, SCANN_HIP_ROWS_INT8, (uint32_t)qc.bits, qc.mode(), qc.a(), qc.b(),
                                            &s.ix_.h, params, &zp));
        s.quantizer_.set_params(params, zp);
        s.n_ = dataset.size();
        s.dim_ = dataset.dimensionality();
        s.stride_ = dataset.stride();
        return s;
    }
    static ScalarQuantizedBruteForceSearcher from_quantized(const QuantizedDataset &q, DistanceMeasure measure, int device = 0) {
        ScalarQuantizedBruteForceSearcher s(measure, q.quantizer());
        check(scann_hip_bf_create_quantized(context(device), q.raw_data().data(), q.size(), (uint32_t)q.dimensionality(),
                                            (uint32_t)q.dimensionality(), SCANN_HIP_ROWS_INT8, q.quantizer().scale(),
                                            (int)measure, &s.ix_.h));
        s.n_ = q.size();
        s.dim_ = s.stride_ = q.dimensionality();
        return s;
    }
    NNResultsVector search(const std::vector<float> &query, size_t k) const {   // :168-184
        if (n_ == 0) return {};
        if (query.size() != dim_)
            throw ScannError::invalid_argument("Query dimensionality " + std::to_string(query.size()) +
                                               " does not match dataset dimensionality " + std::to_string(dim_));
        return detail::run_search(ix_.h, query.data(), 1, (uint32_t)query.size(), (uint32_t)query.size(), (uint32_t)k,
                                  nullptr)[0];
    }
    std::vector<NNResultsVector> search_batched(const std::vector<std::vector<float>> &queries, size_t k) const {
        if (queries.empty()) return {};                                          // :293-295
        uint32_t d;
        auto flat = detail::flatten(queries, &d);
        return detail::run_search(ix_.h, flat.data(), (uint32_t)queries.size(), d, d, (uint32_t)k, nullptr);
    }
    NNResultsVector search_radius(const std::vector<float> &query, float radius) const {   // :260-285
        if (n_ == 0) return {};
        if (query.size() != dim_) throw ScannError::invalid_argument("Query dimensionality does not match dataset");
        std::vector<uint32_t> idx(256);
        std::vector<float> dist(256);
        uint64_t found = 0;
        for (;;) {
            check(scann_hip_bf_search_radius(ix_.h, query.data(), (uint32_t)query.size(), radius, idx.data(), dist.data(),
                                             idx.size(), &found));
            if (found <= idx.size()) break;
            idx.resize(found);
            dist.resize(found);
        }
        NNResultsVector r(found);
        for (size_t i = 0; i < found; ++i) r[i] = {idx[i], dist[i]};
        return r;
    }
    // bytes the handle keeps on the device: the rows at their stride, plus a squared norm per row where the index
    // qualifies for the shortlist (the reference counts codes + norms, :329-333)
    size_t memory_usage() const { return (size_t)scann_hip_index_device_bytes(ix_.h); }
    float compression_ratio() const {                                            // :336-347
        const size_t quantized = n_ * stride_;
        return quantized ? (float)(n_ * dim_ * sizeof(float)) / (float)quantized : 0.0f;
    }
    const ScalarQuantizer &quantizer() const { return quantizer_; }
    DistanceMeasure distance_measure() const { return measure_; }
    size_t dataset_size() const { return n_; }
    uint64_t dimensionality() const { return dim_; }
    scann_hip_index *handle() const { return ix_.h; }

private:
    ScalarQuantizedBruteForceSearcher(DistanceMeasure m, ScalarQuantizer q) : measure_(m), quantizer_(std::move(q)) {}
    DistanceMeasure measure_;
    ScalarQuantizer quantizer_;
    detail::IndexHandle ix_;
    size_t n_ = 0, dim_ = 0, stride_ = 0;
};

// ---- MutableIndex: MutableDataset (mutator/mod.rs:233-490) over a live brute-force index -------------
// add / remove / update / get / exists / size / compact as MutableDataset names them, plus the rebuild counter of
// IncrementalUpdater (:527-545).  Rows live on the device: an immutable base searcher, a live bitmap over its rows and a
// delta segment of `capacity` rows (include/scann_hip.h "mutable indexes").  Ids are stable and never reused; search
// returns them.  compact() folds the live rows into a new base on the device and rebases onto it: the delta is empty again and
// removed ids are forgotten (NotFound), as after the reference's compact().  Brute-force bases only: the C ABI also takes
// Tree-X-Hybrid and flat-hasher bases (scann_hip_mutable_create over their handles), which this mirror does not wrap.
class MutableIndex {
public:
    MutableIndex(std::shared_ptr<BruteForceSearcher> base, size_t capacity, int device = 0)
        : base_(std::move(base)), device_(device) {
        check(scann_hip_mutable_create(context(device), base_->handle(), (uint32_t)std::min<size_t>(capacity, 0xFFFFFFFFu), &h_));
    }
    MutableIndex(const MutableIndex &) = delete;
    MutableIndex &operator=(const MutableIndex &) = delete;
    ~MutableIndex() { if (h_) scann_hip_mutable_destroy(h_); }   // (before base_: the handle borrows it)

    DatapointIndex add(const std::vector<float> &data) {                       // :286-317
        DatapointIndex id = 0;
        check(scann_hip_mutable_add(h_, data.data(), 1, (uint32_t)data.size(), (uint32_t)data.size(), &id));
        return id;
    }
    std::vector<DatapointIndex> add_batch(const std::vector<std::vector<float>> &rows) {
        if (rows.empty()) return {};
        uint32_t d;
        auto flat = detail::flatten(rows, &d);
        std::vector<DatapointIndex> ids(rows.size());
        check(scann_hip_mutable_add(h_, flat.data(), (uint32_t)rows.size(), d, d, ids.data()));
        return ids;
    }
    void remove(DatapointIndex index) { check(scann_hip_mutable_remove(h_, &index, 1)); }            // :320-330
    void remove_batch(const std::vector<DatapointIndex> &ids) {
        check(scann_hip_mutable_remove(h_, ids.data(), (uint32_t)ids.size()));
    }
    void update(DatapointIndex index, const std::vector<float> &data) {                             // :333-364
        check(scann_hip_mutable_update(h_, &index, data.data(), 1, (uint32_t)data.size(), (uint32_t)data.size()));
    }
    void update_batch(const std::vector<DatapointIndex> &ids, const std::vector<std::vector<float>> &rows) {
        if (ids.size() != rows.size()) throw ScannError::invalid_argument("update_batch: ids and rows differ in length");
        if (rows.empty()) return;
        uint32_t d;
        auto flat = detail::flatten(rows, &d);
        check(scann_hip_mutable_update(h_, ids.data(), flat.data(), (uint32_t)ids.size(), d, d));
    }
    // Option<Vec<f32>> (:367-375): false = None
    bool get(DatapointIndex index, std::vector<float> *out) const {
        std::vector<float> row(base_->dimensionality());
        const int s = scann_hip_mutable_get(h_, index, row.data());
        if (s == SCANN_HIP_NOT_FOUND) return false;
        check(s);
        if (out) *out = std::move(row);
        return true;
    }
    bool exists(DatapointIndex index) const { return scann_hip_mutable_exists(h_, index) != 0; }
    size_t size() const { return (size_t)scann_hip_mutable_size(h_); }
    uint64_t dimensionality() const { return base_->dimensionality(); }
    size_t pending() const { return (size_t)scann_hip_mutable_pending(h_); }
    bool needs_rebuild(size_t threshold) const { return scann_hip_mutable_needs_rebuild(h_, threshold) != 0; }   // :527-545

    // `filter` is asked about EXTERNAL ids below `filter_capacity` (ids at or past it are not allowed)
    NNResultsVector search(const std::vector<float> &query, size_t k, const RestrictFilter *filter = nullptr,
                           size_t filter_capacity = 0) const {
        return search_batched({query}, k, filter, filter_capacity)[0];
    }
    std::vector<NNResultsVector> search_batched(const std::vector<std::vector<float>> &queries, size_t k,
                                                const RestrictFilter *filter = nullptr, size_t filter_capacity = 0) const {
        if (queries.empty()) return {};
        uint32_t d;
        auto flat = detail::flatten(queries, &d);
        const uint32_t nq = (uint32_t)queries.size(), kk = (uint32_t)k;
        scann_hip_search_opts o;
        scann_hip_search_opts_default(&o);
        std::vector<uint64_t> bits;
        if (filter) {
            bits = filter->to_bitmap(filter_capacity);
            if (bits.empty()) bits.push_back(0);
            o.allow_bitmap = bits.data();
            o.allow_bitmap_bits = filter_capacity;
        }
        std::vector<uint32_t> idx((size_t)nq * std::max(1u, kk)), cnt(nq);
        std::vector<float> dist((size_t)nq * std::max(1u, kk));
        check(scann_hip_mutable_search(h_, flat.data(), nq, d, d, kk, &o, idx.data(), dist.data(), cnt.data()));
        std::vector<NNResultsVector> out(nq);
        for (uint32_t i = 0; i < nq; ++i)
            for (uint32_t j = 0; j < cnt[i]; ++j) out[i].emplace_back(idx[(size_t)i * kk + j], dist[(size_t)i * kk + j]);
        return out;
    }

    // every live row and its id, ascending by id
    std::pair<DenseDataset, std::vector<DatapointIndex>> export_live() const {
        const size_t n = size();
        const uint32_t dim = (uint32_t)base_->dimensionality(), stride = scann_hip_compute_stride(dim);
        std::vector<float> rows(std::max<size_t>(n, 1) * stride);
        std::vector<DatapointIndex> ids(std::max<size_t>(n, 1));
        uint64_t got = 0;
        check(scann_hip_mutable_export_live(h_, rows.data(), ids.data(), std::max<size_t>(n, 1), &got));
        ids.resize(got);
        std::vector<float> flat(got * dim);
        for (size_t i = 0; i < got; ++i) std::memcpy(&flat[i * dim], &rows[i * stride], (size_t)dim * 4);
        return {got ? DenseDataset::from_flat(flat, dim) : DenseDataset(), std::move(ids)};
    }
    // new_base's row j has external id base_ids[j] (strictly ascending); nullptr = identity
    void rebase(std::shared_ptr<BruteForceSearcher> new_base, const std::vector<DatapointIndex> *base_ids) {
        check(scann_hip_mutable_rebase(h_, new_base->handle(), base_ids ? base_ids->data() : nullptr, new_base->dataset_size()));
        base_ = std::move(new_base);   // (the old base is destroyed after the swap)
    }
    // MutableDataset::compact (:440-471) in one call and on the device (scann_hip_fold_mutable): the live rows become the
    // new base without visiting the host, the delta is emptied, removed ids are forgotten.  Returns the external id of
    // every row of the new base.  The new base has no host copy of its rows (base().dataset() is empty).
    std::vector<DatapointIndex> compact() {
        const size_t n = size();
        if (n == 0) throw ScannError::failed_precondition("compact: no live rows to build a base from");
        std::vector<DatapointIndex> ids(n);
        scann_hip_index *nb = nullptr;
        uint64_t got = 0;
        check(scann_hip_fold_mutable(h_, &nb, ids.data(), ids.size(), &got));
        ids.resize(got);
        base_ = std::shared_ptr<BruteForceSearcher>(new BruteForceSearcher(nb, base_->distance_measure()));   // (the old base is destroyed after the swap)
        return ids;
    }
    const BruteForceSearcher &base() const { return *base_; }

private:
    std::shared_ptr<BruteForceSearcher> base_;
    int device_;
    scann_hip_mutable *h_ = nullptr;
};

// ---- projections (projection/: pca.rs, random.rs, opq.rs, truncate.rs) ---------------------------------------------------
// The arrays of a trained projection (the reference's eigen-solver and RNG are not reproducible here, SURVEY F2, F4,
// F10: the arrays are the caller's, or PCA's from Projection::train_pca_on_device by the library's own rule).  matrix is [out_dim][in_dim]: column j of the reference's column-major DMatrix
// is row j.  project() is the reference's loop verbatim; to_device() makes the scann_hip_projection whose kernel gives
// the same bits (scann_hip.h "projections").
enum class ProjectionKind : int { Matrix = SCANN_HIP_PROJ_MATRIX, Pca = SCANN_HIP_PROJ_PCA, Truncate = SCANN_HIP_PROJ_TRUNCATE };

class DeviceProjection {
public:
    DeviceProjection() = default;
    explicit DeviceProjection(scann_hip_projection *h) : h_(h) {}
    DeviceProjection(const DeviceProjection &) = delete;
    DeviceProjection &operator=(const DeviceProjection &) = delete;
    DeviceProjection(DeviceProjection &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    ~DeviceProjection() { if (h_) scann_hip_projection_destroy(h_); }
    scann_hip_projection *handle() const { return h_; }
    // n rows of in_dim floats (row_stride apart) -> n rows of out_dim floats, on the device
    std::vector<float> project(const float *rows, size_t n, uint32_t row_stride, uint32_t row_dim) const {
        uint32_t info[4];
        check(scann_hip_projection_info(h_, info));
        std::vector<float> out(n * info[2]);
        check(scann_hip_project(h_, rows, n, row_stride, row_dim, out.data(), info[2]));
        return out;
    }
private:
    scann_hip_projection *h_ = nullptr;
};

class Projection {
public:
    // RandomOrthogonalProjection / GaussianRandomProjection / OpqProjection: no mean
    static Projection matrix(size_t in_dim, size_t out_dim, std::vector<float> m) {
        return Projection(ProjectionKind::Matrix, in_dim, out_dim, 0, std::move(m), {});
    }
    // a trained PcaProjection: components and mean
    static Projection pca(size_t in_dim, size_t out_dim, std::vector<float> components, std::vector<float> mean) {
        return Projection(ProjectionKind::Pca, in_dim, out_dim, 0, std::move(components), std::move(mean));
    }
    // TruncateProjection, and a PcaProjection before train(): out = in[start .. start + out_dim)
    static Projection truncate(size_t in_dim, size_t out_dim, size_t start = 0) {
        return Projection(ProjectionKind::Truncate, in_dim, out_dim, start, {}, {});
    }
    ProjectionKind kind() const { return kind_; }
    size_t input_dim() const { return in_dim_; }
    size_t output_dim() const { return out_dim_; }
    size_t start() const { return start_; }
    const std::vector<float> &matrix_rows() const { return matrix_; }
    const std::vector<float> &mean() const { return mean_; }

    // pca.rs:156-180, random.rs:82-92, opq.rs:179-194: out[j] = 0; for i ascending: out[j] += (in[i] - mean[i]) * M[(i, j)].
    // The product and the sum are separate f32 operations (volatile: no compiler may contract them).
    void project(const float *in, float *out) const {
        if (kind_ == ProjectionKind::Truncate) {
            for (size_t j = 0; j < out_dim_; ++j) out[j] = in[start_ + j];
            return;
        }
        for (size_t j = 0; j < out_dim_; ++j) {
            const float *m = matrix_.data() + j * in_dim_;
            float acc = 0.0f;
            for (size_t i = 0; i < in_dim_; ++i) {
                const float x = kind_ == ProjectionKind::Pca ? in[i] - mean_[i] : in[i];
                volatile float p = x * m[i];
                acc = acc + p;
            }
            out[j] = acc;
        }
    }
    std::vector<float> project(const std::vector<float> &in) const {
        if (in.size() != in_dim_)
            throw ScannError::invalid_argument("Input dimension " + std::to_string(in.size()) + " does not match " +
                                               std::to_string(in_dim_));
        std::vector<float> out(out_dim_);
        project(in.data(), out.data());
        return out;
    }
    DenseDataset project_dataset(const DenseDataset &ds) const {
        if (ds.dimensionality() != in_dim_) throw ScannError::invalid_argument("Dataset dimensionality does not match the projection");
        std::vector<float> flat(ds.size() * out_dim_);
        for (size_t i = 0; i < ds.size(); ++i) project(ds.get((DatapointIndex)i), flat.data() + i * out_dim_);
        return DenseDataset::from_flat(flat, out_dim_);
    }
    // PcaProjection::train on the device (scann_hip_pca_train: the rule is in scann_hip.h) from the resident rows of a
    // brute-force searcher; max_samples 0 = every row (the reference's default is 100 000).  Returns the device object;
    // from_device() reads its arrays back into a Projection.
    static DeviceProjection train_pca_on_device(const BruteForceSearcher &source, size_t out_dim, uint64_t max_samples = 0,
                                                uint64_t seed = 42, uint32_t *sweeps = nullptr, bool *converged = nullptr,
                                                std::vector<double> *eigenvalues = nullptr) {
        scann_hip_projection *h = nullptr;
        int conv = 0;
        uint32_t sw = 0;
        if (eigenvalues) eigenvalues->assign(source.dimensionality(), 0.0);
        check(scann_hip_pca_train(source.handle(), (uint32_t)out_dim, max_samples, seed, &h,
                                  eigenvalues ? eigenvalues->data() : nullptr, nullptr, &sw, &conv));
        if (sweeps) *sweeps = sw;
        if (converged) *converged = conv != 0;
        return DeviceProjection(h);
    }
    static Projection from_device(const DeviceProjection &p) {
        uint32_t info[4];
        check(scann_hip_projection_info(p.handle(), info));
        const ProjectionKind kind = (ProjectionKind)info[0];
        std::vector<float> m(kind == ProjectionKind::Truncate ? 0 : (size_t)info[1] * info[2]);
        std::vector<float> mean(kind == ProjectionKind::Pca ? info[1] : 0);
        check(scann_hip_projection_arrays(p.handle(), m.empty() ? nullptr : m.data(), mean.empty() ? nullptr : mean.data()));
        return Projection(kind, info[1], info[2], info[3], std::move(m), std::move(mean));
    }
    DeviceProjection to_device(int device = 0) const {
        scann_hip_projection *h = nullptr;
        check(scann_hip_projection_create(context(device), (int)kind_, (uint32_t)in_dim_, (uint32_t)out_dim_,
                                          matrix_.empty() ? nullptr : matrix_.data(), mean_.empty() ? nullptr : mean_.data(),
                                          (uint32_t)start_, &h));
        return DeviceProjection(h);
    }

private:
    Projection(ProjectionKind kind, size_t in_dim, size_t out_dim, size_t start, std::vector<float> m, std::vector<float> mean)
        : kind_(kind), in_dim_(in_dim), out_dim_(out_dim), start_(start), matrix_(std::move(m)), mean_(std::move(mean)) {
        if (in_dim == 0 || out_dim == 0) throw ScannError::invalid_argument("projection: in_dim and out_dim must be > 0");
        if (kind == ProjectionKind::Truncate) {
            if (start + out_dim > in_dim) throw ScannError::invalid_argument("projection: start + out_dim exceeds in_dim");
        } else {
            if (matrix_.size() != in_dim * out_dim) throw ScannError::invalid_argument("projection: matrix must hold out_dim * in_dim values");
            if (kind == ProjectionKind::Pca && mean_.size() != in_dim) throw ScannError::invalid_argument("projection: mean must hold in_dim values");
        }
    }
    ProjectionKind kind_;
    size_t in_dim_, out_dim_, start_;
    std::vector<float> matrix_, mean_;
};

// ---- AsymmetricHasher (hashes/hasher.rs) ---------------------------------------------------
struct AsymmetricHasherConfig {      // hasher.rs:19-69 (default 256 x 8: byte codes; K <= 16 takes the LUT16 path)
    size_t num_codes = 256, num_subspaces = 8;
    uint64_t seed = 42;
    bool has_seed = false;
    size_t training_iterations = 25;       // CodebookConfig.max_iterations
    double convergence_threshold = 1e-5;   // CodebookConfig.convergence_threshold
    AsymmetricHasherConfig() = default;
    AsymmetricHasherConfig(size_t codes, size_t subspaces) : num_codes(codes), num_subspaces(subspaces) {}
    AsymmetricHasherConfig with_seed(uint64_t s) const { auto c = *this; c.seed = s; c.has_seed = true; return c; }
};

class AsymmetricHasher {
public:
    explicit AsymmetricHasher(AsymmetricHasherConfig config, int device = 0) : config_(config), device_(device) {}

    void build(DenseDataset dataset) {            // hasher.rs:109-134
        build_impl(dataset, true);
        dataset_ = std::make_shared<DenseDataset>(std::move(dataset));
    }
    void build_no_store(const DenseDataset &dataset) { build_impl(dataset, false); }   // :137-159
    // build / build_no_store from rows that are already on the device, in one call (scann_hip_txh_build with
    // num_partitions 0): `source` keeps its rows and stays the caller's, the new handle takes its own copy when `store`.
    // The codebook is the one build() trains (same training rows, same seeds); it and the codes stay on the device, so
    // codebook() and encoded_database() are empty afterwards.
    void build_on_device(const BruteForceSearcher &source, bool store = true, scann_hip_build_report *report = nullptr) {
        build_device_impl(source, nullptr, store, report);
    }
    // The same for a PROJECTED hasher (scann_hip_txh_build_projected): the rows of `source` (projection.in_dim floats
    // each) are projected on the device, the codebook is trained and the rows are encoded in the projected space, and
    // searches take queries in the rows' own space; with `store` the re-ranking scores the original rows.
    void build_projected_on_device(const BruteForceSearcher &source, const DeviceProjection &projection, bool store = true,
                                   scann_hip_build_report *report = nullptr) {
        build_device_impl(source, &projection, store, report);
    }

private:
    void build_device_impl(const BruteForceSearcher &source, const DeviceProjection *projection, bool store,
                           scann_hip_build_report *report) {
        scann_hip_build_config c;
        scann_hip_build_config_default(&c);
        c.num_partitions = 0;
        c.num_subspaces = (uint32_t)config_.num_subspaces;
        c.num_codes = (uint32_t)config_.num_codes;
        c.training_iterations = (uint32_t)config_.training_iterations;
        c.convergence_threshold = config_.convergence_threshold;
        c.seed = config_.seed;
        c.store_rows = store ? 1 : 0;
        c.partitions_to_search = 1;
        c.pre_reorder_multiplier = 1.0f;
        scann_hip_index *h = nullptr;
        if (projection) check(scann_hip_txh_build_projected(source.handle(), projection->handle(), &c, &h, report));
        else check(scann_hip_txh_build(source.handle(), &c, &h, report));
        if (ix_.h) scann_hip_index_destroy(ix_.h);
        ix_.h = h;
        n_ = source.dataset_size();
        dim_ = source.dimensionality();
        stored_ = store;
        dataset_.reset();
        codebook_.clear();
        codes_.clear();
    }

public:

    NNResultsVector search(const std::vector<float> &query, size_t k) const {          // :162-185
        if (!ix_.h) return {};
        scann_hip_search_opts o;
        scann_hip_search_opts_default(&o);
        o.exact_reorder = 0;
        return detail::run_search(ix_.h, query.data(), 1, (uint32_t)query.size(), (uint32_t)query.size(),
                                  (uint32_t)k, &o)[0];
    }
    NNResultsVector search_with_reordering(const std::vector<float> &query, size_t k, size_t pre_reorder_k) const {
        if (!stored_) throw ScannError::failed_precondition("Dataset not stored");    // :194-197
        scann_hip_search_opts o;
        scann_hip_search_opts_default(&o);
        o.pre_reorder_k = (uint32_t)pre_reorder_k;
        return detail::run_search(ix_.h, query.data(), 1, (uint32_t)query.size(), (uint32_t)query.size(),
                                  (uint32_t)k, &o)[0];
    }
    // CrowdingConstraint::apply(search(query, depth), k) on the device (search = the approximate search above)
    NNResultsVector search_with_crowding(const std::vector<float> &query, size_t k, size_t depth,
                                         const CrowdingConstraint &constraint) const {
        if (!constraint.config().enabled || !ix_.h) return search(query, k);
        scann_hip_search_opts o;
        scann_hip_search_opts_default(&o);
        o.exact_reorder = 0;
        return detail::run_search_crowded(ix_.h, crowd_, query, k, depth, constraint, &o);
    }
    std::vector<NNResultsVector> search_batched(const std::vector<std::vector<float>> &queries, size_t k) const {
        if (queries.empty() || !ix_.h) return std::vector<NNResultsVector>(queries.size());
        uint32_t d;
        auto flat = detail::flatten(queries, &d);
        scann_hip_search_opts o;
        scann_hip_search_opts_default(&o);
        o.exact_reorder = 0;
        return detail::run_search(ix_.h, flat.data(), (uint32_t)queries.size(), d, d, (uint32_t)k, &o);
    }
    // search_with_filter for a batch: query i under filters[i] (null = everything allowed), materialised into one
    // strided bitmap block (scann_hip_search_opts.allow_bitmap_stride) and searched in one call
    std::vector<NNResultsVector> search_batched_with_filters(const std::vector<std::vector<float>> &queries, size_t k,
                                                             const std::vector<const RestrictFilter *> &filters) const {
        if (!ix_.h) return std::vector<NNResultsVector>(queries.size());
        scann_hip_search_opts o;
        scann_hip_search_opts_default(&o);
        o.exact_reorder = 0;
        return detail::run_search_filters(ix_.h, queries, k, filters, num_datapoints(), o);
    }
    // query i under device_map's create_allowlist(token_lists[i]): the bitmap block is built on the device from the
    // resident map and searched on the same stream; no bitmap or id list crosses from the host
    std::vector<NNResultsVector> search_batched_with_tokens(const std::vector<std::vector<float>> &queries, size_t k,
                                                            const std::vector<std::vector<uint64_t>> &token_lists,
                                                            const DeviceTokenMap &device_map) const {
        if (!ix_.h) return std::vector<NNResultsVector>(queries.size());
        scann_hip_search_opts o;
        scann_hip_search_opts_default(&o);
        o.exact_reorder = 0;
        return detail::run_search_tokens(ix_.h, queries, k, token_lists, device_map, o);
    }
    // query i under the ranges bounds[(i * cols.size() + c) * 2 + {0, 1}] over `table`'s clause columns `cols`: the
    // bitmap block is built on the device from the resident columns and searched on the same stream
    std::vector<NNResultsVector> search_batched_with_ranges(const std::vector<std::vector<float>> &queries, size_t k,
                                                            const std::vector<uint32_t> &cols,
                                                            const std::vector<scann_hip_range_bound> &bounds,
                                                            const AttributeTable &table) const {
        if (!ix_.h) return std::vector<NNResultsVector>(queries.size());
        scann_hip_search_opts o;
        scann_hip_search_opts_default(&o);
        o.exact_reorder = 0;
        return detail::run_search_ranges(ix_.h, queries, k, cols, bounds, table, o);
    }
    size_t num_datapoints() const { return n_; }
    size_t dimensionality() const { return dim_; }
    const std::vector<float> &codebook() const { return codebook_; }
    const std::vector<uint8_t> &encoded_database() const { return codes_; }

private:
    void build_impl(const DenseDataset &ds, bool store) {
        if (ds.is_empty()) throw ScannError::invalid_argument("Cannot build from empty dataset");  // :110-112
        dim_ = ds.dimensionality();
        n_ = ds.size();
        const uint32_t S = (uint32_t)config_.num_subspaces, K = (uint32_t)config_.num_codes;
        {
            detail::IndexHandle tmp;   // training rows resident on the GPU for the k-means passes
            check(scann_hip_bf_create(context(device_), ds.raw_data(), n_, (uint32_t)dim_, ds.stride(),
                                      SCANN_HIP_SQUARED_L2, &tmp.h));
            codebook_ = detail::train_codebook(tmp.h, n_, (uint32_t)dim_, S, K, config_.seed,
                                               config_.training_iterations, config_.convergence_threshold);
        }
        codes_.assign(n_ * S, 0);
        check(scann_hip_encode(context(device_), codebook_.data(), S, K, (uint32_t)dim_ / S, ds.raw_data(), n_,
                               ds.stride(), nullptr, nullptr, codes_.data()));
        scann_hip_txh_desc d{};
        d.data = store ? ds.raw_data() : nullptr;
        d.n_rows = n_;
        d.dim = (uint32_t)dim_;
        d.stride = ds.stride();
        d.n_local = n_;
        d.codebook = codebook_.data();
        d.num_subspaces = S;
        d.num_codes = K;
        d.dims_per_subspace = (uint32_t)dim_ / S;
        d.codes = codes_.data();
        d.partitions_to_search = 1;
        d.pre_reorder_multiplier = 1.0f;
        if (ix_.h) { scann_hip_index_destroy(ix_.h); ix_.h = nullptr; }
        check(scann_hip_txh_create(context(device_), &d, &ix_.h));
        stored_ = store;
    }
    AsymmetricHasherConfig config_;
    int device_;
    std::shared_ptr<DenseDataset> dataset_;
    std::vector<float> codebook_;
    std::vector<uint8_t> codes_;
    size_t n_ = 0, dim_ = 0;
    bool stored_ = false;
    detail::IndexHandle ix_;
    detail::CrowdAttach crowd_;
};

// ---- TreeXHybridSearcher (tree_x_hybrid/mod.rs) ------------------------------------------------
struct TreeXHybridConfig {           // mod.rs:23-78
    size_t num_partitions = 100, partitions_to_search = 10;
    AsymmetricHasherConfig hash_config;
    bool use_residuals = true;
    float pre_reorder_multiplier = 3.0f;
    bool parallel_partition_search = true;   // no effect: every leaf scan is parallel on the GPU
    size_t kmeans_iterations = 100;   // tree_partitioner.rs:72 with_max_iterations(100)
    TreeXHybridConfig() = default;
    TreeXHybridConfig(size_t parts, size_t to_search) : num_partitions(parts), partitions_to_search(to_search) {}
    TreeXHybridConfig with_hash(AsymmetricHasherConfig c) const { auto t = *this; t.hash_config = c; return t; }
    TreeXHybridConfig with_residuals(bool r) const { auto t = *this; t.use_residuals = r; return t; }
    TreeXHybridConfig with_pre_reorder(float m) const { auto t = *this; t.pre_reorder_multiplier = m; return t; }
};

class TreeXHybridSearcher {
public:
    explicit TreeXHybridSearcher(TreeXHybridConfig config, int device = 0) : config_(config), device_(device) {}

    void build(DenseDataset dataset) {     // mod.rs:131-209
        if (dataset.is_empty()) throw ScannError::invalid_argument("Cannot build from empty dataset");
        dataset_ = std::make_shared<DenseDataset>(std::move(dataset));
        const DenseDataset &ds = *dataset_;
        const size_t n = ds.size(), dim = ds.dimensionality();
        const uint32_t S = (uint32_t)config_.hash_config.num_subspaces, K = (uint32_t)config_.hash_config.num_codes;
        if (dim % S != 0)
            throw ScannError::invalid_argument("Dimensionality " + std::to_string(dim) +
                                               " must be divisible by num_subspaces " + std::to_string(S));
        detail::build_partition(ds, config_.num_partitions, config_.kmeans_iterations, device_, centers_, leaf_off_,
                                leaf_ids_);
        const uint32_t L = (uint32_t)(centers_.size() / dim);
        // residual rows in CSR order (mod.rs:177-189), codebook on residuals (:151-158)
        std::vector<float> rows(n * dim);
        std::vector<uint32_t> leaf_of_row(n);
        for (uint32_t l = 0; l < L; ++l)
            for (uint32_t r = leaf_off_[l]; r < leaf_off_[l + 1]; ++r) {
                const float *x = ds.get(leaf_ids_[r]);
                leaf_of_row[r] = l;
                for (size_t j = 0; j < dim; ++j)
                    rows[r * dim + j] = config_.use_residuals ? x[j] - centers_[l * dim + j] : x[j];
            }
        {
            detail::IndexHandle tmp;   // residual rows resident on the GPU for the codebook k-means
            check(scann_hip_bf_create(context(device_), rows.data(), n, (uint32_t)dim, (uint32_t)dim,
                                      SCANN_HIP_SQUARED_L2, &tmp.h));
            codebook_ = detail::train_codebook(tmp.h, n, (uint32_t)dim, S, K, config_.hash_config.seed,
                                               config_.hash_config.training_iterations,
                                               config_.hash_config.convergence_threshold);
        }
        codes_.assign(n * S, 0);
        check(scann_hip_encode(context(device_), codebook_.data(), S, K, (uint32_t)dim / S, rows.data(), n,
                               (uint32_t)dim, nullptr, nullptr, codes_.data()));
        n_ = n;
        dim_ = dim;
        const scann_hip_txh_desc d = desc();
        if (ix_.h) { scann_hip_index_destroy(ix_.h); ix_.h = nullptr; }
        check(scann_hip_txh_create(context(device_), &d, &ix_.h));
    }

    // build() from rows that are already on the device, in one call (scann_hip_txh_build): partitioner, residuals,
    // codebook, codes and CSR layout never leave it; `source` keeps its rows and stays the caller's.  NOT the arrays of
    // build() above: that trains the codebook on the residuals in CSR order against the k-means assignment, this one --
    // as the reference does (mod.rs:151-158, 211-237) -- in datapoint order against partition(x, 1), another training
    // order and therefore another codebook.  The index lives on the device only: save() needs a searcher made by
    // build() or load().
    void build_on_device(const BruteForceSearcher &source, scann_hip_build_report *report = nullptr) {
        build_device_impl(source, nullptr, report);
    }
    // The same for a PROJECTED index (scann_hip_txh_build_projected): the rows of `source` (projection.in_dim floats each)
    // are projected on the device, the index is built in the projected space, searches take queries in the rows' own
    // space and re-rank against the original rows.
    void build_projected_on_device(const BruteForceSearcher &source, const DeviceProjection &projection,
                                   scann_hip_build_report *report = nullptr) {
        build_device_impl(source, &projection, report);
    }
    // build_on_device with the partitioner of TreePartitioner::build_hierarchical (scann_hip_txh_build_hierarchical): a
    // k-means tree trained level by level on the device and flattened to its leaves, which become the partitions.
    // `tree` replaces config().num_partitions and kmeans_iterations; everything else is read from config() as above.
    void build_hierarchical_on_device(const BruteForceSearcher &source, const scann_hip_tree_config &tree,
                                      scann_hip_build_report *report = nullptr,
                                      scann_hip_tree_report *tree_report = nullptr) {
        build_device_impl(source, nullptr, report, &tree, tree_report);
    }

private:
    void build_device_impl(const BruteForceSearcher &source, const DeviceProjection *projection,
                           scann_hip_build_report *report, const scann_hip_tree_config *tree = nullptr,
                           scann_hip_tree_report *tree_report = nullptr) {
        scann_hip_build_config c;
        scann_hip_build_config_default(&c);
        c.num_partitions = (uint32_t)config_.num_partitions;
        c.kmeans_iterations = (uint32_t)config_.kmeans_iterations;
        c.num_subspaces = (uint32_t)config_.hash_config.num_subspaces;
        c.num_codes = (uint32_t)config_.hash_config.num_codes;
        c.training_iterations = (uint32_t)config_.hash_config.training_iterations;
        c.convergence_threshold = config_.hash_config.convergence_threshold;
        c.seed = config_.hash_config.seed;
        c.use_residuals = config_.use_residuals ? 1 : 0;
        c.partitions_to_search = (uint32_t)config_.partitions_to_search;
        c.pre_reorder_multiplier = config_.pre_reorder_multiplier;
        if (!tree && c.num_partitions == 0) throw ScannError::invalid_argument("num_partitions is 0");
        scann_hip_index *h = nullptr;
        scann_hip_tree_report trep;
        if (tree) check(scann_hip_txh_build_hierarchical(source.handle(), tree, &c, &h, report, &trep));
        else if (projection) check(scann_hip_txh_build_projected(source.handle(), projection->handle(), &c, &h, report));
        else check(scann_hip_txh_build(source.handle(), &c, &h, report));
        if (tree && tree_report) *tree_report = trep;
        if (ix_.h) scann_hip_index_destroy(ix_.h);
        ix_.h = h;
        n_ = source.dataset_size();
        dim_ = source.dimensionality();
        L_ = tree ? (size_t)trep.num_leaves : std::min<size_t>(config_.num_partitions, n_);
        dataset_.reset();
        centers_.clear(); codebook_.clear(); leaf_off_.clear(); leaf_ids_.clear(); codes_.clear();
    }

public:

    NNResultsVector search(const std::vector<float> &query, size_t k) const {   // mod.rs:240-294
        if (!ix_.h) throw ScannError::failed_precondition("Partitioner not built");
        return detail::run_search(ix_.h, query.data(), 1, (uint32_t)query.size(), (uint32_t)query.size(),
                                  (uint32_t)k, nullptr)[0];
    }
    // CrowdingConstraint::apply(search(query, depth), k) on the device
    NNResultsVector search_with_crowding(const std::vector<float> &query, size_t k, size_t depth,
                                         const CrowdingConstraint &constraint) const {
        if (!constraint.config().enabled) return search(query, k);
        if (!ix_.h) throw ScannError::failed_precondition("Partitioner not built");
        return detail::run_search_crowded(ix_.h, crowd_, query, k, depth, constraint, nullptr);
    }
    // mod.rs:245-294: disallowed datapoints are skipped before scoring.  The filter is
    // materialised once into an allow-bitmap that the scan kernels test.
    NNResultsVector search_with_filter(const std::vector<float> &query, size_t k,
                                       const RestrictFilter *filter) const {
        if (!filter) return search(query, k);
        if (!ix_.h) throw ScannError::failed_precondition("Partitioner not built");
        const auto bits = filter->to_bitmap(num_datapoints());
        scann_hip_search_opts o;
        scann_hip_search_opts_default(&o);
        o.allow_bitmap = bits.data();
        o.allow_bitmap_bits = bits.size() * 64;
        return detail::run_search(ix_.h, query.data(), 1, (uint32_t)query.size(), (uint32_t)query.size(),
                                  (uint32_t)k, &o)[0];
    }
    std::vector<NNResultsVector> search_batched(const std::vector<std::vector<float>> &queries, size_t k) const {
        if (!ix_.h) throw ScannError::failed_precondition("Partitioner not built");
        if (queries.empty()) return {};
        uint32_t d;
        auto flat = detail::flatten(queries, &d);
        return detail::run_search(ix_.h, flat.data(), (uint32_t)queries.size(), d, d, (uint32_t)k, nullptr);
    }
    // search_with_filter for a batch: query i under filters[i] (null = everything allowed), materialised into one
    // strided bitmap block (scann_hip_search_opts.allow_bitmap_stride) and searched in one call
    std::vector<NNResultsVector> search_batched_with_filters(const std::vector<std::vector<float>> &queries, size_t k,
                                                             const std::vector<const RestrictFilter *> &filters) const {
        if (!ix_.h) throw ScannError::failed_precondition("Partitioner not built");
        scann_hip_search_opts o;
        scann_hip_search_opts_default(&o);
        return detail::run_search_filters(ix_.h, queries, k, filters, num_datapoints(), o);
    }
    // query i under device_map's create_allowlist(token_lists[i]): the bitmap block is built on the device from the
    // resident map and searched on the same stream; no bitmap or id list crosses from the host
    std::vector<NNResultsVector> search_batched_with_tokens(const std::vector<std::vector<float>> &queries, size_t k,
                                                            const std::vector<std::vector<uint64_t>> &token_lists,
                                                            const DeviceTokenMap &device_map) const {
        if (!ix_.h) throw ScannError::failed_precondition("Partitioner not built");
        scann_hip_search_opts o;
        scann_hip_search_opts_default(&o);
        return detail::run_search_tokens(ix_.h, queries, k, token_lists, device_map, o);
    }
    // query i under the ranges bounds[(i * cols.size() + c) * 2 + {0, 1}] over `table`'s clause columns `cols`: the
    // bitmap block is built on the device from the resident columns and searched on the same stream
    std::vector<NNResultsVector> search_batched_with_ranges(const std::vector<std::vector<float>> &queries, size_t k,
                                                            const std::vector<uint32_t> &cols,
                                                            const std::vector<scann_hip_range_bound> &bounds,
                                                            const AttributeTable &table) const {
        if (!ix_.h) throw ScannError::failed_precondition("Partitioner not built");
        scann_hip_search_opts o;
        scann_hip_search_opts_default(&o);
        return detail::run_search_ranges(ix_.h, queries, k, cols, bounds, table, o);
    }
    // Searcher::search_batched_with_params (tree_x_hybrid/mod.rs:399-409): params[i].num_neighbors per query
    std::vector<NNResultsVector> search_batched_with_params(const std::vector<std::vector<float>> &queries,
                                                            const std::vector<uint32_t> &num_neighbors) const {
        if (!ix_.h) throw ScannError::failed_precondition("Partitioner not built");
        if (queries.size() != num_neighbors.size()) throw ScannError::invalid_argument("one SearchParameters per query");
        if (queries.empty()) return {};
        uint32_t d;
        auto flat = detail::flatten(queries, &d);
        return detail::run_search_params(ix_.h, flat.data(), (uint32_t)queries.size(), d, d, num_neighbors, nullptr);
    }
    size_t num_partitions() const { return L_ ? L_ : (leaf_off_.empty() ? 0 : leaf_off_.size() - 1); }
    size_t num_datapoints() const { return n_; }
    size_t dataset_size() const { return num_datapoints(); }
    uint64_t dimensionality() const { return dim_; }
    const TreeXHybridConfig &config() const { return config_; }

    // Index files (include/scann_hip.h "index files"; the reference has no save/load): the built
    // index as one SCANNIDX container, and a searcher over a file that is mmap'ed and uploaded
    // without a second host copy.
    void save(const std::string &path) const {
        if (!ix_.h || !dataset_) throw ScannError::failed_precondition("Partitioner not built");
        if (quantized_ || projected_) {   // the rows live on the device only, as stored: sections rows_q / rows_q_meta, or proj_*
            check(scann_hip_index_write_file(ix_.h, path.c_str()));
            return;
        }
        const scann_hip_txh_desc d = desc();
        check(scann_hip_txh_write_file(path.c_str(), &d));
    }
    // This searcher's trained index (centres, codebook, codes) over re-rank rows the caller stores quantized
    // (scann_hip_txh_create_quantized): n rows of `stride` elements of row_format (SCANN_HIP_ROWS_BF16 / _FP8_E4M3 /
    // _INT8; int8 value = i8 * inv_multiplier), by datapoint index.  The new searcher keeps no f32 rows on the device;
    // it re-ranks with the arithmetic of a quantized brute-force handle.  load() reads a file it saved.
    TreeXHybridSearcher with_quantized_rows(const void *rows, int row_format, float inv_multiplier, uint32_t stride) const {
        if (!ix_.h || !dataset_) throw ScannError::failed_precondition("Partitioner not built");
        TreeXHybridSearcher s(config_, device_);
        s.dataset_ = dataset_;
        s.centers_ = centers_; s.codebook_ = codebook_; s.leaf_off_ = leaf_off_; s.leaf_ids_ = leaf_ids_; s.codes_ = codes_;
        s.n_ = n_; s.dim_ = dim_;
        s.quantized_ = true;
        scann_hip_txh_desc d = s.desc();
        d.data = nullptr;
        d.stride = stride;
        check(scann_hip_txh_create_quantized(context(device_), &d, rows, row_format, inv_multiplier, &s.ix_.h));
        return s;
    }
    // This searcher was built over PROJECTED rows (Projection::project_dataset): the new searcher takes queries of the
    // original dimensionality, projects them on the device, runs this searcher's trained index (centres, codebook,
    // codes) in the projected space and re-ranks the survivors against `original` (scann_hip_txh_create_projected).
    TreeXHybridSearcher with_projection(const Projection &projection, const DenseDataset &original) const {
        if (!ix_.h || !dataset_) throw ScannError::failed_precondition("Partitioner not built");
        if (original.size() != n_) throw ScannError::invalid_argument("the original dataset must hold the indexed rows");
        TreeXHybridSearcher s(config_, device_);
        s.dataset_ = dataset_;
        s.centers_ = centers_; s.codebook_ = codebook_; s.leaf_off_ = leaf_off_; s.leaf_ids_ = leaf_ids_; s.codes_ = codes_;
        s.n_ = n_; s.dim_ = original.dimensionality();
        s.projected_ = true;
        scann_hip_txh_desc d = s.desc();
        d.data = nullptr;
        const DeviceProjection dp = projection.to_device(device_);
        check(scann_hip_txh_create_projected(context(device_), &d, dp.handle(), original.raw_data(), original.size(),
                                             (uint32_t)original.dimensionality(), original.stride(), &s.ix_.h));
        return s;
    }
    static TreeXHybridSearcher load(const std::string &path, int device = 0) {
        scann_hip_file_info info;
        check(scann_hip_index_file_info(path.c_str(), &info));
        if (info.kind != 1 || info.num_partitions == 0 || info.num_subspaces == 0)
            throw ScannError::invalid_argument(path + " does not hold a Tree-X-Hybrid index");
        TreeXHybridConfig c(info.num_partitions, info.partitions_to_search);
        c.hash_config = AsymmetricHasherConfig(info.num_codes, info.num_subspaces);
        c.use_residuals = info.use_residuals != 0;
        c.pre_reorder_multiplier = info.pre_reorder_multiplier;
        TreeXHybridSearcher s(c, device);
        check(scann_hip_index_load_file(context(device), path.c_str(), &s.ix_.h));
        s.n_ = info.n_rows;
        s.dim_ = scann_hip_index_dimensionality(s.ix_.h);   // (a projected file: the rows' space, not info.dim)
        s.L_ = info.num_partitions;
        return s;
    }

private:
    scann_hip_txh_desc desc() const {
        const DenseDataset &ds = *dataset_;
        const uint32_t S = (uint32_t)config_.hash_config.num_subspaces;
        scann_hip_txh_desc d{};
        d.data = ds.raw_data();
        d.n_rows = ds.size();
        d.dim = (uint32_t)ds.dimensionality();
        d.stride = ds.stride();
        d.centers = centers_.data();
        d.num_partitions = (uint32_t)(leaf_off_.size() - 1);
        d.leaf_offsets = leaf_off_.data();
        d.leaf_ids = leaf_ids_.data();
        d.n_local = ds.size();
        d.codebook = codebook_.data();
        d.num_subspaces = S;
        d.num_codes = (uint32_t)config_.hash_config.num_codes;
        d.dims_per_subspace = d.dim / S;
        d.codes = codes_.data();
        d.use_residuals = config_.use_residuals ? 1 : 0;
        d.partitions_to_search = (uint32_t)config_.partitions_to_search;
        d.pre_reorder_multiplier = config_.pre_reorder_multiplier;
        return d;
    }
    TreeXHybridConfig config_;
    int device_;
    std::shared_ptr<DenseDataset> dataset_;
    std::vector<float> centers_, codebook_;
    std::vector<uint32_t> leaf_off_, leaf_ids_;
    std::vector<uint8_t> codes_;
    size_t n_ = 0, dim_ = 0, L_ = 0;
    bool projected_ = false;   // with_projection: the handle searches through a projection, dataset_ holds the projected rows
    bool quantized_ = false;   // with_quantized_rows: the handle's rows are quantized, dataset_ only names the model's rows
    detail::IndexHandle ix_;
    detail::CrowdAttach crowd_;
};

namespace detail {
inline void build_partition(const DenseDataset &ds, size_t num_partitions, size_t iterations, int device,
                            std::vector<float> &centers, std::vector<uint32_t> &leaf_off,
                            std::vector<uint32_t> &leaf_ids) {
    const size_t n = ds.size(), dim = ds.dimensionality();
    std::vector<uint32_t> assign;
    {
        IndexHandle tmp;
        check(scann_hip_bf_create(context(device), ds.raw_data(), n, (uint32_t)dim, ds.stride(), SCANN_HIP_SQUARED_L2,
                                  &tmp.h));
        kmeans_gpu(tmp.h, n, 0, dim, num_partitions, iterations, 1e-5, 42, centers, assign);
    }
    const uint32_t L = (uint32_t)(centers.size() / dim);
    leaf_off.assign(L + 1, 0);
    for (uint32_t a : assign) ++leaf_off[a + 1];
    for (uint32_t l = 0; l < L; ++l) leaf_off[l + 1] += leaf_off[l];
    leaf_ids.assign(n, 0);
    std::vector<uint32_t> cur(leaf_off.begin(), leaf_off.end() - 1);
    for (size_t i = 0; i < n; ++i) leaf_ids[cur[assign[i]]++] = (uint32_t)i;   // ascending idx per leaf
}
}  // namespace detail

// ---- ScannConfig (config.rs:10-320: the fields the hot path reads) ------------------------------
struct PartitioningConfig {          // config.rs:134-199
    uint32_t num_partitions = 100, num_partitions_to_search = 10;
};
struct HashConfig {                  // config.rs:202-261
    uint32_t num_buckets = 256, num_blocks = 16;
};
struct ExactReorderingConfig {       // config.rs:283-320
    uint32_t num_candidates = 100;
};
struct ScannConfig {                 // config.rs:10-118
    uint32_t num_neighbors = 10;
    DistanceMeasure distance_measure = DistanceMeasure::SquaredL2;
    bool brute_force = false;
    bool has_partitioning = false, has_hash = false, has_exact_reordering = false;
    PartitioningConfig partitioning;
    HashConfig hash;
    ExactReorderingConfig exact_reordering;
    ScannConfig with_num_neighbors(uint32_t k) const { auto c = *this; c.num_neighbors = k; return c; }
    ScannConfig with_distance_measure(DistanceMeasure m) const { auto c = *this; c.distance_measure = m; return c; }
    ScannConfig with_brute_force() const {   // :63-68 clears the other two
        auto c = *this; c.brute_force = true; c.has_partitioning = false; c.has_hash = false; return c;
    }
    ScannConfig with_partitioning(PartitioningConfig p) const { auto c = *this; c.partitioning = p; c.has_partitioning = true; return c; }
    ScannConfig with_hash(HashConfig h) const { auto c = *this; c.hash = h; c.has_hash = true; return c; }
    ScannConfig with_exact_reordering(ExactReorderingConfig r) const {
        auto c = *this; c.exact_reordering = r; c.has_exact_reordering = true; return c;
    }
};

enum class SearchMode { BruteForce, Partitioned, Hashed, TreeAH };   // scann.rs:17-28

// ---- Scann facade (scann.rs:30-362) ------------------------------------------------------------
// One GPU index per mode, all configurations of the same kernels (include/scann_hip.h):
//   Partitioned  exact scan of the selected leaves' rows     search_partitioned  :213-252
//   Hashed       AsymmetricHasher::search                    search_impl         :189-192
//   TreeAH       one non-residual table per query, k best    search_tree_ah      :255-294
// and the exact reordering of the k-truncated list with the configured measure (:199-209) runs
// inside the same search call (pre_reorder_k = k, exact_reorder = 1).
class Scann {
public:
    explicit Scann(DenseDataset dataset, int device = 0) : Scann(std::move(dataset), ScannConfig(), device) {}
    Scann(DenseDataset dataset, ScannConfig config, int device = 0) : config_(config), device_(device) {   // :63-103
        if (dataset.is_empty()) throw ScannError::invalid_argument("Dataset cannot be empty");  // :64-66
        dataset_ = std::make_shared<DenseDataset>(std::move(dataset));
        bf_.reset(new BruteForceSearcher(dataset_, config_.distance_measure, device));
        if (config_.brute_force) {
            mode_ = SearchMode::BruteForce;
        } else if (config_.has_partitioning && config_.has_hash) {
            init_partitioning();
            init_hashing();
            mode_ = SearchMode::TreeAH;
            create_index(true, true);
        } else if (config_.has_partitioning) {
            init_partitioning();
            mode_ = SearchMode::Partitioned;
            create_index(true, false);
        } else if (config_.has_hash) {
            init_hashing();
            mode_ = SearchMode::Hashed;
            create_index(false, true);
        }
    }
    static Scann brute_force(DenseDataset ds) { return Scann(std::move(ds), ScannConfig().with_brute_force()); }   // :106-109
    static Scann partitioned(DenseDataset ds, uint32_t num_partitions, uint32_t partitions_to_search) {          // :112-124
        PartitioningConfig p;
        p.num_partitions = num_partitions;
        p.num_partitions_to_search = partitions_to_search;
        return Scann(std::move(ds), ScannConfig().with_partitioning(p));
    }
    static Scann hashed(DenseDataset ds, uint32_t num_blocks) {                                                  // :127-137
        HashConfig h;
        h.num_blocks = num_blocks;
        return Scann(std::move(ds), ScannConfig().with_hash(h));
    }

    NNResultsVector search(const std::vector<float> &q, size_t k) const {      // :175-212
        return search_batched({q}, k)[0];
    }
    // :297-303 maps search over the queries; here the whole batch is one GPU call
    std::vector<NNResultsVector> search_batched(const std::vector<std::vector<float>> &qs, size_t k) const {
        if (qs.empty()) return {};
        // the reordering of a brute-force result re-scores it with the same kernel: a no-op
        if (mode_ == SearchMode::BruteForce) return bf_->search_batched(qs, k);
        uint32_t d;
        auto flat = detail::flatten(qs, &d);
        scann_hip_search_opts o;
        scann_hip_search_opts_default(&o);
        o.pre_reorder_k = (uint32_t)k;
        const bool reorder = config_.has_exact_reordering && config_.exact_reordering.num_candidates > k;   // :199-201
        o.exact_reorder = (reorder && mode_ != SearchMode::Partitioned) ? 1 : 0;
        if (mode_ != SearchMode::Hashed) o.partitions_to_search = config_.partitioning.num_partitions_to_search;
        return detail::run_search(ix_.h, flat.data(), (uint32_t)qs.size(), d, d, (uint32_t)k, &o);
    }
    // CrowdingConstraint::apply(search(query, depth), k) on the device, search as configured above
    NNResultsVector search_with_crowding(const std::vector<float> &q, size_t k, size_t depth,
                                         const CrowdingConstraint &constraint) const {
        if (!constraint.config().enabled) return search(q, k);
        if (mode_ == SearchMode::BruteForce) return bf_->search_with_crowding(q, k, depth, constraint);
        const size_t dd = depth ? depth : k;
        scann_hip_search_opts o;
        scann_hip_search_opts_default(&o);
        o.pre_reorder_k = (uint32_t)dd;
        const bool reorder = config_.has_exact_reordering && config_.exact_reordering.num_candidates > dd;
        o.exact_reorder = (reorder && mode_ != SearchMode::Partitioned) ? 1 : 0;
        if (mode_ != SearchMode::Hashed) o.partitions_to_search = config_.partitioning.num_partitions_to_search;
        return detail::run_search_crowded(ix_.h, crowd_, q, k, dd, constraint, &o);
    }
    SearchMode search_mode() const { return mode_; }
    size_t size() const { return dataset_->size(); }
    uint64_t dimensionality() const { return dataset_->dimensionality(); }
    DistanceMeasure distance_measure() const { return config_.distance_measure; }
    const ScannConfig &config() const { return config_; }
    size_t dataset_size() const { return size(); }

private:
    void init_partitioning() {   // :140-150 -> TreePartitioner::build (tree_partitioner.rs:48-98)
        detail::build_partition(*dataset_, config_.partitioning.num_partitions, 100, device_, centers_, leaf_off_,
                                leaf_ids_);
    }
    void init_hashing() {        // :153-165 -> AsymmetricHasher::build (hasher.rs:109-134)
        const DenseDataset &ds = *dataset_;
        const uint32_t S = config_.hash.num_blocks, K = config_.hash.num_buckets, dim = (uint32_t)ds.dimensionality();
        AsymmetricHasherConfig hc(K, S);
        detail::IndexHandle tmp;
        check(scann_hip_bf_create(context(device_), ds.raw_data(), ds.size(), dim, ds.stride(), SCANN_HIP_SQUARED_L2,
                                  &tmp.h));
        codebook_ = detail::train_codebook(tmp.h, ds.size(), dim, S, K, hc.seed, hc.training_iterations,
                                           hc.convergence_threshold);
        codes_.assign(ds.size() * S, 0);
        check(scann_hip_encode(context(device_), codebook_.data(), S, K, dim / S, ds.raw_data(), ds.size(),
                               ds.stride(), nullptr, nullptr, codes_.data()));
    }
    void create_index(bool tree, bool hash) {
        const DenseDataset &ds = *dataset_;
        const size_t n = ds.size();
        scann_hip_txh_desc d{};
        d.data = ds.raw_data();
        d.n_rows = n;
        d.dim = (uint32_t)ds.dimensionality();
        d.stride = ds.stride();
        d.n_local = n;
        d.distance_measure = (int)config_.distance_measure;
        d.partitions_to_search = tree ? config_.partitioning.num_partitions_to_search : 1;
        d.pre_reorder_multiplier = 1.0f;
        std::vector<uint8_t> csr_codes;
        if (tree) {
            d.centers = centers_.data();
            d.num_partitions = (uint32_t)(leaf_off_.size() - 1);
            d.leaf_offsets = leaf_off_.data();
            d.leaf_ids = leaf_ids_.data();
        }
        if (hash) {
            const uint32_t S = config_.hash.num_blocks;
            d.codebook = codebook_.data();
            d.num_subspaces = S;
            d.num_codes = config_.hash.num_buckets;
            d.dims_per_subspace = d.dim / S;
            d.codes = codes_.data();
            if (tree) {   // encoded_database()[idx] (scann.rs:283) laid out in CSR row order
                csr_codes.resize(n * S);
                for (size_t r = 0; r < n; ++r)
                    std::memcpy(&csr_codes[r * S], &codes_[(size_t)leaf_ids_[r] * S], S);
                d.codes = csr_codes.data();
            }
        }
        check(scann_hip_txh_create(context(device_), &d, &ix_.h));
    }

    ScannConfig config_;
    int device_;
    SearchMode mode_ = SearchMode::BruteForce;
    std::shared_ptr<DenseDataset> dataset_;
    std::unique_ptr<BruteForceSearcher> bf_;
    std::vector<float> centers_, codebook_;
    std::vector<uint32_t> leaf_off_, leaf_ids_;
    std::vector<uint8_t> codes_;
    detail::IndexHandle ix_;
    detail::CrowdAttach crowd_;
};

class ScannBuilder {   // scann.rs:364-426
public:
    ScannBuilder &num_neighbors(uint32_t k) { config_.num_neighbors = k; return *this; }
    ScannBuilder &distance_measure(DistanceMeasure m) { config_.distance_measure = m; return *this; }
    ScannBuilder &brute_force() { config_ = config_.with_brute_force(); return *this; }
    ScannBuilder &tree(uint32_t num_partitions, uint32_t partitions_to_search) {
        config_.partitioning.num_partitions = num_partitions;
        config_.partitioning.num_partitions_to_search = partitions_to_search;
        config_.has_partitioning = true;
        return *this;
    }
    ScannBuilder &hash(uint32_t num_blocks) {
        config_.hash = HashConfig();
        config_.hash.num_blocks = num_blocks;
        config_.has_hash = true;
        return *this;
    }
    ScannBuilder &reorder(uint32_t num_candidates) {
        config_.exact_reordering.num_candidates = num_candidates;
        config_.has_exact_reordering = true;
        return *this;
    }
    Scann build(DenseDataset dataset) const { return Scann(std::move(dataset), config_); }

private:
    ScannConfig config_;
};

}  // namespace scann

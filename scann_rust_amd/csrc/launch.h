// launch.h -- the one place that launches kernels: the launch-error check, the dynamic-LDS attribute
// rule, the cached CU count and the run-time value -> template argument dispatch.
#pragma once

#include <mutex>
#include <type_traits>
#include <unordered_map>
#include <utility>

#include "common.h"

namespace scann {

#define LAUNCH_CHECK()                                                                \
    do {                                                                              \
        hipError_t _e = hipGetLastError();                                            \
        if (_e != hipSuccess)                                                         \
            return ::scann::fail(SCANN_HIP_INTERNAL, std::string("kernel launch: ") + hipGetErrorString(_e)); \
    } while (0)

// Drops the error a failed query (an event never recorded, a mapping that cannot be pinned) leaves behind,
// or the next launch check reports it as its own.
inline void clear_last_hip_error() { (void)hipGetLastError(); }

// CUs of the current device, read once per process (grid sizes).
inline int num_cus() {
    static const int cus = [] {
        int dev = 0, n = 256;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        return n;
    }();
    return cus;
}

// Static LDS (the kernel's own __shared__ arrays) of a kernel, asked of the code object once per kernel.
inline int static_lds_bytes(const void *kernel, size_t *out) {
    static std::mutex mu;
    static std::unordered_map<const void *, size_t> cache;
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(kernel);
    if (it == cache.end()) {
        hipFuncAttributes fa;
        SCANN_HIP_CHECK(hipFuncGetAttributes(&fa, kernel));
        it = cache.emplace(kernel, fa.sharedSizeBytes).first;
    }
    *out = it->second;
    return SCANN_HIP_OK;
}

// LDS of one CU.  A launcher that has a choice (a smaller tile, another kernel) sizes it against this, so that the
// dims an entry point refuses do not depend on the batch size (DESIGN.md "Dimensionality ceilings").
constexpr size_t kMaxLdsBytes = 160 * 1024;

// The dynamic-LDS attribute of a launch that asks for `bytes`.  Nothing is set at 64 KB or below.  Above, it is one
// constant per kernel (the CU's 160 KB less the kernel's static arrays: the attribute bounds the DYNAMIC part, and
// static + dynamic may not exceed the CU's LDS), never the launch's own size: threads searching different indexes
// set this attribute concurrently, and a smaller value written by one of them must not undercut another's launch.
inline int set_dyn_lds(const void *kernel, size_t bytes) {
    constexpr size_t kMaxLds = kMaxLdsBytes;
    if (bytes <= 64 * 1024) return SCANN_HIP_OK;
    size_t static_bytes = 0;
    if (bytes <= kMaxLds) SCANN_TRY(static_lds_bytes(kernel, &static_bytes));
    if (bytes + static_bytes > kMaxLds) return fail(SCANN_HIP_RESOURCE_EXHAUSTED, "kernel needs more than 160 KB of LDS");
    SCANN_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kMaxLds - static_bytes)));
    return SCANN_HIP_OK;
}

// Every kernel launch of the library: the LDS attribute rule, the launch, the launch-error check.
template <typename... Params, typename... Args>
int launch(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, Args &&...args) {
    SCANN_TRY(set_dyn_lds(reinterpret_cast<const void *>(kernel), lds_bytes));
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, std::forward<Args>(args)...);
    LAUNCH_CHECK();
    return SCANN_HIP_OK;
}

// ---- run-time value -> template argument ------------------------------------------------------------
// with_value<V0, V1, ..., Vn>(v, f) calls f(std::integral_constant<int, Vi>{}) for the Vi equal to v and returns
// what f returns; Vn is also the `default:` arm.  Only the listed values are instantiated.
template <int V, int... Vs, typename F>
int with_value(int v, F &&f) {
    if constexpr (sizeof...(Vs) == 0) {
        return f(std::integral_constant<int, V>{});
    } else {
        if (v == V) return f(std::integral_constant<int, V>{});
        return with_value<Vs...>(v, std::forward<F>(f));
    }
}

// every measure (default: DotProduct)
template <typename F>
int with_measure(int measure, F &&f) {
    return with_value<SCANN_HIP_L1, SCANN_HIP_COSINE, SCANN_HIP_SQUARED_L2, SCANN_HIP_L2, SCANN_HIP_DOT_PRODUCT>(
        measure, std::forward<F>(f));
}
// the measures of the dot-product family of kernels: SquaredL2, L2, DotProduct (default)
template <typename F>
int with_dot_measure(int measure, F &&f) {
    return with_value<SCANN_HIP_SQUARED_L2, SCANN_HIP_L2, SCANN_HIP_DOT_PRODUCT>(measure, std::forward<F>(f));
}
// quantized row formats (default: 0, f32 rows)
template <typename F>
int with_row_format(int fmt, F &&f) {
    return with_value<SCANN_HIP_ROWS_BF16, SCANN_HIP_ROWS_FP8_E4M3, SCANN_HIP_ROWS_INT8, 0>(fmt, std::forward<F>(f));
}

}  // namespace scann

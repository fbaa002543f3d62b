"""Per-query allow-lists, the parts that need no GPU: the ABI field scann_hip_search_opts.allow_bitmap_stride, the two
bitmaps-from-id-lists symbols, the host form of scann_hip_allow_bitmaps_from_ids against a numpy model
(tests/helpers.py words_of per query), and scann.hpp's search_batched_with_filters (compiled in the host C++ harness;
its materialised block equals the per-filter to_bitmap rows)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("scann_hip_allow_bitmaps_from_ids", "scann_hip_allow_bitmaps_from_ids_device")
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def _hip():
    from scann_rust_amd import build, hip
    build.build()
    return hip


def test_stride_is_the_last_field_and_defaults_to_zero():
    hip = _hip()
    assert hip.SearchOpts._fields_[-1][0] == "allow_bitmap_stride"
    assert hip.SearchOpts._fields_[-2][0] == "bf_exact"
    assert ctypes.sizeof(hip.SearchOpts._fields_[-1][1]) == 8
    o = hip.default_opts()
    assert o.allow_bitmap_stride == 0
    # the compiled library agrees with the ctypes layout (the size reaches past the new field)
    lay = hip.abi_layout()
    assert lay[2] == ctypes.sizeof(hip.SearchOpts) == hip.SearchOpts.allow_bitmap_stride.offset + 8
    assert lay[3] == hip.SearchOpts.bf_exact.offset


def test_from_ids_symbols_are_exported_and_documented():
    hip = _hip()
    lib = ctypes.CDLL(hip.LIB_PATH)
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    header = open(os.path.join(ROOT, "include", "scann_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in hip.EXPORTS
        assert re.search(r"\bfn %s\s*\(" % name, text), "INTEGRATION.md lacks " + name
        assert re.search(r"\b%s\s*\(" % name, header)
    assert "pub allow_bitmap_stride: u64," in text


def _lists(bits, nq, rng):
    """nq id lists for capacity `bits`: empty, single, duplicated, unsorted, with ids at and past the capacity"""
    kinds = [
        [],
        [0] if bits else [5],
        [bits - 1, bits - 1, 0, 0] if bits else [0, 0],
        sorted(rng.integers(0, max(bits, 1), 40).tolist(), reverse=True),
        [bits, bits + 1, bits + 63, bits + 64, 0xFFFFFFFF] + ([bits - 1] if bits else []),
    ]
    return [np.asarray(kinds[(i + 1) % len(kinds)] if nq == 1 else kinds[i % len(kinds)], np.uint32) for i in range(nq)]


@pytest.mark.parametrize("nq", [1, 5])
@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("bits", [0, 1, 63, 64, 65, 1000])
def test_host_from_ids_matches_the_numpy_model(bits, extra, nq):
    hip = _hip()
    L = hip.load()
    rng = np.random.default_rng([bits, extra, nq])
    words = -(-bits // 64)
    stride = words + extra
    lists = _lists(bits, nq, rng)
    if nq == 1 and bits:   # the single query gets every kind of id at once
        lists = [np.concatenate(_lists(bits, 5, rng))]
    ids = np.concatenate(lists + [np.zeros(0, np.uint32)]).astype(np.uint32)
    off = np.concatenate([[0], np.cumsum([l.size for l in lists])]).astype(np.uint64)
    out = np.full(max(nq * stride, 1), ONES)   # the function writes every word: gaps come back zero
    status = L.scann_hip_allow_bitmaps_from_ids(hip.ptr(ids, hip.u32p) if ids.size else None, hip.ptr(off, hip.u64p), nq,
                                                bits, stride, hip.ptr(out, hip.u64p))
    assert status == hip.OK
    got = out[:nq * stride].reshape(nq, stride)
    for i, l in enumerate(lists):
        want = H.words_of(l[l < bits], bits)[0][:words]
        assert np.array_equal(got[i, :words], want), "query %d" % i
        assert np.all(got[i, words:] == 0), "gap words of query %d" % i
    if nq * stride < out.size:
        assert out[nq * stride] == ONES   # nothing past the block
    # the Python wrapper: the same block
    assert np.array_equal(hip.allow_bitmaps_from_ids(ids, off, bits, stride), got)


def test_host_from_ids_refuses_a_short_stride():
    hip = _hip()
    L = hip.load()
    ids = np.array([1, 2, 3], np.uint32)
    off = np.array([0, 3], np.uint64)
    out = np.full(4, ONES)
    for bits, stride in ((65, 1), (1000, 15), (1, 0)):
        assert L.scann_hip_allow_bitmaps_from_ids(hip.ptr(ids, hip.u32p), hip.ptr(off, hip.u64p), 1, bits, stride,
                                                  hip.ptr(out, hip.u64p)) == hip.INVALID_ARGUMENT
        assert np.all(out == ONES), "a refused call wrote"
    with pytest.raises(hip.ScannError) as e:
        hip.allow_bitmaps_from_ids(ids, off, 65, 1)
    assert e.value.code == hip.INVALID_ARGUMENT


CPP = r"""
#include "scann.hpp"
#include <cstdio>
using namespace scann;
struct Odd : RestrictFilter {   // a filter that is not an allow-list: materialised through is_allowed
    bool is_allowed(DatapointIndex i) const override { return i % 3 == 1; }
};
int main() {
    // the batched entry exists on the tree and the hasher types, with this signature
    std::vector<NNResultsVector> (TreeXHybridSearcher::*pt)(const std::vector<std::vector<float>> &, size_t,
        const std::vector<const RestrictFilter *> &) const = &TreeXHybridSearcher::search_batched_with_filters;
    std::vector<NNResultsVector> (AsymmetricHasher::*pa)(const std::vector<std::vector<float>> &, size_t,
        const std::vector<const RestrictFilter *> &) const = &AsymmetricHasher::search_batched_with_filters;
    if (!pt || !pa) return 3;
    for (size_t n : {size_t(1), size_t(63), size_t(64), size_t(65), size_t(1000)}) {
        RestrictAllowlist a = RestrictAllowlist::from_indices({0, 5, 63, 64, 999, 5, 70000}, n);
        RestrictAllowlist big = RestrictAllowlist::from_indices({1, 2, 900, 1500}, 2000);   // capacity past n
        RestrictDenylist d = RestrictDenylist::from_indices({0, 1, 2, 64}, n);
        Odd o;
        std::vector<const RestrictFilter *> f = {&a, nullptr, &big, &d, &o, &a};
        uint64_t stride = 0;
        const auto block = detail::materialise_filters(f, n, &stride);
        const size_t words = (n + 63) / 64;
        if (stride != words || block.size() != f.size() * words) return 4;
        for (size_t i = 0; i < f.size(); ++i) {
            std::vector<uint64_t> want;
            if (f[i]) want = f[i]->to_bitmap(n);
            else {   // no filter: every datapoint below n
                want.assign(words, 0);
                for (size_t r = 0; r < n; ++r) want[r >> 6] |= 1ull << (r & 63);
            }
            if (want.size() != words) return 5;
            for (size_t w = 0; w < words; ++w)
                if (block[i * stride + w] != want[w]) {
                    std::printf("n %zu filter %zu word %zu\n", n, i, w);
                    return 6;
                }
        }
    }
    std::printf("filters ok\n");
    return 0;
}
"""


def test_scann_hpp_batched_filters_compile_and_materialise(tmp_path):
    """search_batched_with_filters in the host C++ harness (the flags of build.build_host): it compiles on the tree and
    hasher types, and the strided block it searches with equals the per-filter to_bitmap rows (null = everything)"""
    from scann_rust_amd import build
    build.build()
    src = tmp_path / "filters_test.cpp"
    src.write_text(CPP)
    exe = str(tmp_path / "filters_test")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I" + build.HOST, "-o", exe, str(src), "-L" + build.HERE, "-lscann_hip",
           "-Wl,-rpath," + build.HERE, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "filters ok" in r.stdout, r.stdout + r.stderr

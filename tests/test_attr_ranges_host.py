"""Range filters, the parts that need no GPU: the attribute-table symbols (exported, declared, bound, documented), the
stateless host form scann_hip_allow_bitmaps_from_ranges against the numpy model (tests/attr_range_model.py) on the edge
values of the semantics, the refusals, and scann.hpp's RangeFilter / AttributeTable / search_batched_with_ranges compiled
in the host C++ harness."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import attr_range_cases as RC
from tests import attr_range_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("scann_hip_attr_table_create", "scann_hip_attr_table_destroy", "scann_hip_attr_table_num_datapoints",
               "scann_hip_attr_table_num_columns", "scann_hip_attr_table_column_type",
               "scann_hip_attr_table_allow_bitmaps_device", "scann_hip_attr_table_allow_bitmaps",
               "scann_hip_allow_bitmaps_from_ranges", "scann_hip_search_batched_ranges")
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)
I64_MIN, I64_MAX = RC.I64_MIN, RC.I64_MAX
ROW = M.ROW_INDEX


def _hip():
    from scann_rust_amd import build, hip
    build.build()
    return hip


def test_range_symbols_are_exported_and_documented():
    hip = _hip()
    lib = ctypes.CDLL(hip.LIB_PATH)
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    header = open(os.path.join(ROOT, "include", "scann_hip.h")).read()
    L = hip.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in hip.EXPORTS
        assert getattr(L, name).argtypes is not None, name + " has no argtypes"
        assert re.search(r"\bfn %s\s*\(" % name, text), "INTEGRATION.md lacks " + name
        assert re.search(r"\b%s\s*\(" % name, header)
    # the handle is opaque (no struct body in the header); the bound is an 8-byte union, #[repr(C)] in the Rust block
    assert re.search(r"typedef\s+struct\s+scann_hip_attr_table\s+scann_hip_attr_table\s*;", header)
    assert not re.search(r"struct\s+scann_hip_attr_table\s*\{", header)
    assert "pub struct scann_hip_attr_table { _p: [u8; 0] }" in text
    assert re.search(r"typedef\s+union\s*\{[^}]*int64_t\s+i64;[^}]*float\s+f32;[^}]*uint64_t\s+bits;[^}]*\}\s*scann_hip_range_bound\s*;",
                     header)
    assert re.search(r"#\[repr\(C\)\]\n(#\[derive\([^\n]*\)\]\n)?pub union scann_hip_range_bound \{", text)
    # the constants of header and binding agree
    for name, value in (("ATTR_I64", 1), ("ATTR_F32", 2), ("ATTR_MAX_CLAUSES", 8)):
        assert re.search(r"#define\s+SCANN_HIP_%s\s+%d\b" % (name, value), header) and getattr(hip, name) == value
    assert re.search(r"#define\s+SCANN_HIP_ATTR_ROW_INDEX\s+0xFFFFFFFFu\b", header) and hip.ATTR_ROW_INDEX == 0xFFFFFFFF
    m = re.search(r"#define\s+SCANN_HIP_RANGE_TILE_BITS\s+(\d+)", header)
    assert m and int(m.group(1)) == hip.RANGE_TILE_BITS
    t = hip.RANGE_TILE_BITS
    assert t & (t - 1) == 0 and t >= 128, "a power of two of at least one 16-byte store"
    assert (M.ATTR_I64, M.ATTR_F32, M.ROW_INDEX) == (hip.ATTR_I64, hip.ATTR_F32, hip.ATTR_ROW_INDEX)
    assert (M.AND, M.OR, M.ANDNOT) == (hip.ALLOW_AND, hip.ALLOW_OR, hip.ALLOW_ANDNOT)
    for name in ("AttrTable", "allow_bitmaps_from_ranges", "search_batched_ranges", "_range_bounds"):
        assert hasattr(hip, name)
    for name in ("num_datapoints", "num_columns", "column_type", "allow_bitmaps", "allow_bitmaps_device", "close", "destroy"):
        assert hasattr(hip.AttrTable, name)
    assert "RangeFilter is not built" not in header


def test_range_bounds_packs_eight_byte_words():
    hip = _hip()
    b = hip._range_bounds([hip.ATTR_I64, hip.ATTR_F32, 0], [[-1, 2 ** 53 + 1], [np.float32(-0.0), np.float32(1e-40)], 3],
                          [[I64_MAX, I64_MIN], [np.inf, np.nan], [7, 8]])
    assert b.shape == (2, 3, 2) and b.dtype == np.uint64
    assert b[0, 0, 0] == 2 ** 64 - 1 and b[1, 0, 0] == 2 ** 53 + 1 and b[0, 0, 1] == 2 ** 63 - 1 and b[1, 0, 1] == 2 ** 63
    assert b[0, 1, 0] == 0x80000000 and b[1, 1, 0] == int(np.array(1e-40, np.float32).view(np.uint32))   # f32 in the low four
    assert b[0, 1, 1] == 0x7F800000 and (int(b[1, 1, 1]) & 0x7F800000) == 0x7F800000 and int(b[1, 1, 1]) >> 32 == 0
    assert b[0, 2, 0] == 3 and b[1, 2, 0] == 3 and b[0, 2, 1] == 7 and b[1, 2, 1] == 8


def _raw(hip, n, columns, cols, bounds, nq, op, stride, out, types=None, null_column=None, cols_null=False,
         bounds_null=False, out_null=False):
    """scann_hip_allow_bitmaps_from_ranges with every argument as given (refusal tests pass wrong ones)"""
    L = hip.load()
    arrs = [np.ascontiguousarray(c) for c in columns]
    if types is None:
        types = [hip.ATTR_I64 if a.dtype == np.int64 else hip.ATTR_F32 for a in arrs]
    types = np.array(types, np.int32)
    ptrs = (ctypes.c_void_p * max(len(arrs), 1))(*[None if i == null_column else a.ctypes.data for i, a in enumerate(arrs)])
    cols = np.array(cols, np.uint32)
    b = np.ascontiguousarray(bounds, np.uint64)
    return L.scann_hip_allow_bitmaps_from_ranges(
        n, len(arrs), hip.ptr(types, hip.i32p) if len(arrs) else None, ptrs,
        None if cols_null or not cols.size else hip.ptr(cols, hip.u32p), cols.size,
        None if bounds_null or not b.size else hip.ptr(b, hip.u64p), nq, op, stride,
        None if out_null else hip.ptr(out, hip.u64p))


@pytest.mark.parametrize("name", list(RC.CLAUSE_SETS))
@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_host_from_ranges_matches_the_model(n, extra, name):
    hip = _hip()
    tile = 256   # (the host form has no tile: edges at a few word multiples)
    columns = RC.make_columns(n, tile)
    cols = RC.CLAUSE_SETS[name]
    nq = 10
    lo, hi, kinds = RC.make_bounds(n, tile, columns, cols, nq) if n else ([[0] * len(cols)] * nq, [[0] * len(cols)] * nq, None)
    words = -(-n // 64)
    stride = words + extra
    want = M.allow_bitmaps(n, columns, cols, lo, hi, stride)
    b = RC.pack_bounds(hip, cols, lo, hi)
    out = np.full(nq * stride + 1, SENTINEL)   # op 0 writes every word of the block: gaps come back zero
    assert _raw(hip, n, columns, cols, b, nq, 0, stride, out) == hip.OK
    got = out[:nq * stride].reshape(nq, stride)
    assert np.array_equal(got, want), np.argwhere(got != want)[:3]
    assert np.all(got[:, words:] == 0), "gap words"
    assert out[-1] == SENTINEL, "a word past the block was written"
    assert np.array_equal(hip.allow_bitmaps_from_ranges(n, columns, cols, b, stride), want)
    if n % 64:
        assert np.all(got[:, words - 1] >> np.uint64(n % 64) == 0), "a bit at or past num_datapoints"
    if not cols:
        assert all(RC.popcount(row) == n for row in got), "the empty conjunction allows every row"
    elif n >= 63:   # not vacuous: the point range holds its row, the empty range nothing, the full range every non-NaN row
        pr = RC.point_row(n, tile, columns)
        assert (int(got[0, pr // 64]) >> (pr % 64)) & 1 and not got[1].any() and not got[6].any()
        nan_rows = sum(int(np.isnan(columns[c]).sum()) for c in set(cols) if c in (1, 7))
        assert n - nan_rows <= RC.popcount(got[2]) <= n and (nan_rows == 0 or RC.popcount(got[2]) < n)
        if name in ("i64", "f32", "row", "repeat"):   # (a conjunction over the edge rows' extreme values may hold no row)
            assert 0 < RC.popcount(got[3]) < n
        if any(c in (1, 7) for c in cols):
            assert not got[4].any(), "a NaN bound matched"


def test_i64_compares_as_signed_64_bit_integers():
    hip = _hip()
    col = np.array([I64_MIN, I64_MAX, 2 ** 53, 2 ** 53 + 1, 0, -1, 5, 2 ** 53 + 1, 7, I64_MIN + 1], np.int64)
    n = col.size
    cases = [((2 ** 53 + 1, 2 ** 53 + 1), [3, 7]),          # not rows that hold 2^53: no detour through a double
             ((2 ** 53, 2 ** 53), [2]),
             ((I64_MIN, I64_MIN), [0]), ((I64_MAX, I64_MAX), [1]),
             ((I64_MIN, I64_MAX), list(range(n))),
             ((-1, 5), [4, 5, 6]),                            # both bounds inclusive, equal to stored values
             ((5, -1), []),                                   # lo > hi
             ((I64_MAX, I64_MIN), []),
             ((I64_MIN, I64_MIN + 1), [0, 9])]
    lo = [[c[0][0]] for c in cases]
    hi = [[c[0][1]] for c in cases]
    got = hip.allow_bitmaps_from_ranges(n, [col], [0], RC.pack_bounds(hip, [0], lo, hi))
    for q, (_, rows) in enumerate(cases):
        assert int(got[q, 0]) == sum(1 << r for r in rows), "case %d" % q
    assert np.array_equal(got, M.allow_bitmaps(n, [col], [0], lo, hi))


def test_f32_compares_by_ieee_on_the_stored_value():
    hip = _hip()
    col = np.array([0.0, -0.0, 1e-40, np.inf, -np.inf, np.nan, 1.0, -1e-40, 2.5], np.float32)
    n = col.size
    nan = np.nan
    cases = [((0.0, 0.0), [0, 1]),                 # -0.0 matches [0, 0]; the denormals do not (no flush)
             ((-0.0, -0.0), [0, 1]),
             ((1e-41, 1e-39), [2]),                # a denormal against denormal bounds, as stored
             ((-np.inf, np.inf), [0, 1, 2, 3, 4, 6, 7, 8]),   # every non-NaN row
             ((nan, np.inf), []), ((-np.inf, nan), []), ((nan, nan), []),
             ((np.inf, np.inf), [3]), ((-np.inf, -np.inf), [4]),
             ((1.0, 2.5), [6, 8]),
             ((2.5, 1.0), []),
             ((-1e-40, 0.0), [0, 1, 7])]
    lo = [[np.float32(c[0][0])] for c in cases]
    hi = [[np.float32(c[0][1])] for c in cases]
    # column 1 of RC's numbering is f32: one f32 column at index 1 behind an unused i64 one
    columns = [np.zeros(n, np.int64), col]
    got = hip.allow_bitmaps_from_ranges(n, columns, [1], RC.pack_bounds(hip, [1], lo, hi))
    for q, (_, rows) in enumerate(cases):
        assert int(got[q, 0]) == sum(1 << r for r in rows), "case %d: %s" % (q, bin(int(got[q, 0])))
    assert np.array_equal(got, M.allow_bitmaps(n, columns, [1], lo, hi))
    # a query that does not care ([-inf, +inf]) still excludes the NaN row while the column is among the clauses ...
    both = hip.allow_bitmaps_from_ranges(n, columns, [0, 1], RC.pack_bounds(hip, [0, 1], [[I64_MIN, -np.inf]], [[I64_MAX, np.inf]]))
    assert int(both[0, 0]) == (1 << n) - 1 - (1 << 5)
    # ... and two clauses on one column intersect
    twice = hip.allow_bitmaps_from_ranges(n, columns, [1, 1], RC.pack_bounds(hip, [1, 1], [[0.0, 1.0]], [[2.5, np.inf]]))
    assert int(twice[0, 0]) == (1 << 6) | (1 << 8)


@pytest.mark.parametrize("n", [1, 64, 70, 200])
def test_row_index_is_the_reference_range_filter(n):
    """RangeFilter::new(start, end) is lo = start, hi = (int64_t)end - 1 on the row-index column; no columns needed"""
    hip = _hip()
    ranges = [(0, 0), (0, n), (n - 1, n + 7), (5, 3), (0, 1), (63, 65), (n, n + 1), (0, 2 ** 32 - 1), (2 ** 32 - 1, 0)]
    lo = [[s] for s, _ in ranges]
    hi = [[e - 1] for _, e in ranges]
    stride = -(-n // 64) + 1
    got = hip.allow_bitmaps_from_ranges(n, [], [ROW], RC.pack_bounds(hip, [ROW], lo, hi), stride)
    for q, (s, e) in enumerate(ranges):
        assert np.array_equal(got[q], M.range_filter_bitmap(n, s, e, stride)), "RangeFilter::new(%d, %d)" % (s, e)
    assert not got[0].any() and not got[3].any() and RC.popcount(got[1]) == n and RC.popcount(got[2]) == 1
    assert np.array_equal(got, M.allow_bitmaps(n, [], [ROW], lo, hi, stride))
    # the empty conjunction: every bit below num_datapoints
    none = hip.allow_bitmaps_from_ranges(n, [], [], np.zeros((2, 0, 2), np.uint64), stride)
    assert RC.popcount(none[0]) == n and np.array_equal(none[0], none[1]) and none[0, -1] == 0


@pytest.mark.parametrize("n", [1, 65, 1000, 1024])
def test_host_ops_combine_in_place_and_leave_the_gap(n):
    hip = _hip()
    rng = np.random.default_rng(n)
    tile = 256
    columns = RC.make_columns(n, tile)
    cols = RC.CLAUSE_SETS["mixed"]
    nq = 5
    lo, hi, _ = RC.make_bounds(n, tile, columns, cols, nq, shift=2)
    b = RC.pack_bounds(hip, cols, lo, hi)
    words = -(-n // 64)
    stride = words + 3
    block = rng.integers(0, 2 ** 63, (nq, stride), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (nq, stride), dtype=np.uint64)
    if n % 64:   # an allow-bitmap block: no bit at or past the capacity
        block[:, words - 1] &= np.uint64((1 << (n % 64)) - 1)
    block[:, words:] = SENTINEL
    for op in (hip.ALLOW_AND, hip.ALLOW_OR, hip.ALLOW_ANDNOT):
        want = M.allow_bitmaps(n, columns, cols, lo, hi, stride, op, block)
        got = hip.allow_bitmaps_from_ranges(n, columns, cols, b, stride, op, block.copy())
        assert np.array_equal(got, want), "op %d" % op
        assert np.all(got[:, words:] == SENTINEL), "gap words are not touched"
        assert n < 65 or not np.array_equal(got, block), "op %d changed nothing" % op
        if n % 64:
            assert np.all(got[:, words - 1] >> np.uint64(n % 64) == 0), "a bit at or past num_datapoints"
    got = hip.allow_bitmaps_from_ranges(n, columns, cols, b, stride, 0, block.copy())
    assert np.array_equal(got, M.allow_bitmaps(n, columns, cols, lo, hi, stride)) and np.all(got[:, words:] == 0)


def test_host_from_ranges_refusals():
    hip = _hip()
    n = 130
    columns = [np.arange(n, dtype=np.int64), np.arange(n, dtype=np.float32)]
    out = np.full(2 * 5 + 1, SENTINEL)
    b1 = np.zeros((2, 1, 2), np.uint64)
    call = lambda **kw: _raw(hip, kw.pop("n", n), kw.pop("columns", columns), kw.pop("cols", [0]), kw.pop("bounds", b1), 2,
                             kw.pop("op", 0), kw.pop("stride", 3), out, **kw)
    assert call(n=2 ** 32 - 1, stride=2 ** 26) == hip.OUT_OF_RANGE
    assert call(types=[1, 3]) == hip.INVALID_ARGUMENT and call(types=[0, 2]) == hip.INVALID_ARGUMENT   # an unknown type
    assert call(null_column=1) == hip.INVALID_ARGUMENT                                # a null column with rows
    assert call(cols=[0] * 9, bounds=np.zeros((2, 9, 2), np.uint64)) == hip.UNIMPLEMENTED
    assert call(cols=[2]) == hip.INVALID_ARGUMENT and call(cols=[0xFFFFFFFE]) == hip.INVALID_ARGUMENT
    L = hip.load()
    types = np.array([1, 2], np.int32)
    ptrs = (ctypes.c_void_p * 2)(columns[0].ctypes.data, columns[1].ctypes.data)
    raw = lambda cols_p, bounds_p, out_p, op=0, stride=3, n_cols=1: L.scann_hip_allow_bitmaps_from_ranges(
        n, 2, hip.ptr(types, hip.i32p), ptrs, cols_p, n_cols, bounds_p, 2, op, stride, out_p)
    c0 = np.zeros(1, np.uint32)
    good = (hip.ptr(c0, hip.u32p), hip.ptr(b1, hip.u64p), hip.ptr(out, hip.u64p))
    assert raw(None, good[1], good[2]) == hip.INVALID_ARGUMENT
    assert raw(good[0], None, good[2]) == hip.INVALID_ARGUMENT
    assert raw(good[0], good[1], None) == hip.INVALID_ARGUMENT
    for stride in (0, 2, 2 ** 32):
        assert raw(*good, stride=stride) == hip.INVALID_ARGUMENT
    for op in (hip.ALLOW_NOT, 5, -1, 100):
        assert raw(*good, op=op) == hip.INVALID_ARGUMENT
    assert np.all(out == SENTINEL), "a refused call wrote"
    with pytest.raises(hip.ScannError) as e:
        hip.allow_bitmaps_from_ranges(n, columns, [0], b1, 2)
    assert e.value.code == hip.INVALID_ARGUMENT
    with pytest.raises(ValueError):
        hip.allow_bitmaps_from_ranges(n, [np.arange(n, dtype=np.int32)], [0], b1)   # neither int64 nor float32
    # valid: no columns at all (the row index alone), no rows at all (nothing but gap words), null arrays then allowed
    assert raw(None, None, good[2], n_cols=0) == hip.OK and RC.popcount(out[:3]) == n and out[10] == SENTINEL
    out[:] = SENTINEL
    assert L.scann_hip_allow_bitmaps_from_ranges(0, 2, hip.ptr(types, hip.i32p), None, good[0], 1, good[1], 2, 0, 2, good[2]) == hip.OK
    assert np.all(out[:4] == 0) and np.all(out[4:] == SENTINEL)


def test_attr_table_without_a_gpu_fails_loudly():
    """no quiet host fall-back: without a device the handle cannot be created; with one it reports what it holds"""
    import torch
    hip = _hip()
    columns = [np.arange(10, dtype=np.int64), np.ones(10, np.float32)]
    if torch.cuda.device_count() == 0:
        with pytest.raises(hip.ScannError) as e:
            hip.AttrTable(10, columns)
        assert e.value.code in (hip.UNAVAILABLE, hip.INTERNAL)
    else:
        t = hip.AttrTable(10, columns)
        assert (t.num_datapoints(), t.num_columns()) == (10, 2)
        assert [t.column_type(c) for c in (0, 1, 2)] == [hip.ATTR_I64, hip.ATTR_F32, 0]
        t.close()


CPP = r"""
#include "scann.hpp"
#include <cstdio>
using namespace scann;
int main(int argc, char **argv) {
    // the batched entry exists on the tree and the hasher types, with this signature
    std::vector<NNResultsVector> (TreeXHybridSearcher::*pt)(const std::vector<std::vector<float>> &, size_t,
        const std::vector<uint32_t> &, const std::vector<scann_hip_range_bound> &, const AttributeTable &) const =
        &TreeXHybridSearcher::search_batched_with_ranges;
    std::vector<NNResultsVector> (AsymmetricHasher::*pa)(const std::vector<std::vector<float>> &, size_t,
        const std::vector<uint32_t> &, const std::vector<scann_hip_range_bound> &, const AttributeTable &) const =
        &AsymmetricHasher::search_batched_with_ranges;
    if (!pt || !pa) return 3;
    static_assert(sizeof(scann_hip_range_bound) == 8, "two bounds are 16 bytes");
    const RangeFilter r(3, 70), empty(0, 0), backwards(9, 4);
    const RestrictFilter &f = r;
    if (f.is_allowed(2) || !f.is_allowed(3) || !f.is_allowed(69) || f.is_allowed(70)) return 4;
    if (r.num_allowed() != 67 || empty.num_allowed() != 0 || backwards.num_allowed() != 0) return 5;
    if (empty.is_allowed(0) || backwards.is_allowed(5)) return 6;
    const auto w = r.to_bitmap(100);
    if (w.size() != 2 || w[0] != ~7ull || w[1] != 63ull) return 7;
    if (r.lo_bound().i64 != 3 || r.hi_bound().i64 != 69 || empty.hi_bound().i64 != -1) return 8;
    // the stateless host form under the filter's bounds gives the filter's bitmap
    const uint32_t col = AttributeTable::kRowIndex;
    const scann_hip_range_bound b[2] = {r.lo_bound(), r.hi_bound()};
    uint64_t out[2] = {1, 1};
    if (scann_hip_allow_bitmaps_from_ranges(100, 0, nullptr, nullptr, &col, 1, b, 1, 0, 2, out) != 0) return 9;
    if (out[0] != w[0] || out[1] != w[1]) return 10;
    if (AttributeTable::f32_bound(-0.0f).bits != 0x80000000ull || AttributeTable::i64_bound(-1).bits != ~0ull) return 11;
    std::printf("range filter ok\n");
    if (argc > 1) {   // without a device the upload fails loudly; a default handle makes the search throw
        const std::vector<int64_t> ts = {5, 6, 7};
        try {
            AttributeTable t(context(0), 3, {SCANN_HIP_ATTR_I64}, {ts.data()});
            std::printf("on device %zu %zu %d\n", t.num_datapoints(), t.num_columns(), t.column_type(0));
        } catch (const ScannError &e) {
            std::printf("create failed: %d\n", (int)e.code);
        }
        try {
            detail::run_search_ranges(nullptr, {{1.0f}}, 1, {col}, {b[0], b[1]}, AttributeTable(), scann_hip_search_opts());
            return 12;
        } catch (const ScannError &e) {
            std::printf("search failed: %d\n", (int)e.code);
        }
    }
    return 0;
}
"""


def test_scann_hpp_range_filter_compiles_and_matches_the_model(tmp_path):
    """RangeFilter, AttributeTable and search_batched_with_ranges in the host C++ harness (the flags of build.build_host):
    the reference's is_allowed, the same bitmap as the Python model and the stateless host form; the search entry exists
    on both searcher types and fails loudly without a device table"""
    import torch
    from scann_rust_amd import build
    build.build()
    assert [int(x) for x in M.range_filter_bitmap(100, 3, 70)] == [2 ** 64 - 8, 63]
    src = tmp_path / "range_filter_test.cpp"
    src.write_text(CPP)
    exe = str(tmp_path / "range_filter_test")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I" + build.HOST, "-o", exe, str(src), "-L" + build.HERE, "-lscann_hip",
           "-Wl,-rpath," + build.HERE, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "device"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "range filter ok" in r.stdout, r.stdout + r.stderr
    assert "search failed: %d" % 9 in r.stdout, r.stdout   # FailedPrecondition: no device table
    if torch.cuda.device_count() == 0:
        assert re.search(r"create failed: (13|14)\b", r.stdout), r.stdout   # Internal / Unavailable: never a quiet host table
    else:
        assert "on device 3 1 1" in r.stdout, r.stdout

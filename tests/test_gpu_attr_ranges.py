"""Range filters on the device: the attribute table's bitmap kernel against the stateless host form (bitwise), and end
to end -- a block built on a stream by the table (alone, or ANDed in place into a token map's block) and read by
scann_hip_search_batched_device on the same stream with no synchronisation between them -- against the oracle and
against the search fed the host-built block.  The kernel's blocks are also compared with the numpy model of
tests/attr_range_model.py directly.

Sizes sit on the kernel's edges, with T = RANGE_TILE_BITS: one row, one word less / exactly / more than one bit, one tile
less / exactly / more than one bit, and 2T + 5 (three tiles, the last of one word and five bits).  The columns hold the
edge values of the semantics on both sides of every word and tile edge; the output is pre-filled with a sentinel so
that a word no workgroup wrote, or one it should have left, shows."""
import ctypes

import numpy as np
import pytest
import torch

from scann_rust_amd import hip
from tests import attr_range_cases as RC
from tests import attr_range_model as M
from tests import helpers as H
from tests.test_gpu_filters import K, NQ, Case, _same_rows
from tests.test_gpu_token_map import _check_end_to_end, _search_on_stream

pytestmark = pytest.mark.gpu

T = hip.RANGE_TILE_BITS
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)
DEV = "cuda:0"
ROW = hip.ATTR_ROW_INDEX


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).to(DEV)


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def device_block(table, cols, bounds, nq, stride, op=0, block=None):
    """the device form on torch's current stream into a sentinel-filled block, or into `block`, + one guard word"""
    d_b = _dev(bounds) if bounds.size else None
    init = np.full(nq * stride, SENTINEL) if block is None else block.ravel()
    d_out = _dev(np.concatenate([init, [SENTINEL]]))
    table.allow_bitmaps_device(cols, d_b.data_ptr() if d_b is not None else 0, nq, stride, d_out.data_ptr(), op, _stream())
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint64)
    assert out[-1] == SENTINEL, "a word past the block was written"
    return out[:-1].reshape(nq, stride)


@pytest.fixture(scope="module")
def tables():
    """one (columns, device table) per num_datapoints, shared by the tests below"""
    cache = {}

    def get(n):
        if n not in cache:
            columns = RC.make_columns(n, T)
            cache[n] = (columns, hip.AttrTable(n, columns))
        return cache[n]

    yield get
    for _, t in cache.values():
        t.close()
    cache.clear()


@pytest.mark.parametrize("nq", [1, 5, 33])
@pytest.mark.parametrize("extra", [0, 1, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 5])
def test_device_forms_equal_the_host_form(tables, n, extra, nq):
    columns, table = tables(n)
    assert table.num_datapoints() == n and table.num_columns() == 8
    assert [table.column_type(c) for c in (0, 1, 7, 8)] == [hip.ATTR_I64, hip.ATTR_F32, hip.ATTR_F32, 0]
    words = -(-n // 64)
    stride = words + extra   # (the odd extras make rows that are not 16-byte aligned)
    counts = []
    for shift, (name, cols) in enumerate(RC.CLAUSE_SETS.items()):
        lo, hi, _ = RC.make_bounds(n, T, columns, cols, nq, shift)
        b = RC.pack_bounds(hip, cols, lo, hi)
        want = hip.allow_bitmaps_from_ranges(n, columns, cols, b, stride)
        got = device_block(table, cols, b, nq, stride)
        assert np.array_equal(got, want), "%s device form: first differing word %s" % (name, np.argwhere(got != want)[:1])
        # ... and the numpy model's, which shares no compare with the library (edge rows placed for this tile size)
        assert np.array_equal(got, M.allow_bitmaps(n, columns, cols, lo, hi, stride)), name + " device form vs the model"
        out = np.full((nq, stride), SENTINEL)
        assert table.allow_bitmaps(cols, b, stride, out=out) is out
        assert np.array_equal(out, want), name + " host-pointer handle form"
        assert np.all(want[:, words:] == 0)
        counts += [RC.popcount(row) for row in want]
    # the cases are not vacuous: some bitmap is full, some is empty, some (where there is more than one row) partial
    assert n in counts and 0 in counts and (n == 1 or any(0 < c < n for c in counts))


def test_in_place_ops_leave_the_gap_and_write_rewrites_it(tables):
    n = T + 70
    columns, table = tables(n)
    rng = np.random.default_rng(5)
    words = -(-n // 64)
    nq = 11
    for stride in (words + 2, words + 3):   # 16-byte aligned rows and rows that are not
        block = rng.integers(0, 2 ** 63, (nq, stride), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (nq, stride), dtype=np.uint64)
        block[:, words - 1] &= np.uint64((1 << (n % 64)) - 1)
        block[:, words:] = SENTINEL
        for shift, name in enumerate(("mixed", "eight", "row", "f32")):
            cols = RC.CLAUSE_SETS[name]
            lo, hi, _ = RC.make_bounds(n, T, columns, cols, nq, shift)
            b = RC.pack_bounds(hip, cols, lo, hi)
            for op in (hip.ALLOW_AND, hip.ALLOW_OR, hip.ALLOW_ANDNOT):
                want = hip.allow_bitmaps_from_ranges(n, columns, cols, b, stride, op, block.copy())
                got = device_block(table, cols, b, nq, stride, op, block)
                assert np.array_equal(got, want), "%s op %d" % (name, op)
                assert np.array_equal(got, M.allow_bitmaps(n, columns, cols, lo, hi, stride, op, block)), "%s op %d vs the model" % (name, op)
                assert np.all(got[:, words:] == SENTINEL), "gap words are not touched"
                assert not np.array_equal(got, block), "op %d changed nothing" % op
                assert np.all(got[:, words - 1] >> np.uint64(n % 64) == 0), "a bit at or past num_datapoints"
                assert np.array_equal(table.allow_bitmaps(cols, b, stride, op, block.copy()), want), "host-pointer form"
            got = device_block(table, cols, b, nq, stride, 0, block)
            assert np.array_equal(got, hip.allow_bitmaps_from_ranges(n, columns, cols, b, stride)) and np.all(got[:, words:] == 0)


def test_many_queries_loop_over_the_grid(tables):
    """nq = 65537 at num_datapoints = 130: more query groups than the grid has rows of workgroups; about 1.5 MB"""
    n, nq = 130, 65537
    columns, table = tables(n)
    cols = RC.CLAUSE_SETS["mixed"]
    lo, hi, kinds = RC.make_bounds(n, T, columns, cols, nq, shift=1)
    b = RC.pack_bounds(hip, cols, lo, hi)
    want = hip.allow_bitmaps_from_ranges(n, columns, cols, b)
    assert want.shape == (nq, 3) and kinds[65534] == "point" and want[65534].any() and kinds[65536] == "full" and want[65536].any()
    got = device_block(table, cols, b, nq, 3)
    assert np.array_equal(got, want)


def test_tables_without_columns_or_rows():
    # no columns: the row index alone (the reference's RangeFilter), and the empty conjunction
    n = T + 1
    t = hip.AttrTable(n, [])
    assert t.num_columns() == 0 and t.num_datapoints() == n and t.column_type(0) == 0
    words = -(-n // 64)
    b = RC.pack_bounds(hip, [ROW], [[0], [T - 1], [5], [0]], [[-1], [n + 6], [3], [n - 1]])   # [0, 0), [T - 1, n + 7), 5 > 3, [0, n)
    got = device_block(t, [ROW], b, 4, words + 1)
    assert np.array_equal(got, hip.allow_bitmaps_from_ranges(n, [], [ROW], b, words + 1))
    assert [RC.popcount(r) for r in got] == [0, 2, 0, n]
    every = device_block(t, [], np.zeros((3, 0, 2), np.uint64), 3, words + 1)
    assert [RC.popcount(r) for r in every] == [n, n, n] and not every[:, words:].any()
    t.close()
    # no rows: nothing but gap words, zeroed by a write and left by an op
    t0 = hip.AttrTable(0, [np.zeros(0, np.int64)])
    b = RC.pack_bounds(hip, [0], [[0], [0]], [[1], [1]])
    assert not device_block(t0, [0], b, 2, 3).any()
    assert np.all(device_block(t0, [0], b, 2, 3, hip.ALLOW_OR) == SENTINEL)
    t0.close()


def test_create_and_device_entry_refusals(tables):
    L = hip.load()
    h = ctypes.c_void_p()
    ctx = hip.context(0)
    col = np.zeros(4, np.int64)
    types = np.array([hip.ATTR_I64], np.int32)
    ptrs = (ctypes.c_void_p * 1)(col.ctypes.data)
    assert L.scann_hip_attr_table_create(ctx, 2 ** 32 - 1, 1, hip.ptr(types, hip.i32p), ptrs, ctypes.byref(h)) == hip.OUT_OF_RANGE
    bad = np.array([3], np.int32)
    assert L.scann_hip_attr_table_create(ctx, 4, 1, hip.ptr(bad, hip.i32p), ptrs, ctypes.byref(h)) == hip.INVALID_ARGUMENT
    null = (ctypes.c_void_p * 1)(None)
    assert L.scann_hip_attr_table_create(ctx, 4, 1, hip.ptr(types, hip.i32p), null, ctypes.byref(h)) == hip.INVALID_ARGUMENT
    assert not h.value
    n = 65
    _, table = tables(n)
    d = _dev(np.full(8, SENTINEL))
    d_b = _dev(np.zeros((2, 9, 2), np.uint64))
    st = _stream()

    def call(cols, n_cols, op, stride, bounds=d_b.data_ptr(), out=d.data_ptr()):
        c = np.array(cols, np.uint32)
        return L.scann_hip_attr_table_allow_bitmaps_device(table.h, hip.ptr(c, hip.u32p) if c.size else None, n_cols, bounds, 2,
                                                           op, stride, out, st)

    assert call([0] * 9, 9, 0, 2) == hip.UNIMPLEMENTED
    assert call([8], 1, 0, 2) == hip.INVALID_ARGUMENT and call([0xFFFFFFFE], 1, 0, 2) == hip.INVALID_ARGUMENT
    for stride in (0, 1, 2 ** 32):
        assert call([0], 1, 0, stride) == hip.INVALID_ARGUMENT
        assert call([0], 1, hip.ALLOW_AND, stride) == hip.INVALID_ARGUMENT
    for op in (hip.ALLOW_NOT, 5, -1):
        assert call([0], 1, op, 2) == hip.INVALID_ARGUMENT
    assert call([], 1, 0, 2) == hip.INVALID_ARGUMENT                      # null cols with a clause
    assert call([0], 1, 0, 2, bounds=None) == hip.INVALID_ARGUMENT
    assert call([0], 1, 0, 2, out=None) == hip.INVALID_ARGUMENT
    with pytest.raises(hip.ScannError):
        table.allow_bitmaps([0], np.zeros((2, 1, 2), np.uint64), 1)
    torch.cuda.synchronize()
    assert np.all(d.cpu().numpy().view(np.uint64) == SENTINEL), "a refused call wrote"


# ---- end to end ---------------------------------------------------------------------------------------------------
TENANTS = 8


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(kind):
        if kind not in cache:
            c = Case(kind, 16)
            # an i64 column holding a fixed pseudo-random permutation of the rows and an f32 column derived from it: every
            # range of width >= n / 8 holds the flat hasher's sampled rows (rows j * 16) in proportion
            perm = np.random.default_rng(4242).permutation(c.n).astype(np.int64)
            price = (perm.astype(np.float64) / c.n).astype(np.float32)
            r = np.arange(c.n, dtype=np.int64)
            tenant = ((r + r // 16) % TENANTS).astype(np.uint64)   # (the skew of tests/test_gpu_token_map.py)
            cache[kind] = (c, [perm, price], hip.AttrTable(c.n, [perm, price]), hip.TokenMap(c.n, r.astype(np.uint32), tenant))
        return cache[kind]

    yield get
    for v in cache.values():
        v[2].close()
        v[3].close()
    cache.clear()


def _query_ranges(n, nq):
    """timestamp in a window of n / 4 .. n / 2 rows that moves with the query, AND price <= a cap that cuts the window to
    n / 8 rows or more"""
    a = np.array([(i * 7919) % (n - n // 2) for i in range(nq)], np.int64)
    width = n // 4 + (np.arange(nq, dtype=np.int64) % 5) * (n // 16)
    cap = ((a + n // 8 + (np.arange(nq) % 3) * (n // 32)).astype(np.float64) / n).astype(np.float32)
    return [a, np.full(nq, -np.inf, np.float32)], [a + width, cap]


@pytest.mark.parametrize("kind", ["ah", "txh"])
def test_search_reads_the_block_built_on_its_stream(cases, kind, monkeypatch):
    c, columns, table, tm = cases(kind)
    H.scan_env(monkeypatch, "default")
    index = hip.txh_create(**c.kw)
    o, q = c.opts(), c.q
    n, words = c.n, -(-c.n // 64)
    cols = [0, 1]
    lo, hi = _query_ranges(n, NQ)
    b = hip._range_bounds(table.clause_types(cols), lo, hi)
    # (a) the table's block, built on the stream the search reads it on
    host_block = hip.allow_bitmaps_from_ranges(n, columns, cols, b)
    sizes = [RC.popcount(r) for r in host_block]
    assert min(sizes) >= n // 8 and max(sizes) < n // 2
    d_b = _dev(b)
    d_block = _dev(np.full((NQ, words), SENTINEL))
    build = lambda: table.allow_bitmaps_device(cols, d_b.data_ptr(), NQ, words, d_block.data_ptr(), 0, _stream())
    status, got_a = _search_on_stream(index, q, K, o, d_block, words, n, build)
    assert np.array_equal(d_block.cpu().numpy().view(np.uint64), host_block)
    for i in range(NQ):
        r = got_a[0][i, :got_a[2][i]]
        assert got_a[2][i] == K and np.all((columns[0][r] >= lo[0][i]) & (columns[0][r] <= hi[0][i]) & (columns[1][r] <= hi[1][i])), \
            "q%d: a row outside its ranges" % i
    _check_end_to_end(c, index, host_block, status, got_a, kind + " ranges")

    # (b) a tenant block written by the token map, narrowed in place by a range on the same stream
    lists = [[i % TENANTS] for i in range(NQ)]
    half = [np.array([(i % 2) * (n // 2) for i in range(NQ)], np.int64)], [np.array([(i % 2) * (n // 2) + n // 2 for i in range(NQ)], np.int64)]
    bh = hip._range_bounds([hip.ATTR_I64], *half)
    r = np.arange(n, dtype=np.uint32)
    host_tenant = hip.allow_bitmaps_from_tokens(r, ((r.astype(np.int64) + r // 16) % TENANTS).astype(np.uint64), n, lists)
    host_and = hip.allow_bitmaps_combine(hip.ALLOW_AND, host_tenant, hip.allow_bitmaps_from_ranges(n, columns, [0], bh), n)
    assert np.array_equal(host_and, hip.allow_bitmaps_from_ranges(n, columns, [0], bh, op=hip.ALLOW_AND, out=host_tenant.copy()))
    assert host_and.any() and not np.array_equal(host_and, host_tenant)
    qt, off = hip._token_lists(lists)
    d_tok, d_off, d_bh = _dev(qt), _dev(off), _dev(bh)

    def build_and():
        tm.allow_bitmaps_device(d_tok.data_ptr(), d_off.data_ptr(), NQ, words, d_block.data_ptr(), _stream())
        table.allow_bitmaps_device([0], d_bh.data_ptr(), NQ, words, d_block.data_ptr(), hip.ALLOW_AND, _stream())

    status, got = _search_on_stream(index, q, K, o, d_block, words, n, build_and)
    assert np.array_equal(d_block.cpu().numpy().view(np.uint64), host_and)
    _check_end_to_end(c, index, host_and, status, got, kind + " tenant AND range")

    # (c) the host-pointer entry: the rows of (a); then with one query whose range allows fewer rows than k and one whose
    # range is empty -- short rows, and the batch answered by the host entry under the same block
    _same_rows(table.search_batched(index, q, K, cols, b, o), got_a, kind + " search_batched_ranges")
    assert np.array_equal(hip.search_batched_ranges(index, table, q, K, cols, b, o)[0], table.search_batched(index, q, K, cols, b, o)[0])
    lo2, hi2 = [x.copy() for x in lo], [x.copy() for x in hi]
    lo2[0][3], hi2[0][3], hi2[1][3] = 100, 103, np.inf      # four rows
    lo2[0][5], hi2[0][5] = 9, 8                              # lo > hi
    b2 = hip._range_bounds(table.clause_types(cols), lo2, hi2)
    block2 = hip.allow_bitmaps_from_ranges(n, columns, cols, b2)
    assert RC.popcount(block2[3]) == 4 < K and not block2[5].any()
    gi, gd, gc = table.search_batched(index, q, K, cols, b2, o)
    # (the flat hasher sees all four rows; the tree those in the query's probed leaves)
    found = sorted(columns[0][gi[3, :gc[3]]].tolist())
    assert 0 < gc[3] <= 4 and found == sorted(set(found)) and set(found) <= {100, 101, 102, 103} and gc[5] == 0
    assert kind == "txh" or gc[3] == 4
    assert np.all(gi[3, gc[3]:] == 0xFFFFFFFF) and np.all(gi[5] == 0xFFFFFFFF) and np.all(np.isposinf(gd[5]))
    o.allow_bitmap_stride = words
    try:
        ref = index.search_batched(q, K, o, allow=block2, allow_bits=n)
    finally:
        o.allow_bitmap_stride = 0
    _same_rows((gi, gd, gc), ref, kind + " search_batched_ranges with short rows")
    keep = [i for i in range(NQ) if i not in (3, 5)]
    _same_rows((gi[keep], gd[keep], gc[keep]), tuple(x[keep] for x in got_a), kind + " the other queries")

    # (d) the mismatches
    small = hip.AttrTable(n - 1, [columns[0][:-1], columns[1][:-1]])
    with pytest.raises(hip.ScannError) as e:
        small.search_batched(index, q, K, cols, b, o)
    assert e.value.code == hip.INVALID_ARGUMENT
    small.close()
    one = np.ones(words, np.uint64)
    o.allow_bitmap, o.allow_bitmap_bits = hip.ptr(one, hip.u64p), n
    try:
        with pytest.raises(hip.ScannError) as e:
            table.search_batched(index, q, K, cols, b, o)
        assert e.value.code == hip.INVALID_ARGUMENT
    finally:
        o.allow_bitmap, o.allow_bitmap_bits = None, 0
    with pytest.raises(hip.ScannError) as e:
        table.search_batched(index, q, 0, cols, b, o)
    assert e.value.code == hip.INVALID_ARGUMENT

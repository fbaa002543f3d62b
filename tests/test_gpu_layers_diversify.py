"""Crowding, multi-attribute crowding and MMR over the integer-MFMA prefilter scans.

The stages ask the base for `depth` rows, so the inner search is planned for k = depth = 100 (m = 300), not for the
k = 10 of the answer -- and in tests/test_gpu_crowding.py / test_gpu_diversify.py that inner plan is always the gather
scan (2000 rows, m x 128 > stream).  Here it is forced onto the prefilters, at the shapes of
tests/test_gpu_sp_bitmap.py:
  flat-bitmap    Case("ah", 32, n=4133, nq=65), sp-lanes + SP_PAIRS=64: adc_smfmac_bits_kernel64 + adc_refine_bits_kernel
  flat-lists     the same under SCANN_HIP_SP_BITMAP=0
  tree-sp-words  Case("txh", 32, n=20000, nq=65) under sp-words

Every case is checked two ways, as tests/test_gpu_crowding.py test_hashed_crowded:
  (A) the model over the handle's own plain depth-row search (bitwise);
  (B) the model over the oracle's depth rows, whose depth + 1 distances are strictly increasing (asserted here and, for
      the seeds, in tests/test_layer_checkers.py on the CPU).

Which scan ran.  The HOST entries of the stages run the base search on the primary workspace without touching the
handle's kernel timing (api_search.hip search_device_ws with no device slot), so scann_hip_index_last_kernel_ms does not
report them: the plan is asserted through the plain search with the same nq, depth and opts on the same handle, and --
the workspace IS reported -- through debug_survivor_bitmap_bytes right after the stage's call on a fresh handle (bitmaps
of the call's size under the bitmap form, none under the lists).  The DEVICE entries are named by the handle."""
import ctypes

import numpy as np
import pytest

import diversify_model as DM
import helpers as H
from oracle import pyoracle as orc
from scann_rust_amd import hip
from test_gpu_crowding import check_rows
from test_gpu_diversify import _ptr, _two_streams, check_against, plain_rows
from test_gpu_filters import Case
from test_gpu_sp_bitmap import _bitmap_bytes, _knob

pytestmark = pytest.mark.gpu

K, DEPTH, M = 10, 100, 300
LIMITS = (1, 3)
FORMS = {   # name: (index kind, _knob arguments, kernel, survivor bitmaps)
    "flat-bitmap": ("ah", dict(value=None), "adc_smfmac_kernel", True),
    "flat-lists": ("ah", dict(value="0"), "adc_smfmac_kernel", False),
    "tree-sp-words": ("txh", dict(value=None, pairs=None, scan="sp-words"), "adc_smfmac_kernel", False),
}
SHAPES = {"ah": dict(n=4133, nq=65), "txh": dict(n=20000, nq=65)}
# seeds of the "f50" filters for which no oracle row of 101 entries holds equal neighbours, on either index (picked on
# the CPU; tests/test_layer_checkers.py asserts it without a GPU): the shared bitmap, and query i's own (seed + i)
SHARED_SEED, PER_QUERY_SEED = 3, 400


def oracle_row(c, i, depth, allowed=None):
    """(idx, dist, depth + 1 distances) of the oracle's row of query i at k = depth, m = M, over the rows `allowed`
    (ascending datapoint indices; None: all)"""
    if c.kind == "ah":
        codes, data = c.codes, c.data.reshape(c.n, c.stride)
        if allowed is not None:
            codes, data = np.ascontiguousarray(codes[allowed]), np.ascontiguousarray(data[allowed])
        oi, od = orc.ah_search_with_reordering(c.cb, codes, data, c.stride, c.q[i], depth + 1, M)
        if allowed is not None:
            oi = allowed[oi].astype(np.uint32)
        return oi[:depth], od[:depth], od
    keep = c.oix.pre_reorder_multiplier
    try:
        c.oix.pre_reorder_multiplier = float(M) / depth
        assert orc.pre_reorder_k(depth, c.oix.pre_reorder_multiplier) == M
        c.oix.allow = None if allowed is None else H.words_of(allowed, c.n)[0]
        r = orc.txh_search(c.oix, c.q[i], depth, stages=True)
    finally:
        c.oix.allow = None
        c.oix.pre_reorder_multiplier = keep
    more = orc.reorder(c.data, c.stride, c.dim, c.q[i], r[4], depth + 1)
    return r[0], r[1], more[1]


def oracle_rows(c, depth=DEPTH, allowed=None):
    """the rows of every query; `allowed`: None, one array for the batch, or one per query.  Tie-free: asserted."""
    nq = c.q.shape[0]
    per_query = isinstance(allowed, list)
    rows = [oracle_row(c, i, depth, allowed[i] if per_query else allowed) for i in range(nq)]
    for i, r in enumerate(rows):
        assert np.all(np.diff(r[2]) > 0), "the oracle's row of query %d has tied neighbours" % i
    return rows


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(kind):
        if kind not in cache:
            c = Case(kind, 32, **SHAPES[kind])
            cache[kind] = (c, oracle_rows(c))
        return cache[kind]

    yield get
    cache.clear()


def _create(form, cases, monkeypatch):
    kind, knob, name, bitmap = FORMS[form]
    c, orows = cases(kind)
    _knob(monkeypatch, **knob)
    index = hip.txh_create(**c.kw)
    index.enable_timing(True)
    return c, orows, index, name, (_bitmap_bytes(c.n, c.q.shape[0]) if bitmap else 0)


def _attrs(n):
    i = np.arange(n, dtype=np.uint64)
    return i % np.uint64(7), ((i % np.uint64(13)) << np.uint64(32)) | np.uint64(1)


def _plain(index, c, name, **allow):
    """the handle's own depth rows, on the scan under test"""
    plain = index.search_batched(c.q, DEPTH, c.opts(M), **allow)
    assert index.last_kernel_ms()[1] == name, index.last_kernel_ms()[1]
    return plain


# ---- host entries ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(FORMS))
def test_crowded_host(form, cases, monkeypatch):
    c, orows, index, name, want_bytes = _create(form, cases, monkeypatch)
    nq = c.q.shape[0]
    a7, a13 = _attrs(c.n)
    index.set_crowding_attributes(a7)
    first = index.search_crowded(c.q, K, DEPTH, 1, opts=c.opts(M))       # the stage's call sizes the fresh workspace
    assert index.debug_survivor_bitmap_bytes() == want_bytes
    plain = _plain(index, c, name)
    assert index.debug_survivor_bitmap_bytes() == want_bytes
    for attrs in (a7, a13):
        index.set_crowding_attributes(attrs)
        for limit in LIMITS:
            got = index.search_crowded(c.q, K, DEPTH, limit, opts=c.opts(M))
            check_rows(got, plain_rows(plain), attrs, limit, K, nq, ("A", form, limit))
            check_rows(got, lambda i: orows[i][:2], attrs, limit, K, nq, ("B", form, limit))
    check_rows(first, plain_rows(plain), a7, 1, K, nq, ("A", form, "first call"))


@pytest.mark.parametrize("form", sorted(FORMS))
def test_crowded_md_host(form, cases, monkeypatch):
    c, orows, index, name, want_bytes = _create(form, cases, monkeypatch)
    nq = c.q.shape[0]
    a7, a13 = _attrs(c.n)
    attrs = np.stack([a7, a13, np.arange(c.n, dtype=np.uint64) % np.uint64(2)])
    index.set_crowding_attributes_md(attrs)
    index.search_crowded_md(c.q, K, DEPTH, [1, 1, 1], opts=c.opts(M))
    assert index.debug_survivor_bitmap_bytes() == want_bytes
    plain = _plain(index, c, name)
    for limits in ([1, 1, 1], [3, 3, 3], [3, 1, 2 ** 32 - 1]):
        got = index.search_crowded_md(c.q, K, DEPTH, limits, opts=c.opts(M))
        check_against(got, nq, K, plain_rows(plain), lambda i: orows[i][:2],
                      lambda ri, rd: DM.md_apply(ri, rd, attrs, limits, K), (form, limits))


@pytest.mark.parametrize("form", sorted(FORMS))
def test_mmr_host(form, cases, monkeypatch):
    """f32 rows.  (A base whose re-rank rows are bf16 has no MMR: scann_hip_search_mmr refuses quantized rows, which
    tests/test_gpu_quantized_rerank.py test_entry_points_that_refuse_quantized_rows pins.)"""
    c, orows, index, name, want_bytes = _create(form, cases, monkeypatch)
    nq = c.q.shape[0]
    index.search_mmr(c.q, K, DEPTH, 0.5, opts=c.opts(M))
    assert index.debug_survivor_bitmap_bytes() == want_bytes
    plain = _plain(index, c, name)
    for lam in (0.25, 0.7):
        got = index.search_mmr(c.q, K, DEPTH, lam, opts=c.opts(M))
        check_against(got, nq, K, plain_rows(plain), lambda i: orows[i][:2],
                      lambda ri, rd: DM.mmr_apply_rows(ri, rd, K, lam, c.data, c.stride, c.dim, hip.SQUARED_L2)[:2],
                      (form, lam))
        assert np.array_equal(got[0][:, 0], plain[0][:, 0])


# ---- device entries, two streams ------------------------------------------------------------------------------------
def _device_named(index, name, want_bytes, seen):
    """after a _two_streams run whose calls noted their streams in `seen` (emptied here)"""
    assert index.last_kernel_ms()[1] == name, index.last_kernel_ms()[1]
    assert len(set(seen)) == 2
    for st in set(seen):
        assert index.debug_survivor_bitmap_bytes(st) == want_bytes, "the workspace of stream %x" % st
    del seen[:]


@pytest.mark.parametrize("form", sorted(FORMS))
def test_device_entries_two_streams(form, cases, monkeypatch):
    """scann_hip_search_crowded_device, _crowded_md_device and _mmr_device after their reserve, on two streams each:
    the host entry's rows (which the tests above hold against the model), no allocation, status Ok; the handle names
    the scan, and each stream's workspace holds the form's survivor bitmaps"""
    c, orows, index, name, want_bytes = _create(form, cases, monkeypatch)
    nq, L = c.q.shape[0], hip.load()
    a7, a13 = _attrs(c.n)
    index.set_crowding_attributes(a7)
    index.set_crowding_attributes_md(np.stack([a7, a13]))
    o = c.opts(M)
    seen = []

    def crowded(limit, qd, out, st):
        seen.append(st)
        hip.check(L.scann_hip_search_crowded_device(index.h, ctypes.c_void_p(_ptr(qd)), nq, c.dim, K, DEPTH, limit,
                                                    ctypes.byref(o), ctypes.c_void_p(_ptr(out[0])),
                                                    ctypes.c_void_p(_ptr(out[1])), ctypes.c_void_p(_ptr(out[2])),
                                                    ctypes.c_void_p(st)))

    def md(limits, qd, out, st):
        seen.append(st)
        index.search_crowded_md_device(_ptr(qd), nq, c.dim, K, DEPTH, list(limits), _ptr(out[0]), _ptr(out[1]),
                                       _ptr(out[2]), st, opts=o)

    def mmr(lam, qd, out, st):
        seen.append(st)
        index.search_mmr_device(_ptr(qd), nq, c.dim, K, DEPTH, lam, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), st, opts=o)

    reserve = lambda: hip.check(L.scann_hip_index_reserve_crowded(index.h, nq, K, DEPTH, ctypes.byref(o)))
    _two_streams(index, c.q, nq, K, DEPTH, host=lambda limit: index.search_crowded(c.q, K, DEPTH, limit, opts=c.opts(M)),
                 device=crowded, reserve=reserve, params=list(LIMITS), opts=o)
    _device_named(index, name, want_bytes, seen)
    _two_streams(index, c.q, nq, K, DEPTH,
                 host=lambda lim: index.search_crowded_md(c.q, K, DEPTH, list(lim), opts=c.opts(M)),
                 device=md, reserve=reserve, params=[(1, 1), (3, 3)], opts=o)
    _device_named(index, name, want_bytes, seen)
    _two_streams(index, c.q, nq, K, DEPTH, host=lambda lam: index.search_mmr(c.q, K, DEPTH, lam, opts=c.opts(M)),
                 device=mmr, reserve=lambda: index.reserve_mmr(nq, K, DEPTH, opts=o), params=[0.25, 0.7], opts=o)
    _device_named(index, name, want_bytes, seen)


# ---- allow-lists ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(FORMS))
def test_crowded_with_a_shared_allow_list(form, cases, monkeypatch):
    """one bitmap for the batch (about half of the points) through the crowded host entry: (A) over the handle's
    filtered plain rows, (B) over the oracle's rows under the same filter; no disallowed index"""
    c, _, index, name, want_bytes = _create(form, cases, monkeypatch)
    nq = c.q.shape[0]
    words, cap = c.family("f50", seed=SHARED_SEED)
    allowed = H.allowed_ids(words, cap, c.n)
    orows = oracle_rows(c, allowed=allowed)
    a7, _ = _attrs(c.n)
    index.set_crowding_attributes(a7)
    index.search_crowded(c.q, K, DEPTH, 1, opts=c.opts(M), allow=words, allow_bits=cap)
    assert index.debug_survivor_bitmap_bytes() == want_bytes
    plain = _plain(index, c, name, allow=words, allow_bits=cap)
    ok = np.zeros(c.n, bool)
    ok[allowed] = True
    for limit in LIMITS:
        got = index.search_crowded(c.q, K, DEPTH, limit, opts=c.opts(M), allow=words, allow_bits=cap)
        check_rows(got, plain_rows(plain), a7, limit, K, nq, ("A", form, "shared", limit))
        check_rows(got, lambda i: orows[i][:2], a7, limit, K, nq, ("B", form, "shared", limit))
        assert ok[got[0][got[0] != 0xFFFFFFFF]].all()


@pytest.mark.parametrize("form", sorted(FORMS))
def test_crowded_device_with_one_allow_list_per_query(form, cases, monkeypatch):
    """allow_bitmap_stride through scann_hip_search_crowded_device: every query its own random half of the points, as a
    device block of nq bitmaps.  (A) over the handle's plain rows under the same block, (B) over the oracle's rows of
    each query's own subset; a query filtered by its neighbour's bitmap would return a disallowed index."""
    import torch
    c, _, index, name, want_bytes = _create(form, cases, monkeypatch)
    nq, L = c.q.shape[0], hip.load()
    block = np.stack([c.family("f50", seed=PER_QUERY_SEED + i)[0] for i in range(nq)])
    assert len({b.tobytes() for b in block}) == nq
    allowed = [H.allowed_ids(block[i], c.n, c.n) for i in range(nq)]
    orows = oracle_rows(c, allowed=allowed)
    a7, _ = _attrs(c.n)
    index.set_crowding_attributes(a7)
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    qd = torch.from_numpy(np.ascontiguousarray(c.q)).to(dev)
    da = torch.from_numpy(np.ascontiguousarray(block).view(np.int64).copy()).to(dev)
    o = c.opts(M)
    o.allow_bitmap = ctypes.cast(ctypes.c_void_p(da.data_ptr()), ctypes.POINTER(ctypes.c_uint64))
    o.allow_bitmap_bits, o.allow_bitmap_stride = c.n, block.shape[1]
    hip.check(L.scann_hip_index_reserve_crowded(index.h, nq, K, DEPTH, ctypes.byref(o)))
    got = {}
    for limit in LIMITS:
        oi = torch.zeros((nq, K), dtype=torch.int32, device=dev)
        od = torch.zeros((nq, K), dtype=torch.float32, device=dev)
        oc = torch.zeros(nq, dtype=torch.int32, device=dev)
        hip.check(L.scann_hip_search_crowded_device(index.h, ctypes.c_void_p(qd.data_ptr()), nq, c.dim, K, DEPTH, limit,
                                                    ctypes.byref(o), ctypes.c_void_p(oi.data_ptr()),
                                                    ctypes.c_void_p(od.data_ptr()), ctypes.c_void_p(oc.data_ptr()),
                                                    ctypes.c_void_p(st)))
        assert L.scann_hip_index_last_device_status(index.h, ctypes.c_void_p(st)) == hip.OK
        torch.cuda.synchronize()
        assert index.last_kernel_ms()[1] == name
        assert index.debug_survivor_bitmap_bytes(st) == want_bytes
        got[limit] = (oi.cpu().numpy().view(np.uint32), od.cpu().numpy(), oc.cpu().numpy().view(np.uint32))
    o.allow_bitmap, o.allow_bitmap_bits, o.allow_bitmap_stride = None, 0, 0
    plain = _plain(index, c, name, allow=block, allow_bits=c.n)
    for limit in LIMITS:
        check_rows(got[limit], plain_rows(plain), a7, limit, K, nq, ("A", form, "per query", limit))
        check_rows(got[limit], lambda i: orows[i][:2], a7, limit, K, nq, ("B", form, "per query", limit))
        for i in range(nq):
            row = got[limit][0][i]
            assert np.isin(row[row != 0xFFFFFFFF], allowed[i]).all(), "q%d: an index its own bitmap does not allow" % i

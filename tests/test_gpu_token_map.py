"""Tag filters on the device: the token map's bitmap kernel and the block-combination kernel against their stateless host
forms (bitwise), and end to end -- a block built on a stream by the token map and read by
scann_hip_search_batched_device on the same stream with no synchronisation between them -- against the oracle and
against the search fed the host-built block.

Sizes sit on the kernel's edges, with T = TOKEN_TILE_BITS: one word, one tile less / exactly / more than one bit, and
2T + 5 (three tiles, the last of one word and five bits).  Postings place ids on both sides of every tile edge; the
output is pre-filled with a sentinel so that a word no workgroup wrote shows."""
import ctypes

import numpy as np
import pytest
import torch

from scann_rust_amd import hip
from tests import helpers as H
from tests.test_gpu_filters import K, NQ, Case, _same_rows
from tests.token_map_model import TokenMapModel

pytestmark = pytest.mark.gpu

T = hip.TOKEN_TILE_BITS
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)
U64_MAX = 2 ** 64 - 1
DEV = "cuda:0"
# tokens of the synthetic map
EDGES, WORD, SPAN, ALL, OUTSIDE, MANY0 = 3, 4, 5, 6, 8, 5000


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).to(DEV)


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def make_pairs(n, seed=0):
    """(indices, tokens), shuffled: ids on the tile edges, a posting inside one word, one across every tile, a token
    that holds every row, a token with only out-of-range ids, 300 short postings, duplicates"""
    rng = np.random.default_rng([n, seed])
    parts = []
    add = lambda ids, t: parts.append((np.asarray(ids, np.int64), np.full(len(ids), t, np.uint64)))
    add([0, T - 1, T, T + 63, 2 * T, n - 1, n, n + 63, 0xFFFFFFFF, 0, n - 1], EDGES)   # (ids >= n are dropped by create)
    w = max(n - 2, 0) // 64 * 64   # (the last word that holds more than one row)
    add([i for i in (w + 1, w + 3, w + 62, w + 3) if i < n], WORD)
    add(np.arange(n - 1, -1, -97), SPAN)
    add(np.arange(n), ALL)
    add([n, n + 1, 0xFFFFFFFF], OUTSIDE)
    add(rng.integers(0, n, 50), 0)
    add(rng.integers(0, n, 50), U64_MAX)
    for j in range(300):
        add(rng.integers(0, n, 3), MANY0 + j)
    idx = np.concatenate([p[0] for p in parts])
    tok = np.concatenate([p[1] for p in parts])
    order = rng.permutation(idx.size)
    return idx[order].astype(np.uint32), tok[order]


def make_lists(nq):
    many = list(range(MANY0, MANY0 + 300))   # more tokens than a workgroup has threads
    kinds = [[EDGES, WORD], [ALL], many + [424242, EDGES, EDGES], [], [SPAN, 777, SPAN, 0, U64_MAX, OUTSIDE]]
    if nq == 1:
        return [kinds[0] + kinds[2] + kinds[4]]
    return [kinds[i % len(kinds)] for i in range(nq)]


def device_block(tm, lists, stride):
    """the device form on torch's current stream into a sentinel-filled block (+ one guard word)"""
    tok, off = hip._token_lists(lists)
    nq = off.size - 1
    d_tok, d_off = _dev(tok if tok.size else np.zeros(1, np.uint64)), _dev(off)
    d_out = _dev(np.full(nq * stride + 1, SENTINEL))
    tm.allow_bitmaps_device(d_tok.data_ptr(), d_off.data_ptr(), nq, stride, d_out.data_ptr(), _stream())
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint64)
    assert out[-1] == SENTINEL, "a word past the block was written"
    return out[:-1].reshape(nq, stride)


@pytest.fixture(scope="module")
def maps():
    """one (pairs, host model, device map) per num_datapoints, shared by the tests below"""
    cache = {}

    def get(n):
        if n not in cache:
            idx, tok = make_pairs(n)
            cache[n] = (idx, tok, hip.TokenMap(n, idx, tok))
        return cache[n]

    yield get
    for _, _, tm in cache.values():
        tm.close()
    cache.clear()


@pytest.mark.parametrize("nq", [1, 5])
@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("n", [1, 64, 65, T - 1, T, T + 1, 2 * T + 5])
def test_device_forms_equal_the_host_form(maps, n, extra, nq):
    idx, tok, tm = maps(n)
    lists = make_lists(nq)
    words = -(-n // 64)
    stride = words + extra
    want = hip.allow_bitmaps_from_tokens(idx, tok, n, lists, stride)
    got = device_block(tm, lists, stride)
    assert np.array_equal(got, want), "device form: first differing word %s" % (np.argwhere(got != want)[:1],)
    assert np.array_equal(tm.allow_bitmaps(lists, stride), want), "host-pointer handle form"
    assert np.all(want[:, words:] == 0)
    # the cases are not vacuous
    if nq == 5:
        full = want[1, :words].copy()
        assert all(bin(int(w)).count("1") == 64 for w in full[:n // 64]) and not want[3].any()
        assert want[0].any() and want[2].any() and want[4].any()


def test_empty_map_and_empty_lists(maps):
    n = T + 1
    tm = hip.TokenMap(n, np.zeros(0, np.uint32), np.zeros(0, np.uint64))
    assert tm.num_tokens() == 0 and tm.num_datapoints() == n and tm.get_indices(5).size == 0
    words = -(-n // 64)
    got = device_block(tm, [[1, 2], [], [U64_MAX]], words + 3)
    assert not got.any()
    assert not tm.allow_bitmaps([[1, 2], []]).any()
    tm.close()
    # a populated map, every list empty (no token array is read)
    _, _, tm = maps(65)
    assert not device_block(tm, [[], [], []], 2).any()
    # capacity 0: nothing but gap words
    tm0 = hip.TokenMap(0, [0, 1], [5, 5])
    assert tm0.num_tokens() == 1 and tm0.get_indices(5).size == 0
    assert not device_block(tm0, [[5], []], 3).any()
    tm0.close()


def test_many_queries_loop_over_the_grid(maps):
    """nq = 65537 > the grid's y extent at num_datapoints = 130: about 1.5 MB of bitmaps"""
    n, nq = 130, 65537
    idx, tok, tm = maps(n)
    kinds = [[EDGES], [SPAN, WORD], [], [0, U64_MAX], [MANY0, MANY0 + 1, MANY0 + 2], [OUTSIDE, 31337], [WORD]]
    lists = [kinds[(i + 2) % 7] for i in range(nq)]   # (queries 65535 and 65536, past the grid, name tokens)
    want = hip.allow_bitmaps_from_tokens(idx, tok, n, lists)
    assert want.shape == (nq, 3) and want[65535].any() and want[65536].any()
    got = device_block(tm, lists, 3)
    assert np.array_equal(got, want)


def test_get_indices_and_num_tokens_match_the_model(maps):
    n = T + 70
    idx, tok, tm = maps(n)
    model = TokenMapModel(n).add_pairs(idx, tok)
    assert tm.num_tokens() == model.num_tokens() == 307 and tm.num_datapoints() == n
    for t in (EDGES, WORD, SPAN, OUTSIDE, 0, U64_MAX, MANY0, MANY0 + 299, 424242):
        assert np.array_equal(tm.get_indices(t), model.stored_posting(t)), "token %d" % t
    assert tm.get_indices(OUTSIDE).size == 0 and model.get_indices(OUTSIDE) is not None   # known, nothing in range
    assert np.array_equal(tm.get_indices(EDGES), [0, T - 1, T, T + 63, n - 1])
    assert np.array_equal(tm.get_indices(ALL), np.arange(n))
    # a short buffer: ResourceExhausted, the count reported, nothing written
    L = hip.load()
    out, cnt = np.full(8, 0xFFFFFFFF, np.uint32), ctypes.c_uint64(0)
    assert L.scann_hip_token_map_get_indices(tm.h, EDGES, hip.ptr(out, hip.u32p), 4, ctypes.byref(cnt)) == hip.RESOURCE_EXHAUSTED
    assert cnt.value == 5 and np.all(out == 0xFFFFFFFF)
    assert L.scann_hip_token_map_get_indices(tm.h, 424242, None, 0, ctypes.byref(cnt)) == hip.OK and cnt.value == 0


def test_create_and_block_refusals(maps):
    L = hip.load()
    h = ctypes.c_void_p()
    one32, one64 = np.zeros(1, np.uint32), np.zeros(1, np.uint64)
    ctx = hip.context(0)
    assert L.scann_hip_token_map_create(ctx, 2 ** 32 - 1, hip.ptr(one32, hip.u32p), hip.ptr(one64, hip.u64p), 1,
                                        ctypes.byref(h)) == hip.OUT_OF_RANGE
    assert L.scann_hip_token_map_create(ctx, 10, None, hip.ptr(one64, hip.u64p), 1, ctypes.byref(h)) == hip.INVALID_ARGUMENT
    assert L.scann_hip_token_map_create(ctx, 10, hip.ptr(one32, hip.u32p), None, 1, ctypes.byref(h)) == hip.INVALID_ARGUMENT
    assert not h.value
    _, _, tm = maps(65)
    d = _dev(np.full(8, SENTINEL))
    off = _dev(np.array([0, 0], np.uint64))
    for stride in (1, 0, 2 ** 32):
        assert L.scann_hip_token_map_allow_bitmaps_device(tm.h, None, off.data_ptr(), 1, stride, d.data_ptr(),
                                                          _stream()) == hip.INVALID_ARGUMENT
    with pytest.raises(hip.ScannError):
        tm.allow_bitmaps([[1]], 1)
    torch.cuda.synchronize()
    assert np.all(d.cpu().numpy().view(np.uint64) == SENTINEL), "a refused call wrote"


# ---- combining blocks ---------------------------------------------------------------------------------------------
def _rand_block(nq, stride, rng):
    return rng.integers(0, 2 ** 63, (nq, stride), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (nq, stride), dtype=np.uint64)


@pytest.mark.parametrize("bits", [1, 65, 1000, T + 70])
@pytest.mark.parametrize("op", [hip.ALLOW_AND, hip.ALLOW_OR, hip.ALLOW_ANDNOT, hip.ALLOW_NOT])
def test_device_combine_equals_the_host_form(op, bits):
    """per-query and shared operands, even strides (16 bytes a lane) and odd ones (8), gap words untouched, out = a"""
    rng = np.random.default_rng([op, bits])
    words = -(-bits // 64)
    nq = 5
    even = words + (words & 1)
    for sa, sb, so in ((even, even, even), (even + 2, even, even + 4), (words + 1 - (words & 1), even, even),
                       (0, even, even + 2), (even, 0, even), (0, words | 1, words | 1)):
        a = _rand_block(nq if sa else 1, sa or even, rng)
        b = _rand_block(nq if sb else 1, sb or even, rng)
        out = np.full((nq, so), SENTINEL)
        want = hip.allow_bitmaps_combine(op, a if sa else a[0], None if op == hip.ALLOW_NOT else (b if sb else b[0]), bits,
                                         out=out.copy())
        da, db, do = _dev(a), _dev(b), _dev(out)
        hip.allow_bitmaps_combine_device(op, da.data_ptr(), sa, 0 if op == hip.ALLOW_NOT else db.data_ptr(), sb, nq, bits,
                                         do.data_ptr(), so, _stream())
        torch.cuda.synchronize()
        got = do.cpu().numpy().view(np.uint64)
        assert np.array_equal(got, want), "op %d strides %s" % (op, (sa, sb, so))
        assert np.all(got[:, words:] == SENTINEL)
    # in place: d_out is d_a, same stride
    a, b = _rand_block(nq, even, rng), _rand_block(nq, even, rng)
    want = hip.allow_bitmaps_combine(op, a, b, bits, out=a.copy())
    da, db = _dev(a), _dev(b)
    hip.allow_bitmaps_combine_device(op, da.data_ptr(), even, db.data_ptr(), even, nq, bits, da.data_ptr(), even, _stream())
    torch.cuda.synchronize()
    assert np.array_equal(da.cpu().numpy().view(np.uint64), want)
    L = hip.load()
    assert L.scann_hip_allow_bitmaps_combine_device(hip.context(0), 9, da.data_ptr(), even, db.data_ptr(), even, nq, bits,
                                                    da.data_ptr(), even, _stream()) == hip.INVALID_ARGUMENT
    if words > 1:
        assert L.scann_hip_allow_bitmaps_combine_device(hip.context(0), op, da.data_ptr(), words - 1, db.data_ptr(), even, nq,
                                                        bits, da.data_ptr(), even, _stream()) == hip.INVALID_ARGUMENT


# ---- end to end ---------------------------------------------------------------------------------------------------
TENANTS, CATS = 8, 16
CAT0 = 1000


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(kind):
        if kind not in cache:
            c = Case(kind, 16)
            r = np.arange(c.n, dtype=np.int64)
            # tenant: eight disjoint classes, skewed so that the flat hasher's threshold sample (rows j * 16) meets
            # every class (tests/test_gpu_query_filters.py); category: sixteen pseudo-random classes
            tenant = (r + r // 16) % TENANTS
            cat = np.random.default_rng(77).integers(0, CATS, c.n)
            idx = np.concatenate([r, r]).astype(np.uint32)
            tok = np.concatenate([tenant, CAT0 + cat]).astype(np.uint64)
            cache[kind] = (c, idx, tok, hip.TokenMap(c.n, idx, tok))
        return cache[kind]

    yield get
    for v in cache.values():
        v[3].close()
    cache.clear()


def _search_on_stream(index, q, k, o, d_block, stride, bits, build):
    """build() enqueues the block's kernels on torch's current stream; the search is enqueued right behind them, with
    no synchronisation in between"""
    L = hip.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    nq, dim = q.shape
    qd = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(DEV)
    oi = torch.full((nq, k), -1, dtype=torch.int32, device=DEV)
    od = torch.zeros((nq, k), dtype=torch.float32, device=DEV)
    oc = torch.full((nq,), 7, dtype=torch.int32, device=DEV)
    st = ctypes.c_void_p(_stream())
    o.allow_bitmap = ctypes.cast(ctypes.c_void_p(d_block.data_ptr()), ctypes.POINTER(ctypes.c_uint64))
    o.allow_bitmap_bits, o.allow_bitmap_stride = bits, stride
    torch.cuda.synchronize()
    try:
        build()
        hip.check(L.scann_hip_search_batched_device(index.h, p(qd), nq, dim, k, ctypes.byref(o), p(oi), p(od), p(oc), st))
        status = L.scann_hip_index_last_device_status(index.h, st)
        torch.cuda.synchronize()
    finally:
        o.allow_bitmap, o.allow_bitmap_bits, o.allow_bitmap_stride = None, 0, 0
    return status, (oi.cpu().numpy().view(np.uint32), od.cpu().numpy(), oc.cpu().numpy().view(np.uint32))


def _check_end_to_end(c, index, host_block, status, got, what):
    """the token route's rows: those of the search fed the host-built block (device entry), and the oracle's under the
    same per-query filter, every query"""
    o, q = c.opts(), c.q
    assert status == hip.OK, "%s: device status %d" % (what, status)
    o.allow_bitmap_stride = host_block.shape[1]
    try:
        rstatus, ri, rd, rc = H.device_search(index, q, K, o, allow=host_block, allow_bits=c.n)
    finally:
        o.allow_bitmap_stride = 0
    assert rstatus == hip.OK
    _same_rows(got, (ri, rd, rc), what + " vs host-built block")
    staged = index.search_batched(q, K, o, stages=True, allow=host_block, allow_bits=c.n)
    idx, dist, cnt, (tok, tokd, ci, cd, cc) = staged
    for i in range(q.shape[0]):
        s = slice(i, i + 1)
        c.check(q[s], host_block[i], c.n, (idx[s], dist[s], cnt[s], (tok[s], tokd[s], ci[s], cd[s], cc[s])), (0,),
                "%s q%d" % (what, i))
    _same_rows(got, staged[:3], what + " vs oracle-checked rows")


@pytest.mark.parametrize("kind", ["ah", "txh"])
def test_search_reads_the_block_built_on_its_stream(cases, kind, monkeypatch):
    c, idx, tok, tm = cases(kind)
    H.scan_env(monkeypatch, "default")
    index = hip.txh_create(**c.kw)
    o, q = c.opts(), c.q
    words = -(-c.n // 64)
    # one attribute: query i is tenant i % 8
    lists = [[i % TENANTS] for i in range(NQ)]
    host_block = hip.allow_bitmaps_from_tokens(idx, tok, c.n, lists)
    qt, off = hip._token_lists(lists)
    d_tok, d_off = _dev(qt), _dev(off)
    d_block = _dev(np.full((NQ, words), SENTINEL))
    build = lambda: tm.allow_bitmaps_device(d_tok.data_ptr(), d_off.data_ptr(), NQ, words, d_block.data_ptr(), _stream())
    status, got = _search_on_stream(index, q, K, o, d_block, words, c.n, build)
    assert np.array_equal(d_block.cpu().numpy().view(np.uint64), host_block)
    for i in range(NQ):
        r = got[0][i, :got[2][i]].astype(np.int64)
        assert got[2][i] == K and np.all((r + r // 16) % TENANTS == i % TENANTS), "q%d: a row of another tenant" % i
    _check_end_to_end(c, index, host_block, status, got, kind + " tenant")
    # the host-pointer entry of the same route
    _same_rows(tm.search_batched(index, q, K, lists, o), got, kind + " search_batched_tokens")

    # two attributes: tenant i % 8 AND category in (all but i % 16), ANDed on the device into the first block
    cats = [[CAT0 + j for j in range(CATS) if j != i % CATS] for i in range(NQ)]
    host_cat = hip.allow_bitmaps_from_tokens(idx, tok, c.n, cats)
    host_and = hip.allow_bitmaps_combine(hip.ALLOW_AND, host_block, host_cat, c.n)
    assert host_and.any() and not np.array_equal(host_and, host_block)
    ct, coff = hip._token_lists(cats)
    d_ct, d_coff = _dev(ct), _dev(coff)
    d_block2 = _dev(np.full((NQ, words), SENTINEL))

    def build_and():
        tm.allow_bitmaps_device(d_tok.data_ptr(), d_off.data_ptr(), NQ, words, d_block.data_ptr(), _stream())
        tm.allow_bitmaps_device(d_ct.data_ptr(), d_coff.data_ptr(), NQ, words, d_block2.data_ptr(), _stream())
        hip.allow_bitmaps_combine_device(hip.ALLOW_AND, d_block.data_ptr(), words, d_block2.data_ptr(), words, NQ, c.n,
                                         d_block.data_ptr(), words, _stream())

    status, got = _search_on_stream(index, q, K, o, d_block, words, c.n, build_and)
    assert np.array_equal(d_block.cpu().numpy().view(np.uint64), host_and)
    _check_end_to_end(c, index, host_and, status, got, kind + " tenant AND category")

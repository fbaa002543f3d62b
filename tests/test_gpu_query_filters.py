"""Per-query allow-lists (scann_hip_search_opts.allow_bitmap_stride): one bitmap per query of a batch, on every tree scan,
every pipeline and every entry point, each query compared with the ORACLE under its own bitmap.

Shapes and the Case class are those of tests/test_gpu_filters.py (N = 80 000, 64 queries, 16 leaves, P = 6, m = 250,
k = 10: a sampled bound and the integer prefilters are in force).  Three batches:
  residue   query i allows the rows r with r % 8 == i % 8 (capacity n).  Eight disjoint bitmaps: a site that reads
            another query's bitmap -- query 0's, a column index, a slot index after regrouping -- returns a
            disallowed row.
  mixed     query i takes family ("f3", "f10", "not-topm", "m+1", "one-leaf", "empty", "one", "f1")[i % 8], seed i.
  capacity  capacity 65 at stride 4: even queries all-ones words, odd queries 0x5555..., the gap words all-ones.

The residue batch on the FLAT HASHER is aliased with the threshold sample, as the "unsampled" family of
tests/test_gpu_filters.py is: the flat hasher's rows are in datapoint order and its sample reads the rows j * 16
(80 000 rows: st = 16), every one of them in residue class 0.  The queries of classes 1..7 therefore have no allowed
sample, no bound, and 10 000 allowed points against a candidate list of 2 576 (ResourceExhausted); the queries of
class 0 have every sample allowed but only one further allowed row per sample, where the bound of rank J = 65 counts
on fifteen, so it keeps about 130 of the m = 250 points it must (Aborted, as the "sampled" family).  DESIGN section
7's per-query semantics, which this feature keeps unchanged, make the device entry fail every query of that batch with
count 0 -- status Aborted, the larger of the two codes, when a class-0 query is in the batch, else ResourceExhausted
-- and make the host entry repeat the batch without a bound.  For that batch the tests below assert exactly that
(never a wrong row; the host's rows equal to the oracle's), and they run the flat hasher additionally on the SKEWED
residue batch -- r allowed for query i iff (r + r // 16) % 8 == i % 8: the same eight
disjoint classes, every class holding one sample row in eight -- where, as on the tree for the plain residue batch,
the forced kernel must run on the first attempt and the device entry must return Ok with the host's rows."""
import ctypes

import numpy as np
import pytest

from oracle import pyoracle as orc
from scann_rust_amd import hip, synth
from tests import helpers as H
from tests.test_gpu_filters import ABORTED, FILTER_SCANS, K, M, N, NQ, PIPELINES, Case, _same_rows

pytestmark = pytest.mark.gpu

W = -(-N // 64)
MIXED = ("f3", "f10", "not-topm", "m+1", "one-leaf", "empty", "one", "f1")
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(kind, S):
        if (kind, S) not in cache:
            cache[kind, S] = Case(kind, S)
        return cache[kind, S]

    yield get
    cache.clear()


def residue_block(n=N, nq=NQ, skew=False):
    r = np.arange(n, dtype=np.int64)
    cls = ((r + r // 16) if skew else r) % 8
    rows = [H.words_of(np.flatnonzero(cls == j), n)[0] for j in range(8)]
    return np.stack([rows[i % 8] for i in range(nq)])


def mixed_block(c):
    rows = []
    for i in range(NQ):
        words, cap = c.family(MIXED[i % 8], seed=i)
        assert cap == c.n and words.size == W
        rows.append(words)
    return np.stack(rows)


def capacity_block(nq=NQ):
    b = np.full((nq, 4), ONES)
    b[1::2, :2] = np.uint64(0x5555555555555555)
    return b, 65


def device(index, q, k, o, block, cap):
    """H.device_search with one bitmap per query: the block goes to the device as it is, its row pitch is the stride"""
    o.allow_bitmap_stride = block.shape[1]
    try:
        return H.device_search(index, q, k, o, allow=block, allow_bits=cap)
    finally:
        o.allow_bitmap_stride = 0


def check_rows(c, q, block, cap, staged, qs, what, k=K):
    """Case.check per query under that query's own bitmap: all queries for allowed / capacity / unused slots, the
    queries `qs` also against the oracle, stage by stage"""
    idx, dist, cnt, (tok, tokd, ci, cd, cc) = staged
    for i in range(q.shape[0]):
        s = slice(i, i + 1)
        c.check(q[s], block[i], cap, (idx[s], dist[s], cnt[s], (tok[s], tokd[s], ci[s], cd[s], cc[s])),
                (0,) if i in qs else (), "%s q%d" % (what, i), k=k)


def aliased(kind, skew):
    """the plain residue batch on the flat hasher: classes 1..7 have no allowed sample (module docstring)"""
    return kind == "ah" and not skew


def device_residue(status, got, ref, kind, skew, what, lo=0):
    """the device entry on a residue batch that starts at query `lo`: Ok with the reference rows -- on the aliased batch
    every query fails with count 0: Aborted if a class-0 query is among them, else ResourceExhausted (module docstring)"""
    if not aliased(kind, skew):
        assert status == hip.OK, "%s: status %d" % (what, status)
        _same_rows(got, ref, what)
        return
    nq = got[2].size
    want = ABORTED if (np.arange(lo, lo + nq) % 8 == 0).any() else hip.RESOURCE_EXHAUSTED
    assert status == want, "%s: status %d, expected %d" % (what, status, want)
    assert np.all(got[2] == 0), what + ": a failed query with a count"


# ---- 1. every scan -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scan", FILTER_SCANS)
@pytest.mark.parametrize("S", [8, 32, 48])
@pytest.mark.parametrize("kind", ["ah", "txh"])
def test_every_scan_with_per_query_bitmaps(cases, kind, S, scan, monkeypatch):
    """64 queries, 64 bitmaps, under each forced scan: the forced kernel ran, every returned index is allowed under its
    own query's bitmap, the staged outputs of one query per residue class / per family equal the oracle's under that
    query's bitmap, the fast path's rows equal the staged rows, and the device entry answers the residue batch"""
    c = cases(kind, S)
    H.scan_env(monkeypatch, scan)
    index = hip.txh_create(**c.kw)
    index.enable_timing(True)
    o, q = c.opts(), c.q
    want = H.scan_kernel_name(scan, S)
    retry = H.scan_kernel_name("resident" if scan == "resident" else "gather", S)
    batches = [("residue", residue_block(), False), ("mixed", mixed_block(c), None)]
    if kind == "ah":
        batches.append(("skewed", residue_block(skew=True), True))
    for name, block, skew in batches:
        what = "%s S%d %s %s" % (kind, S, scan, name)
        # (the mixed batch holds families that make the sampled bound miss, the aliased residue batch queries without a
        # sample: the host entry's second attempt scans without a bound, as "sampled" does in tests/test_gpu_filters.py)
        ran = (want, retry) if name == "mixed" or aliased(kind, skew) else (want,)
        staged = index.search_batched(q, K, o, stages=True, allow=block, allow_bits=c.n)
        assert index.last_kernel_ms()[1] in ran, what + ": " + index.last_kernel_ms()[1]
        check_rows(c, q, block, c.n, staged, range(0, NQ, 9) if name != "mixed" else range(8, 16), what)
        fast = index.search_batched(q, K, o, allow=block, allow_bits=c.n)
        assert index.last_kernel_ms()[1] in ran, what + " fast"
        _same_rows(fast, staged[:3], what + " fast")
        if name != "mixed":
            status, di, dd, dc = device(index, q, K, o, block, c.n)
            device_residue(status, (di, dd, dc), staged[:3], kind, skew, what + " device")
    assert sorted(i % 8 for i in range(0, NQ, 9)) == list(range(8))   # (one query per residue class)


# ---- 2. against the shared-bitmap path ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ah", "txh"])
def test_strided_rows_equal_shared_bitmap_rows(cases, kind, monkeypatch):
    """row i of the strided residue search == row i of a stride-0 search of all 64 queries under bitmap i % 8"""
    c = cases(kind, 16)
    H.scan_env(monkeypatch, "default")
    index = hip.txh_create(**c.kw)
    o, q = c.opts(), c.q
    block = residue_block()
    got = index.search_batched(q, K, o, allow=block, allow_bits=c.n)
    for j in range(8):
        ref = index.search_batched(q, K, o, allow=block[j], allow_bits=c.n)
        sel = np.arange(j, NQ, 8)
        _same_rows(tuple(x[sel] for x in got), tuple(x[sel] for x in ref), "%s class %d" % (kind, j))


def test_byte_codes_with_per_query_bitmaps(monkeypatch):
    """8-bit codes (K = 256, S = 8) on the gather scan, the residue batch: the oracle's rows on each query's subset"""
    n, dim, S, nq, m = 20000, 32, 8, 32, 200
    H.scan_env(monkeypatch, "gather")
    rows = synth.uniform_f32(n, dim, 1100)
    rng = np.random.default_rng(11)
    cb = np.ascontiguousarray(rows[rng.choice(n, 256, replace=False)].reshape(256, S, dim // S).transpose(1, 0, 2),
                              np.float32)
    codes = rng.integers(0, 256, (n, S), dtype=np.uint8)
    kw = H.ah_kwargs_from_codes(rows, cb, codes)
    index = hip.txh_create(**kw)
    index.enable_timing(True)
    q = synth.uniform_f32(nq, dim, 1101)
    block = residue_block(n, nq)
    o = hip.default_opts()
    o.pre_reorder_k = m
    idx, dist, cnt = index.search_batched(q, K, o, allow=block, allow_bits=n)
    assert index.last_kernel_ms()[1] == "adc_scan_kernel"
    for i in range(nq):
        assert np.all(idx[i, :cnt[i]] % 8 == i % 8), "q%d: a row of another query's bitmap" % i
    for i in (0, 5, 10, 15, 20, 25, 30, 3):   # (one query per residue class)
        allowed = np.arange(i % 8, n, 8)
        oi, od = orc.ah_search_with_reordering(cb, np.ascontiguousarray(codes[allowed]),
                                               np.ascontiguousarray(kw["data"].reshape(n, kw["stride"])[allowed]),
                                               kw["stride"], q[i], K, m)
        assert cnt[i] == oi.size
        H.assert_topk_equal_up_to_ties(idx[i, :cnt[i]], dist[i, :cnt[i]], allowed[oi].astype(np.uint32), od,
                                       what="q%d" % i)


# ---- 3. every pipeline, both entries -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ah", "txh"])
def test_every_pipeline_with_per_query_bitmaps(cases, kind, monkeypatch):
    """The staged, small three-launch, small one-launch and wide pipelines at the query counts of PIPELINES, host and
    device entry, each sub-batch with its own rows of the bitmap block: the rows of the 64-query staged search (itself
    checked against the oracle) for the same queries.  The residue batch everywhere (the flat hasher also on the
    skewed one), the capacity batch on "staged" and "small"."""
    c = cases(kind, 16)
    H.scan_env(monkeypatch, "default")
    index = hip.txh_create(**c.kw)
    o, q = c.opts(), c.q
    cap_block, cap65 = capacity_block()
    batches = [("residue", residue_block(), c.n, False, tuple(PIPELINES)), ("capacity", cap_block, cap65, None, ("staged", "small"))]
    if kind == "ah":
        batches.append(("skewed", residue_block(skew=True), c.n, True, tuple(PIPELINES)))
    for bname, block, cap, skew, names in batches:
        H.scan_env(monkeypatch, "default")
        monkeypatch.setenv("SCANN_HIP_SMALL", "0")
        staged = index.search_batched(q, K, o, stages=True, allow=block, allow_bits=cap)
        check_rows(c, q, block, cap, staged, (0, 1, 2, 17, 40, 63), "%s %s staged" % (kind, bname))
        ref = staged[:3]
        for name in names:
            knobs, sizes = PIPELINES[name]
            if name == "fused" and kind == "txh":
                continue   # (P = 6: the tree never takes the one-launch form)
            H.scan_env(monkeypatch, "default")
            for kn, v in knobs.items():
                monkeypatch.setenv(kn, v)
            for nq in sizes:
                lo = 40 if nq == 1 else 0
                sub = tuple(x[lo:lo + nq] for x in ref)
                what = "%s %s %s nq%d" % (kind, bname, name, nq)
                _same_rows(index.search_batched(q[lo:lo + nq], K, o, allow=block[lo:lo + nq], allow_bits=cap), sub,
                           what + " host")
                status, di, dd, dc = device(index, q[lo:lo + nq], K, o, block[lo:lo + nq], cap)
                if bname == "capacity" or not (name == "staged" or nq > 16):
                    assert status == hip.OK, "%s device: status %d" % (what, status)   # (dense lists: no bound to miss)
                    _same_rows((di, dd, dc), sub, what + " device")
                else:
                    device_residue(status, (di, dd, dc), sub, kind, skew, what + " device", lo)


# ---- 4. the entry points that regroup or post-process ------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ah", "txh"])
def test_params_carry_each_querys_bitmap(cases, kind, monkeypatch):
    """search_batched_with_params regroups the queries by k: alternating k in {3, 10}, row i == the fixed-k strided
    search of query i at k_i (bitmap row i travels with query i into its group)"""
    c = cases(kind, 16)
    H.scan_env(monkeypatch, "default")
    index = hip.txh_create(**c.kw)
    o, q = c.opts(), c.q
    block = residue_block()
    ks = np.where(np.arange(NQ) % 2 == 0, 3, 10).astype(np.uint32)
    idx, dist, cnt = index.search_batched_with_params(q, ks, o, allow=block, allow_bits=c.n)
    assert o.allow_bitmap_stride == 0 and not o.allow_bitmap
    for k in (3, 10):
        sel = np.flatnonzero(ks == k)
        wi, wd, wc = index.search_batched(q, k, o, allow=block, allow_bits=c.n)
        _same_rows((idx[sel, :k], dist[sel, :k], cnt[sel]), (wi[sel], wd[sel], wc[sel]), "%s params k%d" % (kind, k))
        assert np.all(idx[sel, k:] == 0xFFFFFFFF)
        for i in sel:
            assert np.all(idx[i, :cnt[i]] % 8 == i % 8), "q%d: a row of another query's bitmap" % i


@pytest.mark.parametrize("kind", ["ah", "txh"])
def test_crowding_forwards_per_query_bitmaps(cases, kind, monkeypatch):
    """search_crowded with the strided residue block == per query, search_crowded with that query's bitmap shared"""
    c = cases(kind, 16)
    H.scan_env(monkeypatch, "default")
    index = hip.txh_create(**c.kw)
    index.set_crowding_attributes((np.arange(c.n, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(40))
    o, q = c.opts(), c.q
    block = residue_block()
    depth, limit = 60, 2
    got = index.search_crowded(q, K, depth, limit, o, allow=block, allow_bits=c.n)
    for j in range(8):
        ref = index.search_crowded(q, K, depth, limit, o, allow=block[j], allow_bits=c.n)
        sel = np.arange(j, NQ, 8)
        _same_rows(tuple(x[sel] for x in got), tuple(x[sel] for x in ref), "%s crowded class %d" % (kind, j))
        for i in sel:
            assert np.all(got[0][i, :got[2][i]] % 8 == j)


@pytest.mark.parametrize("kind", ["ah", "txh"])
def test_per_query_bitmaps_do_not_stick(cases, kind, monkeypatch):
    """an unfiltered search after a strided one, and a stride-0 one after it, equal their results from before"""
    c = cases(kind, 16)
    H.scan_env(monkeypatch, "default")
    index = hip.txh_create(**c.kw)
    o = c.opts()
    block = residue_block()
    words, cap = c.family("f3")
    for nq in (64, 3):
        q = c.q[:nq]
        plain = index.search_batched(q, K, o)
        shared = index.search_batched(q, K, o, allow=words, allow_bits=cap)
        index.search_batched(q, K, o, allow=block[:nq], allow_bits=c.n)
        assert o.allow_bitmap_stride == 0
        _same_rows(index.search_batched(q, K, o), plain, "host unfiltered nq%d" % nq)
        _same_rows(index.search_batched(q, K, o, allow=words, allow_bits=cap), shared, "host shared nq%d" % nq)
        device(index, q, K, o, block[:nq], c.n)
        status, di, dd, dc = H.device_search(index, q, K, o)
        assert status == hip.OK
        _same_rows((di, dd, dc), plain, "device unfiltered nq%d" % nq)
        status, di, dd, dc = H.device_search(index, q, K, o, allow=words, allow_bits=cap)
        assert status == hip.OK
        _same_rows((di, dd, dc), shared, "device shared nq%d" % nq)


# ---- 5. refusals -------------------------------------------------------------------------------------------------
def test_strided_calls_are_refused_where_they_are_not_built(cases, monkeypatch):
    """Unimplemented on a brute-force handle (host and device entry) and on scann_hip_txh_search_local_device;
    InvalidArgument for a stride below one bitmap (stride 1, capacity 65); a stride without a bitmap is ignored"""
    import torch
    c = cases("txh", 16)
    H.scan_env(monkeypatch, "default")
    block = residue_block()
    bf = hip.bf_create(c.data, c.n, c.dim, c.stride, 0)
    with pytest.raises(hip.ScannError) as e:
        bf.search_batched(c.q, K, allow=block, allow_bits=c.n)
    assert e.value.code == hip.UNIMPLEMENTED
    with pytest.raises(hip.ScannError) as e:
        device(bf, c.q, K, hip.default_opts(), block, c.n)
    assert e.value.code == hip.UNIMPLEMENTED
    _same_rows(bf.search_batched(c.q[:4], K, allow=block[0], allow_bits=c.n),
               bf.search_batched(c.q[:4], K, allow=block[0].copy(), allow_bits=c.n), "bf shared bitmap still served")

    index = hip.txh_create(**c.kw)
    o = c.opts()
    cap_block, _ = capacity_block()
    o.allow_bitmap, o.allow_bitmap_bits, o.allow_bitmap_stride = hip.ptr(cap_block, hip.u64p), 65, 1
    try:
        with pytest.raises(hip.ScannError) as e:
            index.search_batched(c.q, K, o)
        assert e.value.code == hip.INVALID_ARGUMENT
    finally:
        o.allow_bitmap, o.allow_bitmap_bits, o.allow_bitmap_stride = None, 0, 0
    with pytest.raises(ValueError):   # (the Python wrapper refuses a capacity past a row's words by itself)
        index.search_batched(c.q, K, o, allow=cap_block[:, :1], allow_bits=65)
    with pytest.raises(hip.ScannError) as e:
        device(index, c.q, K, o, np.ascontiguousarray(cap_block[:, :1]), 65)
    assert e.value.code == hip.INVALID_ARGUMENT
    o.allow_bitmap_stride = 7   # no bitmap: the stride is ignored
    try:
        _same_rows(index.search_batched(c.q, K, o), index.search_batched(c.q, K, c.opts()), "stride without a bitmap")
    finally:
        o.allow_bitmap_stride = 0

    Lh = hip.load()
    dev = torch.device("cuda", 0)
    sptr = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    qd = torch.from_numpy(np.ascontiguousarray(c.q)).to(dev)
    da = torch.from_numpy(block.view(np.int64).copy()).to(dev)
    g_keys = torch.zeros((NQ, M), dtype=torch.int64, device=dev)
    g_idx = torch.zeros((NQ, M), dtype=torch.int32, device=dev)
    g_ex = torch.zeros((NQ, M), dtype=torch.float32, device=dev)
    g_cnt = torch.zeros((NQ,), dtype=torch.int32, device=dev)
    o.allow_bitmap = ctypes.cast(p(da), ctypes.POINTER(ctypes.c_uint64))
    o.allow_bitmap_bits, o.allow_bitmap_stride = c.n, W
    try:
        assert Lh.scann_hip_txh_search_local_device(index.h, p(qd), NQ, c.dim, K, ctypes.byref(o), p(g_keys), p(g_idx),
                                                    p(g_ex), p(g_cnt), sptr) == hip.UNIMPLEMENTED
        o.allow_bitmap_stride = 0   # (one bitmap: served as before)
        hip.check(Lh.scann_hip_txh_search_local_device(index.h, p(qd), NQ, c.dim, K, ctypes.byref(o), p(g_keys), p(g_idx),
                                                       p(g_ex), p(g_cnt), sptr))
        torch.cuda.synchronize()
    finally:
        o.allow_bitmap, o.allow_bitmap_bits, o.allow_bitmap_stride = None, 0, 0


# ---- 6. bitmaps from id lists, on the device ---------------------------------------------------------------------
def _from_ids_device(lists, bits, stride):
    import torch
    dev = torch.device("cuda", 0)
    nq = len(lists)
    ids = np.concatenate(lists + [np.zeros(1, np.uint32)]).astype(np.uint32)   # (never an empty allocation)
    off = np.concatenate([[0], np.cumsum([l.size for l in lists])]).astype(np.uint64)
    d_ids = torch.from_numpy(ids.view(np.int32).copy()).to(dev)
    d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    d_out = torch.full((max(nq * stride, 1) + 1,), -1, dtype=torch.int64, device=dev)   # all-ones, one guard word
    torch.cuda.synchronize()
    hip.allow_bitmaps_from_ids_device(d_ids.data_ptr(), d_off.data_ptr(), nq, bits, stride, d_out.data_ptr(),
                                      torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint64)
    assert out[nq * stride] == ONES, "a word past the block was written"
    host = hip.allow_bitmaps_from_ids(ids[:-1], off, bits, stride)
    return out[:nq * stride].reshape(nq, stride), host, d_out


@pytest.mark.parametrize("bits", [0, 65, 1000])
def test_from_ids_device_small(bits):
    rng = np.random.default_rng(bits)
    lists = [np.zeros(0, np.uint32), np.array([0], np.uint32), np.array([bits, bits + 1, 0xFFFFFFFF, 0, 0], np.uint32),
             rng.integers(0, bits + 70, 200).astype(np.uint32), np.arange(bits + 5, dtype=np.uint32)[::-1].copy()]
    for extra in (0, 3):
        got, host, _ = _from_ids_device(lists, bits, -(-bits // 64) + extra)
        assert np.array_equal(got, host), "bits %d extra %d" % (bits, extra)


def test_from_ids_device_drives_a_search(cases, monkeypatch):
    """300 lists of 0..5000 ids (duplicates, ids past the capacity) over 80 000 bits: bitwise the host function's
    block; and the residue block built on the device from id lists drives a device-entry search to the same rows as
    the host-built block"""
    rng = np.random.default_rng(7)
    lens = np.linspace(0, 5000, 300).astype(np.int64)
    lists = [rng.integers(0, N + 500, l).astype(np.uint32) for l in lens]
    lists[5] = np.repeat(lists[5], 3)
    got, host, _ = _from_ids_device(lists, N, W)
    assert np.array_equal(got, host)
    assert any((l >= N).any() for l in lists) and int(host[-1].view(np.uint8).sum()) > 0

    c = cases("txh", 16)
    H.scan_env(monkeypatch, "default")
    index = hip.txh_create(**c.kw)
    o, q = c.opts(), c.q
    block = residue_block()
    lists = [rng.permutation(np.arange(i % 8, N, 8)).astype(np.uint32) for i in range(NQ)]
    got, host, d_out = _from_ids_device(lists, N, W)
    assert np.array_equal(host, block) and np.array_equal(got, block)
    want = device(index, q, K, o, block, c.n)
    assert want[0] == hip.OK
    o.allow_bitmap = ctypes.cast(ctypes.c_void_p(d_out.data_ptr()), ctypes.POINTER(ctypes.c_uint64))
    o.allow_bitmap_bits, o.allow_bitmap_stride = N, W
    try:
        status, di, dd, dc = H.device_search(index, q, K, o)
    finally:
        o.allow_bitmap, o.allow_bitmap_bits, o.allow_bitmap_stride = None, 0, 0
    assert status == hip.OK
    _same_rows((di, dd, dc), want[1:], "device-built block")
    _same_rows((di, dd, dc), index.search_batched(q, K, o, allow=block, allow_bits=c.n), "device-built block vs host")

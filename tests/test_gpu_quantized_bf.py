"""Brute force over rows stored as bf16, FP8 E4M3 or int8 (scann_hip_bf_create_quantized) against the
checker (tests/quantized_checker.py: the reference's one_to_many_{bf16,fp8,int8}_float_* loops) and the
oracle's TopK.  Distances bitwise against TopK; indices bitwise against the (distance, index) key order that
every brute-force selection of the library uses (the reference's TopK drains equal distances in heap order,
which no index rule reproduces: its tie order is not compared)."""
import ctypes
import threading

import numpy as np
import pytest

from oracle import pyoracle as orc
from scann_rust_amd import hip, synth
from tests import quantized_checker as qc

pytestmark = pytest.mark.gpu

FMTS = [hip.ROWS_BF16, hip.ROWS_FP8_E4M3, hip.ROWS_INT8]
MEASURES = [hip.SQUARED_L2, hip.DOT_PRODUCT, hip.L2]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want):
    """bitwise, NaN compared as NaN"""
    got = np.asarray(got, np.float32); want = np.asarray(want, np.float32)
    both_nan = np.isnan(got) & np.isnan(want)
    return np.array_equal(np.where(both_nan, 0, bits(got)), np.where(both_nan, 0, bits(want)))


def make_rows(fmt, n, dim, stride, seed):
    """(rows [n][stride] in the format, inv_multiplier) from U[0,1) values."""
    x = synth.uniform_f32(n, dim, seed)
    if fmt == hip.ROWS_BF16:
        codes, inv = qc.bf16_from_f32(x), 1.0
    elif fmt == hip.ROWS_FP8_E4M3:
        codes, inv = orc.fp8_quantize(x, 4.0), 1.0
    else:
        codes, inv = hip.symmetric_int8(x * np.float32(2) - np.float32(1))
    out = np.zeros((n, stride), codes.dtype)
    out[:, :dim] = codes
    rng = np.random.default_rng(seed)
    out[:, dim:] = rng.integers(0, 100, size=(n, stride - dim)).astype(codes.dtype)   # padding is never read
    return out, inv


def checker_topk(d, k):
    n = d.size
    return orc.topk_run(min(k, n), np.arange(n, dtype=np.uint32), d)


def assert_topk(idx, dist, cnt, d, k, what=""):
    """distances = TopK's, bitwise; indices = the first min(k, n) by (distance, index) key, bitwise."""
    oi, od = checker_topk(d, k)
    c = int(cnt)
    assert c == oi.size, what
    assert same(dist[:c], od), what
    b = np.asarray(d, np.float32).view(np.uint32)
    key = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))   # common.h f32_to_ordered
    order = np.lexsort((np.arange(d.size), key))[:c]
    assert np.array_equal(np.asarray(idx[:c], np.int64), order), what


# ---- 1. the one-to-many kernels, pinned through the dense matrix ------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("measure", MEASURES)
def test_distances_bitwise(fmt, measure):
    for dim in (1, 7, 8, 9, 50, 96, 128, 256):
        for stride in sorted({dim, dim + 5, ((dim + 15) // 16) * 16}):
            n = 1500
            rows, inv = make_rows(fmt, n, dim, stride, 10 + dim)
            index = hip.bf_create_quantized(rows, n, dim, stride, fmt, measure, inv)
            for nq in (1, 3):
                q = synth.uniform_f32(nq, dim, 7 + nq)
                got = hip.bf_distances(index, q)
                want = qc.distances(q, rows, dim, fmt, measure, inv)
                assert same(got, want), (fmt, measure, dim, stride, nq)


@pytest.mark.parametrize("fmt", FMTS)
def test_distances_large_n(fmt):
    n, dim = 70000, 96
    rows, inv = make_rows(fmt, n, dim, dim, 3)
    index = hip.bf_create_quantized(rows, n, dim, dim, fmt, hip.SQUARED_L2, inv)
    q = synth.uniform_f32(2, dim, 4)
    assert same(hip.bf_distances(index, q), qc.distances(q, rows, dim, fmt, hip.SQUARED_L2, inv))


@pytest.mark.parametrize("measure", MEASURES)
def test_fp8_all_codes_and_bf16_specials(measure):
    dim = 16
    codes = np.arange(256, dtype=np.uint8).reshape(16, 16)
    rows = np.concatenate([codes, np.roll(codes, 3, axis=1), codes[::-1]])
    index = hip.bf_create_quantized(rows, rows.shape[0], dim, dim, hip.ROWS_FP8_E4M3, measure)
    q = (synth.uniform_f32(3, dim, 9) * np.float32(8) - np.float32(4)).astype(np.float32)
    assert same(hip.bf_distances(index, q), qc.distances(q, rows, dim, hip.ROWS_FP8_E4M3, measure))
    # bf16: subnormals, signed zeros, the largest finite values, +-inf, NaN payloads
    special = np.array([0x0001, 0x8001, 0x007F, 0x0000, 0x8000, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x7FC1,
                        0xFFFF, 0x3F80, 0x0080, 0x8080, 0x4000, 0xC000], np.uint16)
    rng = np.random.default_rng(1)
    b = np.stack([rng.permutation(special) for _ in range(40)])
    b[:20] = qc.bf16_from_f32(synth.uniform_f32(20, dim, 2))
    b[25, :] = 0x0001
    index = hip.bf_create_quantized(b, b.shape[0], dim, dim, hip.ROWS_BF16, measure)
    got = hip.bf_distances(index, q)
    assert same(got, qc.distances(q, b, dim, hip.ROWS_BF16, measure))
    assert np.isnan(got).any()


# ---- 2. searches against the oracle's TopK ----------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("measure", MEASURES)
def test_search_batched_matches_topk(fmt, measure):
    dim = 24
    for n in (0, 5, 1000, 70000):
        rows, inv = make_rows(fmt, max(n, 1), dim, dim, n + 1)
        rows = rows[:n]
        index = hip.bf_create_quantized(rows, n, dim, dim, fmt, measure, inv)
        assert index.size() == n and index.dimensionality() == dim
        qall = synth.uniform_f32(1024 if n <= 1000 else 32, dim, 77)
        dmat = qc.distances(qall, rows, dim, fmt, measure, inv) if n else None
        for nq in (1, 3, 16, 32, 1024):
            if nq > qall.shape[0]:
                continue
            for k in (1, 10, 100, 2048, n + 7):
                if min(k, n) > 2048:   # brute-force k <= 2048, as for f32 rows
                    with pytest.raises(hip.ScannError) as e:
                        index.search_batched(qall[:nq], k)
                    assert e.value.code == hip.UNIMPLEMENTED
                    continue
                idx, dist, cnt = index.search_batched(qall[:nq], k)
                for i in range(0, nq, max(1, nq // 16)):
                    if n == 0:
                        assert cnt[i] == 0
                        continue
                    assert_topk(idx[i], dist[i], cnt[i], dmat[i], k,
                                what="fmt %d m %d n %d nq %d k %d q%d" % (fmt, measure, n, nq, k, i))


@pytest.mark.parametrize("measure", MEASURES)
def test_int8_offset_binary_bytes_read_as_signed(measure):
    """ScalarQuantizer writes offset-binary bytes (scalar.rs:162-172); ScalarQuantizedBruteForceSearcher reads
    them as signed i8 with inv_multiplier = quantizer.scale() and no min_value (scalar_quantized.rs:198-225).
    Ties: few distinct codes, so many equal distances, ordered by index."""
    n, dim, k = 3000, 16, 50
    x = synth.uniform_f32(n, dim, 11)
    lo, hi = np.float32(0.0), np.float32(1.0)
    scale = (hi - lo) / np.float32(255)
    u = np.clip(np.rint((np.clip(x, lo, hi) - lo) * (np.float32(1) / scale)), 0, 255).astype(np.int32)
    u = (u // 64) * 64   # 4 levels: plenty of ties
    rows = u.astype(np.uint8).view(np.int8)
    index = hip.bf_create_quantized(rows, n, dim, dim, hip.ROWS_INT8, measure, float(scale))
    q = synth.uniform_f32(20, dim, 12)
    idx, dist, cnt = index.search_batched(q, k)
    d = qc.distances(q, rows, dim, qc.ROWS_INT8, measure, scale)
    for i in range(20):
        assert_topk(idx[i], dist[i], cnt[i], d[i], k, what="q%d" % i)


# ---- 3. / 4. shortlist knobs and the device entry ---------------------------------------------------------
@pytest.fixture
def force_shortlist(monkeypatch):
    """Knobs that make f32 brute-force batches take the bf16-shortlist path (copy of test_gpu_parity's
    fixture).  Quantized rows have only exact passes: the results must not change."""
    monkeypatch.setenv("SCANN_HIP_BF_SHORTLIST_MIN_ROWS", "1")
    monkeypatch.setenv("SCANN_HIP_BF_SHORTLIST_MIN_QUERIES", "1")
    monkeypatch.setenv("SCANN_HIP_SMALL", "0")


def _device_search(index, q, k, exact, stream=None):
    import torch
    dev = torch.device("cuda", 0)
    nq, dim = q.shape
    qd = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    oi = torch.empty((nq, k), dtype=torch.int32, device=dev)
    od = torch.empty((nq, k), dtype=torch.float32, device=dev)
    oc = torch.empty((nq,), dtype=torch.int32, device=dev)
    st = stream or torch.cuda.current_stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    o = hip.default_opts()
    o.bf_exact = 1 if exact else 0
    L = hip.load()
    with torch.cuda.stream(st):
        hip.check(L.scann_hip_index_reserve(index.h, nq, k, ctypes.byref(o)))
        hip.check(L.scann_hip_search_batched_device(index.h, p(qd), nq, dim, k, ctypes.byref(o), p(oi), p(od), p(oc),
                                                    sp))
        status = L.scann_hip_index_last_device_status(index.h, sp)
    return status, oi.cpu().numpy().view(np.uint32), od.cpu().numpy(), oc.cpu().numpy()


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("measure", MEASURES)
def test_shortlist_matches_exact(force_shortlist, fmt, measure):
    """bf16 MFMA with the stored rows as the exact operand and the query split shortlists max(32, 4k) rows, the
    reference's arithmetic re-scores them, the per-format bound proves the rest: identical to bf_exact = 1,
    every query verified on U[0,1) data (device entry status Ok)."""
    n, dim, k, nq = 20000, 128, 10, 64
    rows, inv = make_rows(fmt, n, dim, dim, 21)
    index = hip.bf_create_quantized(rows, n, dim, dim, fmt, measure, inv)
    q = synth.uniform_f32(nq, dim, 22)
    index.enable_timing(True)
    idx, dist, cnt = index.search_batched(q, k)
    assert index.last_kernel_ms()[1] == "bf_bf16_kernel"
    o = hip.default_opts()
    o.bf_exact = 1
    idx2, dist2, cnt2 = index.search_batched(q, k, opts=o)
    assert np.array_equal(idx, idx2) and same(dist, dist2) and np.array_equal(cnt, cnt2)
    st, di, dd, dc = _device_search(index, q, k, exact=False)
    assert st == hip.OK
    assert np.array_equal(di, idx) and same(dd, dist)
    d = qc.distances(q[:8], rows, dim, fmt, measure, inv)
    for i in range(8):
        assert_topk(idx[i], dist[i], cnt[i], d[i], k, what="q%d" % i)


@pytest.mark.parametrize("fmt", FMTS)
def test_shortlist_rejects_near_duplicates(force_shortlist, fmt):
    """Near-duplicate rows (most rows quantize to the same codes): the bound cannot separate the k-th result
    from the shortlist's edge.  The host entry repeats those queries exactly by itself; the device entry reports
    Aborted, and its repeat with bf_exact = 1 equals the host result and the checker."""
    import torch
    n, dim, k, nq = 8000, 64, 10, 40
    base = synth.uniform_f32(1, dim, 5)
    x = (base + np.float32(1e-4) * synth.uniform_f32(n, dim, 6)).astype(np.float32)
    if fmt == hip.ROWS_BF16:
        rows, inv = qc.bf16_from_f32(x), 1.0
    elif fmt == hip.ROWS_FP8_E4M3:
        rows, inv = orc.fp8_quantize(x, 64.0), 1.0
    else:
        rows, inv = hip.symmetric_int8(x)
    index = hip.bf_create_quantized(rows, n, dim, dim, fmt, hip.SQUARED_L2, inv)
    q = synth.uniform_f32(nq, dim, 7)
    hi, hd, hc = index.search_batched(q, k)
    s1 = torch.cuda.Stream()
    st, di, dd, dc = _device_search(index, q, k, exact=False, stream=s1)
    assert st == 10   # Aborted: repeat with bf_exact = 1
    st2, di2, dd2, dc2 = _device_search(index, q, k, exact=True, stream=s1)
    assert st2 == hip.OK
    assert np.array_equal(di2, hi) and same(dd2, hd)
    d = qc.distances(q, rows, dim, fmt, hip.SQUARED_L2, inv)
    for i in range(nq):
        assert_topk(hi[i], hd[i], hc[i], d[i], k, what="q%d" % i)


# ---- 5. per-query k, radius, threads ----------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_params_radius_and_threads(fmt):
    n, dim = 5000, 40
    rows, inv = make_rows(fmt, n, dim, dim + 8, 31)
    index = hip.bf_create_quantized(rows, n, dim, dim + 8, fmt, hip.L2, inv)
    q = synth.uniform_f32(6, dim, 32)
    d = qc.distances(q, rows, dim, fmt, hip.L2, inv)
    ks = np.array([1, 50, 3, 50, 2048, 10], np.uint32)
    idx, dist, cnt = index.search_batched_with_params(q, ks)
    for i in range(6):
        assert_topk(idx[i], dist[i], cnt[i], d[i], int(ks[i]), what="q%d" % i)
    # radius: every d <= r, stable-sorted by distance; capacity overflow reports the full count
    r = float(np.sort(d[0])[300])
    ri, rd, rc = hip.bf_search_radius(index, q[0], r)
    sel = np.nonzero(d[0] <= np.float32(r))[0]
    order = sel[np.argsort(d[0][sel], kind="stable")]
    assert rc == order.size and np.array_equal(ri, order) and same(rd, d[0][order])
    ci, cd, cc = hip.bf_search_radius(index, q[0], r, capacity=10)
    assert cc == order.size and np.array_equal(ci, order[:10])
    # concurrent host threads on one handle
    errs = []

    def worker(t):
        try:
            for rep in range(3):
                qi = synth.uniform_f32(3 + t, dim, 100 + t)
                ii, dd_, cc_ = index.search_batched(qi, 20)
                dm = qc.distances(qi, rows, dim, fmt, hip.L2, inv)
                for j in range(qi.shape[0]):
                    assert_topk(ii[j], dd_[j], cc_[j], dm[j], 20, what="thread %d q%d" % (t, j))
        except Exception as e:   # noqa: BLE001 -- reported below
            errs.append(e)
    ts = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs


# ---- 6. errors --------------------------------------------------------------------------------------------
def test_errors():
    rows = np.zeros((10, 8), np.int8)

    def code(fn):
        with pytest.raises(hip.ScannError) as e:
            fn()
        return e.value.code
    assert code(lambda: hip.bf_create_quantized(rows, 10, 8, 8, 7, hip.SQUARED_L2)) == hip.INVALID_ARGUMENT
    assert code(lambda: hip.bf_create_quantized(rows, 10, 8, 8, 0, hip.SQUARED_L2)) == hip.INVALID_ARGUMENT
    for m in (hip.L1, hip.COSINE):
        assert code(lambda: hip.bf_create_quantized(rows, 10, 8, 8, hip.ROWS_INT8, m)) == hip.UNIMPLEMENTED
    assert code(lambda: hip.bf_create_quantized(rows, 10, 8, 4, hip.ROWS_INT8, hip.SQUARED_L2)) == hip.INVALID_ARGUMENT
    L = hip.load()
    h = ctypes.c_void_p()
    assert L.scann_hip_bf_create_quantized(hip.context(), None, 10, 8, 8, hip.ROWS_BF16, 1.0, 0,
                                           ctypes.byref(h)) == hip.INVALID_ARGUMENT
    for bad in (float("inf"), float("nan")):
        assert code(lambda: hip.bf_create_quantized(rows, 10, 8, 8, hip.ROWS_INT8, hip.SQUARED_L2, bad)) == \
            hip.INVALID_ARGUMENT
    index = hip.bf_create_quantized(rows, 10, 8, 8, hip.ROWS_INT8, hip.SQUARED_L2, 0.5)
    c = np.zeros((2, 8), np.float32)
    assert code(lambda: hip.kmeans_init_pp(index, 2, 1)) == hip.INVALID_ARGUMENT
    assert code(lambda: hip.kmeans_lloyd(index, c)) == hip.INVALID_ARGUMENT
    assert code(lambda: hip.bf_assign_nearest(index, c)) == hip.INVALID_ARGUMENT
    assert code(lambda: hip.txh_partition(index, c, 1)) == hip.INVALID_ARGUMENT
    assert code(lambda: index.search_batched(np.zeros((1, 7), np.float32), 3)) == hip.INVALID_ARGUMENT
    # n == 0: empty rows, no rows pointer needed
    empty = hip.bf_create_quantized(np.zeros((0, 8), np.uint16), 0, 8, 8, hip.ROWS_BF16, hip.DOT_PRODUCT)
    _, _, cnt = empty.search_batched(np.zeros((2, 8), np.float32), 5)
    assert list(cnt) == [0, 0]


def test_bf16_quantize_bitwise():
    rng = np.random.default_rng(8)
    x = np.concatenate([
        rng.standard_normal(100000).astype(np.float32) * np.float32(1e3),
        rng.integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32).view(np.float32),   # every class
        np.array([0x3F808000, 0x3F818000, 0x7F7FFFFF, 0x00008001, 0x7F800001, 0xFF812345], np.uint32).view(np.float32),
    ])
    got = hip.bf16_quantize(x)
    assert np.array_equal(got, qc.bf16_from_f32(x))


# ---- 7. full size --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_fullsize_1m(fmt):
    n, dim, k, nq = 1_000_000, 128, 10, 1024
    x = synth.uniform_f32(n, dim, 42)
    if fmt == hip.ROWS_BF16:
        rows, inv = qc.bf16_from_f32(x), 1.0
    elif fmt == hip.ROWS_FP8_E4M3:
        rows, inv = orc.fp8_quantize(x, 64.0), 1.0
    else:
        rows, inv = hip.symmetric_int8(x)
    del x
    index = hip.bf_create_quantized(rows, n, dim, dim, fmt, hip.SQUARED_L2, inv)
    q = synth.uniform_f32(nq, dim, 123)
    idx, dist, cnt = index.search_batched(q, k)
    sample = np.arange(0, nq, 128)
    d = qc.distances(q[sample], rows, dim, fmt, hip.SQUARED_L2, inv)
    for j, i in enumerate(sample):
        assert_topk(idx[i], dist[i], cnt[i], d[j], k, what="q%d" % i)

"""Brute force over packed int4 rows (SCANN_HIP_ROWS_INT4): the distances are the INT8 format's, bit for bit, on the
unpacked codes, so the checker is tests/quantized_checker.py on hip.unpack_int4 and an INT8 handle over the same codes
must agree; the shortlist of such handles is scored by bf_i8mfma_kernel; quantize_rows packs on the device."""
import numpy as np
import pytest

from scann_rust_amd import hip, synth
from tests import quantized_checker as qc
from tests.test_gpu_quantized_bf import _device_search, assert_topk, force_shortlist, same   # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

MEASURES = [hip.DOT_PRODUCT, hip.SQUARED_L2, hip.L2]
INV = 0.0371


def make_codes(n, dim, stride, seed):
    """int8 codes [n][stride] over all 16 values, a whole row of -8 and one of 7; the pad columns hold noise"""
    codes = np.random.default_rng(seed).integers(-8, 8, size=(n, stride)).astype(np.int8)
    codes[0, :dim] = -8
    codes[-1, :dim] = 7
    return codes


def queries(nq, dim, seed):
    return (synth.uniform_f32(nq, dim, seed) * np.float32(2) - np.float32(1)).astype(np.float32)


def handles(codes, dim, measure):
    n, stride = codes.shape
    return (hip.bf_create_quantized(hip.pack_int4(codes), n, dim, stride, hip.ROWS_INT4, measure, INV),
            hip.bf_create_quantized(codes, n, dim, stride, hip.ROWS_INT8, measure, INV))


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("nq", [1, 3, 17])
def test_streaming_matches_int8_bitwise(measure, nq):
    for n, dim, stride in [(1, 8, 8), (63, 13, 14), (257, 70, 96), (300, 24, 26)]:
        codes = make_codes(n, dim, stride, n)
        i4, i8 = handles(codes, dim, measure)
        q = queries(nq, dim, 5 + nq)
        want = qc.distances(q, codes, dim, qc.ROWS_INT8, measure, np.float32(INV))
        got = hip.bf_distances(i4, q)
        assert same(got, want) and same(hip.bf_distances(i8, q), got), (n, dim, stride)
        k = min(5, n)
        idx, dist, cnt = i4.search_batched(q, k)
        idx8, dist8, _ = i8.search_batched(q, k)
        assert np.array_equal(idx, idx8) and same(dist, dist8), (n, dim, stride)
        for i in range(nq):
            assert_topk(idx[i], dist[i], cnt[i], want[i], k, what="n %d q%d" % (n, i))


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("dim", [32, 128])   # the smallest dim the kernel takes; every dim it takes is whole k-steps of 32
@pytest.mark.parametrize("nq,k", [(33, 1), (33, 10), (70, 1), (70, 10)])
def test_shortlist_on_integer_mfma(force_shortlist, measure, dim, nq, k):
    n = 4133   # 32 stages of 128 rows and a partial one
    codes = make_codes(n, dim, dim, dim + k)
    index, _ = handles(codes, dim, measure)
    q = queries(nq, dim, nq)
    index.enable_timing(True)
    idx, dist, cnt = index.search_batched(q, k)
    assert index.last_kernel_ms()[1] == "bf_i8mfma_kernel"
    o = hip.default_opts()
    o.bf_exact = 1
    idx2, dist2, cnt2 = index.search_batched(q, k, opts=o)
    assert np.array_equal(idx, idx2) and same(dist, dist2) and np.array_equal(cnt, cnt2)
    # the device entry repeats nothing: status Ok means every query was verified from the kernel's own scores
    st, di, dd, _ = _device_search(index, q, k, exact=False)
    assert st == hip.OK
    assert np.array_equal(di, idx) and same(dd, dist)
    d = qc.distances(q, codes, dim, qc.ROWS_INT8, measure, np.float32(INV))
    for i in range(nq):
        assert_topk(idx[i], dist[i], cnt[i], d[i], k, what="q%d" % i)


def test_allow_bitmap_and_radius_on_odd_dim():
    """the brute-force contracts that ride on bf_quant_kernel, on the shape whose last code shares its byte with padding"""
    n, dim, stride = 63, 13, 14
    codes = make_codes(n, dim, stride, 9)
    i4, i8 = handles(codes, dim, hip.L2)
    q = queries(3, dim, 2)
    d = qc.distances(q, codes, dim, qc.ROWS_INT8, hip.L2, np.float32(INV))
    allow = np.array([0x5A5A5A5A5A5A5A5A], np.uint64)
    idx, dist, cnt = i4.search_batched(q, 5, allow=allow)
    idx8, dist8, cnt8 = i8.search_batched(q, 5, allow=allow)
    assert np.array_equal(idx, idx8) and same(dist, dist8) and np.array_equal(cnt, cnt8)
    allowed = np.array([i for i in range(n) if (int(allow[0]) >> i) & 1])
    for i in range(3):
        order = allowed[np.lexsort((allowed, d[i][allowed]))][:5]
        assert np.array_equal(idx[i][:cnt[i]], order) and same(dist[i][:cnt[i]], d[i][order])
    r = float(np.sort(d[0])[20])
    ri, rd, rc = hip.bf_search_radius(i4, q[0], r)
    sel = np.nonzero(d[0] <= np.float32(r))[0]
    order = sel[np.argsort(d[0][sel], kind="stable")]
    assert rc == order.size and np.array_equal(ri, order) and same(rd, d[0][order])


def test_shortlist_rejects_near_duplicates(force_shortlist):
    """Four distinct rows repeated 2000 times each: far more than max(32, 4k) rows tie around the k-th, no bound
    separates them.  Mirrors test_gpu_quantized_bf.test_shortlist_rejects_near_duplicates."""
    import torch
    n, dim, k, nq = 8000, 64, 10, 40
    codes = make_codes(4, dim, dim, 3)[np.arange(n) % 4]
    index, _ = handles(codes, dim, hip.SQUARED_L2)
    q = queries(nq, dim, 7)
    hi, hd, hc = index.search_batched(q, k)
    s1 = torch.cuda.Stream()
    st, _, _, _ = _device_search(index, q, k, exact=False, stream=s1)
    assert st == 10   # Aborted: repeat with bf_exact = 1
    st2, di2, dd2, _ = _device_search(index, q, k, exact=True, stream=s1)
    assert st2 == hip.OK
    assert np.array_equal(di2, hi) and same(dd2, hd)
    d = qc.distances(q, codes, dim, qc.ROWS_INT8, hip.SQUARED_L2, np.float32(INV))
    for i in range(nq):
        assert_topk(hi[i], hd[i], hc[i], d[i], k, what="q%d" % i)


def expected_codes(x, mode, stats, value_range):
    """(codes in -8 .. 7, params4, zero point or None) of scann_hip_index_quantize_rows(ROWS_INT4, bits 4), restated"""
    if mode == hip.SQ_SIGNED:
        m = np.float32(np.abs(x).max())
        s = np.float32(np.float64(m) / 7.0)
        return np.clip(np.rint(x / s), -7, 7).astype(np.int8), np.array([-m, m, s, np.float32(1) / s], np.float32), None
    sq = hip.ScalarQuantizer(bits=4, mode=mode, value_range=value_range)
    p = sq.calibrate(stats)
    mn, inv_scale = np.float32(p["min"]), np.float32(p["inv_scale"])
    t = (np.clip(x, mn, np.float32(p["max"])) - mn) * inv_scale
    c = np.clip(np.floor(t.astype(np.float64) + 0.5), 0, 15).astype(np.int64)   # roundf: half away from zero
    return (((c + 8) & 15) - 8).astype(np.int8), sq.params, p["zero_point"]


@pytest.mark.parametrize("mode", [hip.SQ_STDDEV, hip.SQ_SYMMETRIC, hip.SQ_RANGE, hip.SQ_SIGNED])
@pytest.mark.parametrize("n,dim,stride", [(64, 16, 16), (257, 70, 96)])
def test_quantize_rows_packs_on_device(mode, n, dim, stride):
    x = queries(n, dim, n + mode)
    rows = np.zeros((n, stride), np.float32)
    rows[:, :dim] = x
    src = hip.bf_create(rows, n, dim, stride, hip.DOT_PRODUCT)
    vr = (-0.5, 0.75) if mode == hip.SQ_RANGE else None
    index, params = src.quantize_rows(hip.ROWS_INT4, mode=mode, bits=4, value_range=vr)
    want, p4, zp = expected_codes(x, mode, hip.quantization_stats(src), vr)
    assert [params[key] for key in ("min", "max", "scale", "inv_scale")] == [float(v) for v in p4]
    assert params["zero_point"] == (0 if zp is None else zp)
    # axis queries under DotProduct read the stored values back: distance = -(code * scale)
    values = -hip.bf_distances(index, np.eye(dim, dtype=np.float32)).T
    got = np.rint(values / np.float32(params["scale"])).astype(np.int8)
    assert np.array_equal(got.astype(np.float32) * np.float32(params["scale"]), values)
    assert np.array_equal(hip.pack_int4(got), hip.pack_int4(want))


def test_refusals():
    def code(fn):
        with pytest.raises(hip.ScannError) as e:
            fn()
        return e.value.code
    packed = np.zeros((10, 4), np.uint8)
    assert code(lambda: hip.bf_create_quantized(packed, 10, 7, 7, hip.ROWS_INT4, hip.SQUARED_L2)) == hip.INVALID_ARGUMENT
    for m in (hip.L1, hip.COSINE):
        assert code(lambda: hip.bf_create_quantized(packed, 10, 8, 8, hip.ROWS_INT4, m)) == hip.UNIMPLEMENTED
    empty = hip.bf_create_quantized(packed[:0], 0, 8, 8, hip.ROWS_INT4, hip.DOT_PRODUCT)
    assert list(empty.search_batched(np.zeros((2, 8), np.float32), 5)[2]) == [0, 0]
    src = hip.bf_create(np.ones((10, 8), np.float32), 10, 8, 8, hip.SQUARED_L2)
    odd = hip.bf_create(np.ones((10, 7), np.float32), 10, 7, 7, hip.SQUARED_L2)
    assert code(lambda: src.quantize_rows(hip.ROWS_INT4, bits=8)) == hip.INVALID_ARGUMENT
    assert code(lambda: odd.quantize_rows(hip.ROWS_INT4, bits=4)) == hip.INVALID_ARGUMENT
    assert code(lambda: src.quantize_rows(hip.ROWS_INT8, mode=hip.SQ_SIGNED, bits=4)) == hip.INVALID_ARGUMENT
    from tests import quantized_rerank_cases
    base = quantized_rerank_cases.Base(36)
    tree = hip.txh_create(data=np.ascontiguousarray(base.rows), **base.desc("txh", base.rows.shape[1], hip.SQUARED_L2))
    assert code(lambda: tree.quantize_rows(hip.ROWS_INT4, bits=4)) == hip.UNIMPLEMENTED
    assert code(lambda: hip.txh_create_quantized(rows=np.zeros(base.rows.shape, np.uint8), fmt=hip.ROWS_INT4, inv_multiplier=1.0,
                                                 **base.desc("txh", base.rows.shape[1], hip.SQUARED_L2))) == hip.INVALID_ARGUMENT

"""Brute force over bit rows (SCANN_HIP_ROWS_BIN1) by Hamming distance against numpy: count the positions that differ in
int64, order by (distance, index); all exact.  The pad bits dim .. stride - 1 of every row are SET: reading them shows."""
import functools
import types

import numpy as np
import pytest

from scann_rust_amd import hip
from tests.test_gpu_quantized_bf import _device_search

pytestmark = pytest.mark.gpu

# (n, dim, stride, data): one row; a partial word; two words; 4-byte loads with pad words; 16-byte loads; two register
# chunks; more rows than the 8192-row sample (threshold and filter pass), again with 7 distinct rows repeated; density
# 0.02; a partial last word on 16-byte-loadable rows (the matrix-core pass at 70 queries)
SHAPES = [(1, 1, 32, "half"), (63, 31, 32, "half"), (257, 33, 64, "half"), (300, 70, 96, "half"),
          (513, 128, 128, "half"), (130, 2050, 2176, "half"), (20000, 256, 256, "half"),
          (513, 128, 128, "sparse"), (20000, 256, 256, "dups"), (300, 1000, 1024, "half")]


@functools.lru_cache(maxsize=None)
def case(n, dim, stride, data):
    rng = np.random.default_rng(n + dim)
    bits = rng.random((n, dim)) < (0.02 if data == "sparse" else 0.5)
    if data == "dups":
        bits = bits[:7][rng.integers(0, 7, n)]
    full = np.ones((n, stride), bool)
    full[:, :dim] = bits
    return hip.bf_create_quantized(hip.pack_bits(full), n, dim, stride, hip.ROWS_BIN1, hip.HAMMING), bits


def reference(qb, bits):
    return np.stack([(bits != q).sum(axis=1, dtype=np.int64) for q in qb]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def batch(n, dim, stride, data, nq):
    """(0/1 queries [nq][dim] f32, reference distances [nq][n] f32), the first query a copy of a row"""
    _, bits = case(n, dim, stride, data)
    qb = np.random.default_rng(nq).random((nq, dim)) < 0.5
    qb[0] = bits[n // 2]
    return qb.astype(np.float32), reference(qb, bits)


def assert_rows(idx, dist, cnt, d, k, allowed=None):
    ids = np.arange(d.shape[1]) if allowed is None else allowed
    for i in range(d.shape[0]):
        order = ids[np.lexsort((ids, d[i][ids]))][:k]
        assert cnt[i] == order.size
        assert np.array_equal(idx[i][:order.size], order) and np.array_equal(dist[i][:order.size], d[i][order])


def kernel_for(dim, stride, nq):
    """the matrix-core pass: 16-byte-loadable rows, 64 queries and more, 128 and more on rows wider than 1024 bits"""
    return "bf_hamming_mfma_kernel" if stride % 128 == 0 and nq >= (64 if dim <= 1024 else 128) else "bf_hamming_kernel"


@pytest.mark.parametrize("nq", [1, 3, 17, 70])
@pytest.mark.parametrize("n,dim,stride,data", SHAPES)
def test_search_matches_reference(n, dim, stride, data, nq):
    index, _ = case(n, dim, stride, data)
    q, d = batch(n, dim, stride, data, nq)
    index.enable_timing(True)
    for k in sorted({1, 10, min(n, 100)}):
        assert_rows(*index.search_batched(q, k), d, k)
        assert index.last_kernel_ms()[1] == kernel_for(dim, stride, nq)


@pytest.mark.parametrize("nq", [64, 130])
@pytest.mark.parametrize("n,dim,stride", [(4096, 128, 128), (4096, 1024, 1024), (20000, 256, 256), (130, 2050, 2176)])
def test_matrix_core_pass(n, dim, stride, nq):
    index, _ = case(n, dim, stride, "half")
    q, d = batch(n, dim, stride, "half", nq)
    index.enable_timing(True)
    for k in (1, 10):
        assert_rows(*index.search_batched(q, k), d, k)
        assert index.last_kernel_ms()[1] == kernel_for(dim, stride, nq)   # (the popcount kernel at 2050 bits, 64 queries)
    assert_rows(*index.search_batched(q[:3], 10), d[:3], 10)
    assert index.last_kernel_ms()[1] == "bf_hamming_kernel"


@pytest.mark.parametrize("n,dim,stride", [(300, 70, 96), (130, 2050, 2176)])
def test_distance_matrix_and_the_nonzero_rule(n, dim, stride):
    index, bits = case(n, dim, stride, "half")
    for nq in (3, 17):
        q, d = batch(n, dim, stride, "half", nq)
        assert np.array_equal(hip.bf_distances(index, q), d)
    values = np.array([0.0, -0.0, 1.0, 2.5, -3.0, np.nan], np.float32)   # bit j is q[j] != 0: NaN is a one, -0.0 a zero
    q = values[np.random.default_rng(1).integers(0, values.size, (5, dim))]
    want = reference(np.isnan(q) | (q != 0), bits)
    assert np.array_equal(hip.bf_distances(index, q), want)
    assert_rows(*index.search_batched(q, 10), want, 10)


def test_radius_search():
    index, _ = case(513, 128, 128, "half")
    q, d = batch(513, 128, 128, "half", 3)
    for radius in (0.0, 60.0, 128.0):
        sel = np.nonzero(d[0] <= radius)[0]
        order = sel[np.argsort(d[0][sel], kind="stable")]
        ri, rd, rc = hip.bf_search_radius(index, q[0], radius)
        assert rc == order.size and np.array_equal(ri, order) and np.array_equal(rd, d[0][order])


@pytest.mark.parametrize("mech", ["1", "2"])   # SCANN_HIP_BF_FILTER: compacted id list / bit test in the stream
def test_allow_bitmap(mech, monkeypatch):
    """one bitmap per call, as on every brute-force handle (they take no allow_bitmap_stride)"""
    monkeypatch.setenv("SCANN_HIP_BF_FILTER", mech)
    n, dim, stride = 300, 70, 96
    index, _ = case(n, dim, stride, "half")
    q, d = batch(n, dim, stride, "half", 17)
    mask = np.random.default_rng(3).random(n) < 0.3
    packed = hip.pack_bits(mask)
    allow = np.frombuffer(packed.tobytes() + bytes(-packed.size % 8), np.uint64).copy()
    assert_rows(*index.search_batched(q, 10, allow=allow, allow_bits=n), d, 10, allowed=np.nonzero(mask)[0])


def test_device_entry_after_reserve():
    index, _ = case(20000, 256, 256, "half")
    q, d = batch(20000, 256, 256, "half", 17)
    for exact in (False, True):   # bf_exact is accepted and changes nothing
        status, *rows = _device_search(index, q, 10, exact=exact)
        assert status == hip.OK
        assert_rows(*rows, d, 10)


def create(fmt, measure, dim=64, stride=64, n=10):
    return hip.bf_create_quantized(np.zeros((10, 8), np.uint8), n, dim, stride, fmt, measure)


@functools.lru_cache(maxsize=None)
def ctx():
    from tests import quantized_rerank_cases
    b = quantized_rerank_cases.Base(36)
    n, dim = b.rows.shape
    return types.SimpleNamespace(
        ix=create(hip.ROWS_BIN1, H), rows=np.ascontiguousarray(b.rows), dim=dim, desc=lambda m: b.desc("txh", dim, m),
        src=hip.bf_create(np.ascontiguousarray(b.rows), n, dim, dim, hip.SQUARED_L2),
        proj=hip.Projection(hip.PROJ_TRUNCATE, in_dim=dim, out_dim=dim, start=0))


Z = lambda *shape: np.zeros(shape, np.float32)
H, U, I = hip.HAMMING, hip.UNIMPLEMENTED, hip.INVALID_ARGUMENT
# Every refusal of the header with its code: the two values apart, Hamming in every other create / build call (not the
# fold call: it takes its measure from a source handle, and no source handle can hold Hamming), bit rows where rows
# would have to be binarised, and the entry points that read rows as f32 (the code each gives every quantized handle).
REFUSALS = dict(
    [("bin1_measure_%d" % m, (lambda c, m=m: create(hip.ROWS_BIN1, m), U)) for m in range(5)] +
    [("hamming_format_%d" % f, (lambda c, f=f: create(f, H, 4, 4), U)) for f in (1, 2, 3, 5)],   # BF16, FP8, INT8, INT4
    stride_40=(lambda c: create(hip.ROWS_BIN1, H, 40, 40), I),
    dim_2_24=(lambda c: create(hip.ROWS_BIN1, H, 1 << 24, 1 << 24, n=0), hip.OUT_OF_RANGE),
    bf_create=(lambda c: hip.bf_create(Z(10, 8), 10, 8, 8, H), U),
    txh_create=(lambda c: hip.txh_create(data=c.rows, **c.desc(H)), U),
    txh_create_quantized=(lambda c: hip.txh_create_quantized(rows=c.rows.astype(np.int8), fmt=hip.ROWS_INT8, **c.desc(H)), U),
    txh_create_projected=(lambda c: hip.txh_create_projected(projection=c.proj, rows=c.rows, row_dim=c.dim, **c.desc(H)), U),
    txh_build=(lambda c: hip.txh_build(c.src, distance_measure=H), U),
    txh_build_hierarchical=(lambda c: hip.txh_build_hierarchical(c.src, distance_measure=H), U),
    txh_build_projected=(lambda c: hip.txh_build_projected(c.src, c.proj, distance_measure=H), U),
    quantize_rows=(lambda c: c.src.quantize_rows(hip.ROWS_BIN1), I),
    txh_quantized_bin1=(lambda c: hip.txh_create_quantized(rows=c.rows.astype(np.uint8), fmt=hip.ROWS_BIN1,
                                                           **c.desc(hip.SQUARED_L2)), I),
    assign_nearest=(lambda c: hip.bf_assign_nearest(c.ix, Z(2, 64)), I),
    kmeans_init_pp=(lambda c: hip.kmeans_init_pp(c.ix, 2, 1), I),
    kmeans_lloyd=(lambda c: hip.kmeans_lloyd(c.ix, Z(2, 64)), I),
    search_mmr=(lambda c: c.ix.search_mmr(Z(1, 64), 2, 4, 0.5), U),
    mmr_apply=(lambda c: c.ix.mmr_apply(np.arange(4, dtype=np.uint32)[None], Z(1, 4), np.full(1, 4, np.uint32), 2, 0.5), U),
    mutable_create=(lambda c: hip.Mutable(c.ix, 16), U))


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusal(name):
    call, want = REFUSALS[name]
    with pytest.raises(hip.ScannError) as e:
        call(ctx())
    assert e.value.code == want


def test_empty_index():
    assert list(create(hip.ROWS_BIN1, H, n=0).search_batched(Z(2, 64), 5)[2]) == [0, 0]

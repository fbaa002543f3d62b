"""Tree-X-Hybrid and AsymmetricHasher indexes whose re-rank rows are stored as bf16, FP8 E4M3 or int8
(scann_hip_txh_create_quantized) against tests/quantized_rerank_model.py.

Every result row is compared BITWISE with the model fed with the ORACLE's merged candidates (orc.txh_search(...,
stages=True) / orc.ah_search: the candidate stages read no rows); the device's own candidate list is checked against
the same list the way the parity tests check it (approximate distances bitwise, membership up to their ties).  No
tolerance anywhere.  Every returned distance is also what hip.bf_distances of a quantized brute-force handle over the
same rows gives."""
import ctypes

import numpy as np
import pytest

from oracle import pyoracle as orc
from scann_rust_amd import hip, index_file
from tests import crowding_model as CM
from tests import helpers as H
from tests import quantized_checker as qc
from tests import quantized_rerank_cases as QC
from tests import quantized_rerank_model as QM

pytestmark = pytest.mark.gpu

K = 10
SENT = 0xFFFFFFFF
DATA_LOSS = 15
KINDS = ("txh", "ah")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def bases():
    cache = {}

    def get(dim, n=4096, nq=70):
        if (dim, n) not in cache:
            cache[dim, n] = QC.Base(dim, n=n, nq=nq)
        return cache[dim, n]

    yield get
    cache.clear()


def _create(base, kind, rows_q, fmt, measure, inv):
    return hip.txh_create_quantized(rows=rows_q, fmt=fmt, inv_multiplier=inv,
                                    **base.desc(kind, rows_q.shape[1], measure))


def _assert_rows(got, want, k, what):
    """got = (idx [nq, k], dist [nq, k], count [nq]); want = the model's [(idx, dist)]"""
    gi, gd, gc = got
    for i, (wi, wd) in enumerate(want):
        c = int(gc[i])
        assert c == wi.size, (what, i, c, wi.size)
        assert np.array_equal(_bits(gd[i, :c]), _bits(wd)), (what, i, gd[i, :c], wd)
        assert np.array_equal(gi[i, :c], wi), (what, i, gi[i, :c], wi)
        assert np.all(gi[i, c:k] == SENT), (what, i)


def _assert_candidates(base, kind, m, nq, stage_out, what, queries=None, p=None, allow=None):
    tok, tokd, ci, cd, cc = stage_out
    for i in range(nq):
        al = None if allow is None else (allow[i] if np.ndim(allow) == 2 else allow)
        oci, ocd = base.candidates(kind, i, m, None if queries is None else queries[i], p, al)
        c = int(cc[i])
        assert c == oci.size, (what, i, c, oci.size)
        assert np.array_equal(_bits(cd[i, :c]), _bits(ocd)), (what, i)
        H.assert_topk_equal_up_to_ties(ci[i, :c], cd[i, :c], oci, ocd, what="%s cand q%d" % (what, i))


def _assert_bf_consistent(rows_q, dim, fmt, measure, inv, queries, got, what):
    """every returned distance == the quantized brute-force handle's distance of that query and row"""
    bf = hip.bf_create_quantized(rows_q, rows_q.shape[0], dim, rows_q.shape[1], fmt, measure, inv)
    d = hip.bf_distances(bf, queries)
    gi, gd, gc = got
    for i in range(queries.shape[0]):
        c = int(gc[i])
        assert np.array_equal(_bits(gd[i, :c]), _bits(d[i, gi[i, :c].astype(np.int64)])), (what, i)


def _run(base, kind, rows_q, fmt, measure, inv, k, m, nq, what, queries=None, p=None, stages=True, bf=True):
    """one handle, one batch: plain call (final_topk_kernel) and staged call (sorted candidates, final_sort_kernel)
    against the model; returns (index, plain rows)"""
    q = (base.q if queries is None else queries)[:nq]
    index = _create(base, kind, rows_q, fmt, measure, inv)
    want = base.model_rows(kind, rows_q, fmt, measure, inv, k, m, nq, queries, p)
    got = index.search_batched(q, k, base.opts(kind, m, p))
    _assert_rows(got, want, k, what)
    if stages:
        gi, gd, gc, st = index.search_batched(q, k, base.opts(kind, m, p), stages=True)
        _assert_candidates(base, kind, m, nq, st, what, queries, p)
        _assert_rows((gi, gd, gc), want, k, what + " staged")
    if bf:
        _assert_bf_consistent(rows_q, base.dim, fmt, measure, inv, q, got, what)
    return index, got


# ---- formats x measures, on the tree and on the flat hasher ------------------------------------------------------
@pytest.mark.parametrize("measure", list(QC.MEASURES))
@pytest.mark.parametrize("fmt", list(QC.FMTS))
@pytest.mark.parametrize("kind", KINDS)
def test_formats_and_measures(bases, kind, fmt, measure):
    base = bases(96)
    elems, inv = QC.quantize(base.rows, QC.FMTS[fmt])
    _run(base, kind, QC.with_stride(elems, 96 + 5, seed=3), QC.FMTS[fmt], QC.MEASURES[measure], inv, K, 33, 17,
         "%s %s %s" % (kind, fmt, measure))


# ---- dimensions x strides ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(QC.FMTS))
@pytest.mark.parametrize("dim", [8, 12, 36, 96, 128, 264])
def test_dimensions_and_strides(bases, dim, fmt):
    """dim 12 and 36 reach the int8 tail; stride dim + 5 leaves rows unaligned (odd bytes for the byte formats) with
    junk in the padding, the next multiple of 16 keeps the vector loads with a partial last piece"""
    base = bases(dim)
    f = QC.FMTS[fmt]
    elems, inv = QC.quantize(base.rows, f)
    for si, stride in enumerate(QC.strides(dim)):
        for kind in KINDS:
            measure = list(QC.MEASURES.values())[(si + (kind == "ah")) % 3]
            _run(base, kind, QC.with_stride(elems, stride, seed=4), f, measure, inv, K, 40, 5,
                 "dim %d %s stride %d %s" % (dim, fmt, stride, kind), stages=(si == 1), bf=(si != 0))


# ---- candidate counts --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, K - 1, K, 31, 33, 257, 1000])
@pytest.mark.parametrize("kind", KINDS)
def test_candidate_counts(bases, kind, m):
    """m below, at and above k, around the 32-candidate rounds and the 256-candidate workgroup, and m = 1000: on the
    tree with two leaves probed some queries have fewer points than that (fewer candidates than m) and some have more;
    with m < k fewer than k"""
    base = bases(36)
    f = [qc.ROWS_BF16, qc.ROWS_FP8_E4M3, qc.ROWS_INT8][m % 3]
    elems, inv = QC.quantize(base.rows, f)
    p = 2 if kind == "txh" else None
    index, got = _run(base, kind, QC.with_stride(elems, 36 + 5, seed=5), f, qc.SQUARED_L2, inv, K, m, 16,
                      "%s m %d" % (kind, m), p=p, bf=False)
    if kind == "txh" and m == 1000:
        assert (got[2] == K).all()
        cc = index.search_batched(base.q[:16], K, base.opts(kind, m, p), stages=True)[3][4]
        assert (cc < m).any() and (cc == m).any()   # the premise: queries that ran out of points before m, and not
    if m < K:
        assert (got[2] == m).all()     # k above the candidate count


# ---- batch sizes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(QC.FMTS))
@pytest.mark.parametrize("kind", KINDS)
def test_batch_sizes_give_the_same_rows(bases, kind, fmt):
    base = bases(128)
    f = QC.FMTS[fmt]
    elems, inv = QC.quantize(base.rows, f)
    index, full = _run(base, kind, elems, f, qc.L2, inv, K, 64, 70, "%s %s nq 70" % (kind, fmt), stages=False, bf=False)
    for nq in (1, 3, 4, 16, 17):
        gi, gd, gc = index.search_batched(base.q[:nq], K, base.opts(kind, 64))
        assert np.array_equal(gc, full[2][:nq]) and np.array_equal(_bits(gd), _bits(full[1][:nq])) and \
            np.array_equal(gi, full[0][:nq]), (kind, fmt, nq)


@pytest.fixture(scope="module")
def big():
    """70 000 x 96: an f32 handle builds its int8 shadow store from 65 536 rows, and sends 1 or 4 queries over a
    stream this long to the wide pipeline"""
    return QC.Base(96, n=70000, nq=8, seed=21)


@pytest.mark.parametrize("fmt", list(QC.FMTS))
def test_large_index_and_device_bytes(big, fmt):
    f = QC.FMTS[fmt]
    elems, inv = QC.quantize(big.rows, f)
    stride = 96
    index, _ = _run(big, "ah", elems, f, qc.SQUARED_L2, inv, K, 300, 8, "70k %s" % fmt, stages=False, bf=False)
    for nq in (1, 4):   # an f32 handle takes the wide few-query pipeline here: this one must not
        got = index.search_batched(big.q[:nq], K, big.opts("ah", 300))
        _assert_rows(got, big.model_rows("ah", elems, f, qc.SQUARED_L2, inv, K, 300, nq), K, "70k %s nq %d" % (fmt, nq))
    f32 = hip.txh_create(**dict(big.desc("ah", stride, hip.SQUARED_L2), data=big.rows))
    saved = f32.device_bytes() - index.device_bytes()
    assert saved >= big.n * stride * (4 - elems.dtype.itemsize), (saved, f32.device_bytes(), index.device_bytes())
    assert index.device_bytes() >= elems.nbytes + big.codes.size // 2


# ---- adversarial rows --------------------------------------------------------------------------------------------
def _adversarial(fmt, elems, rng):
    """rows of the format's extreme codes written over a copy of `elems`: (rows, measures whose arithmetic stays free
    of inf - inf and 0 * inf, so that no distance is a NaN -- a NaN's sign is the platform's, see the NaN test below)"""
    e = elems.copy()
    n, dim = e.shape
    pick = rng.choice(n, 600, replace=False)
    if fmt == qc.ROWS_BF16:
        for j, code in enumerate((0x7F80, 0xFF80, 0x7F7F, 0xFF7F, 0x0001)):   # +-inf, +-largest finite, a subnormal
            rows = pick[j * 100:(j + 1) * 100]
            e[rows, rng.integers(0, dim, rows.size)] = code
        e[pick[500:600]] = 0x7F7F                                             # whole rows of the largest finite value
        return e, (qc.SQUARED_L2, qc.L2)
    if fmt == qc.ROWS_FP8_E4M3:
        codes = np.array([0x7F, 0xFF, 0x01, 0x02, 0x07, 0x81, 0x87, 0x00, 0x80, 0x08], np.uint8)   # +-480, exponent 0
        rows = pick[:500]
        e[rows[:, None], rng.integers(0, dim, (rows.size, 3))] = codes[rng.integers(0, codes.size, (rows.size, 3))]
        e[pick[500:550]] = 0x7F
        e[pick[550:600]] = 0x03
        return e, (qc.SQUARED_L2, qc.L2, qc.DOT_PRODUCT)
    e[pick[:500], rng.integers(0, dim, 500)] = -128
    e[pick[500:600]] = -128
    return e, (qc.SQUARED_L2, qc.L2, qc.DOT_PRODUCT)


@pytest.mark.parametrize("fmt", list(QC.FMTS))
@pytest.mark.parametrize("kind", KINDS)
def test_extreme_codes(bases, kind, fmt):
    base = bases(36)
    f = QC.FMTS[fmt]
    elems, inv = QC.quantize(base.rows, f)
    e, measures = _adversarial(f, elems, np.random.default_rng(8))
    q = np.ascontiguousarray(base.q[:12] + np.float32(0.25))   # strictly positive: +-inf rows give +-inf dot products
    for measure in measures:
        _run(base, kind, QC.with_stride(e, 36 + 5, seed=6), f, measure, inv, K, 257, 12,
             "%s %s extreme codes, measure %d" % (kind, fmt, measure), queries=q, stages=False)


@pytest.mark.parametrize("measure", list(QC.MEASURES))
@pytest.mark.parametrize("kind", KINDS)
def test_bf16_nan_rows_order_by_the_key_of_the_device_distance(bases, kind, measure):
    """Rows holding a NaN, and +inf beside -inf (dot products: inf - inf).  IEEE 754 leaves the sign of a NaN result
    open and the platforms differ (q - x with x = +NaN: x86 keeps +NaN, the GPU's subtraction by negated operand gives
    -NaN), so numpy cannot say on which side of the order a NaN distance falls.  The distances of these rows are
    therefore taken from the quantized brute-force handle on the device (bit for bit: its own tests pin it), and the
    model's rule is applied to them: stable order by the f32_to_ordered key (-NaN first, +NaN last) in merged order."""
    base = bases(36)
    elems, _ = QC.quantize(base.rows, qc.ROWS_BF16)
    rng = np.random.default_rng(12)
    pick = rng.choice(base.n, 900, replace=False)
    for j, code in enumerate((0x7FC0, 0xFFC0, 0x7F81)):
        elems[pick[j * 200:(j + 1) * 200], rng.integers(0, 36, 200)] = code
    elems[pick[600:750], 3] = 0x7F80
    elems[pick[600:750], 17] = 0xFF80
    elems[pick[750:900]] = 0x7FC0
    ms, m, nq = QC.MEASURES[measure], 257, 12
    q = np.ascontiguousarray(base.q[:nq] + np.float32(0.25))
    index = _create(base, kind, elems, qc.ROWS_BF16, ms, 1.0)
    gi, gd, gc = index.search_batched(q, K, base.opts(kind, m))
    d = hip.bf_distances(hip.bf_create_quantized(elems, base.n, 36, 36, qc.ROWS_BF16, ms, 1.0), q)
    seen_nan = 0
    for i in range(nq):
        ci, _ = base.candidates(kind, i, m, q[i])
        dc = d[i, ci.astype(np.int64)]
        order = np.argsort(QM.f32_to_ordered(dc), kind="stable")[:K]
        assert int(gc[i]) == order.size and np.array_equal(_bits(gd[i]), _bits(dc[order])), (kind, measure, i)
        assert np.array_equal(gi[i], ci[order]), (kind, measure, i)
        seen_nan += int(np.isnan(dc).sum())
    assert seen_nan > 0


@pytest.mark.parametrize("fmt", list(QC.FMTS))
@pytest.mark.parametrize("kind", KINDS)
def test_duplicated_rows_and_zero_query(bases, kind, fmt):
    """rows i and i + 7 j equal: exact ties everywhere, which fall to the merged order; and a zero query"""
    base = bases(36)
    f = QC.FMTS[fmt]
    elems, inv = QC.quantize(base.rows[np.arange(base.n) % 7], f)
    q = base.q[:9].copy()
    q[4] = 0.0
    for measure in QC.MEASURES.values():
        index, got = _run(base, kind, elems, f, measure, inv, K, 100, 9, "%s %s duplicates" % (kind, fmt), queries=q,
                          stages=(measure == qc.L2))
        assert all(np.unique(_bits(got[1][i])).size < K for i in range(9))   # ties among the k best of every query


@pytest.mark.parametrize("kind", KINDS)
def test_int8_inv_multiplier_extremes(bases, kind):
    """a subnormal inv_multiplier (every decoded value subnormal or zero) and a huge one (every decoded value but 0
    overflows: distances +inf, ties by merged order)"""
    base = bases(36)
    elems, _ = QC.quantize(base.rows, qc.ROWS_INT8)
    elems[::25] = 0    # rows that stay finite under the huge multiplier: two or three of a query's 64 candidates
    for inv, measures in ((1e-40, tuple(QC.MEASURES.values())), (1e37, (qc.SQUARED_L2, qc.L2))):
        for measure in measures:
            index, got = _run(base, kind, elems, qc.ROWS_INT8, measure, inv, K, 64, 8,
                              "%s int8 inv %g measure %d" % (kind, inv, measure), stages=False)
            if inv > 1:
                assert np.isposinf(got[1]).any() and np.isfinite(got[1]).any()


@pytest.mark.parametrize("family", ["offset", "overflow-all", "overflow-most", "near-overflow", "tiny", "magnitudes",
                                    "spike", "permuted", "duplicates"])
def test_rerank_row_families_as_bf16(family):
    """helpers.rerank_rows' families keep f32's exponent range, which bf16 shares: quantized as they are (FP8 and int8
    clip or flush most of them, so those formats take the hand-written codes above)"""
    n, dim, nq = 9000, 64, 6
    d = H.rerank_rows(family, n, dim, nq, seed=5)
    rows_q = qc.bf16_from_f32(d["rows"])
    q = d["queries"]
    kw = {k: v for k, v in H.ah_kwargs_from_codes(d["rows"], d["codebook"], d["codes"]).items()
          if k not in ("data", "stride")}
    index = hip.txh_create_quantized(rows=rows_q, fmt=qc.ROWS_BF16, stride=dim, distance_measure=hip.SQUARED_L2, **kw)
    o = hip.default_opts()
    o.pre_reorder_k = 512
    got = index.search_batched(q, K, o)
    want = []
    for i in range(nq):
        ci, cd = orc.ah_search(d["codebook"], d["codes"], q[i], 512)
        ci, _ = QC.merged_order(ci, cd, ci)   # a flat hasher's merge key is the datapoint index
        want.append(QM.rerank(q[i], ci, rows_q, dim, qc.ROWS_BF16, qc.SQUARED_L2, 1.0, K))
    _assert_rows(got, want, K, family)


# ---- entry points ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def int8_tree(bases):
    base = bases(36)
    elems, inv = QC.quantize(base.rows, qc.ROWS_INT8)
    rows_q = QC.with_stride(elems, 36 + 5, seed=7)
    return base, rows_q, inv, _create(base, "txh", rows_q, qc.ROWS_INT8, qc.SQUARED_L2, inv)


def test_allow_bitmap_with_fewer_than_m_allowed(int8_tree):
    base, rows_q, inv, index = int8_tree
    rng = np.random.default_rng(3)
    allow = hip.allow_bitmap(base.n, rng.choice(base.n, 30, replace=False))
    m, nq = 33, 12
    gi, gd, gc, st = index.search_batched(base.q[:nq], K, base.opts("txh", m), stages=True, allow=allow)
    assert (st[4] < m).all()    # the premise: the filter leaves every query fewer than m candidates
    _assert_candidates(base, "txh", m, nq, st, "allow", allow=allow)
    want = base.model_rows("txh", rows_q, qc.ROWS_INT8, qc.SQUARED_L2, inv, K, m, nq, allow=allow)
    _assert_rows((gi, gd, gc), want, K, "allow staged")
    _assert_rows(index.search_batched(base.q[:nq], K, base.opts("txh", m), allow=allow), want, K, "allow")


def test_allow_bitmap_per_query(int8_tree):
    base, rows_q, inv, index = int8_tree
    rng = np.random.default_rng(4)
    m, nq = 33, 9
    allow = np.stack([hip.allow_bitmap(base.n, rng.choice(base.n, 40 + 400 * i, replace=False)) for i in range(nq)])
    want = base.model_rows("txh", rows_q, qc.ROWS_INT8, qc.SQUARED_L2, inv, K, m, nq, allow=allow)
    _assert_rows(index.search_batched(base.q[:nq], K, base.opts("txh", m), allow=allow), want, K, "allow per query")


def test_search_batched_params_mixed_k(int8_tree):
    base, rows_q, inv, index = int8_tree
    ks = np.array([1, 10, 5, 33, 2, 10, 7, 1, 20], np.uint32)
    m = 33
    gi, gd, gc = index.search_batched_with_params(base.q[:ks.size], ks, base.opts("txh", m))
    want = base.model_rows("txh", rows_q, qc.ROWS_INT8, qc.SQUARED_L2, inv, ks, m, ks.size)
    for i, (wi, wd) in enumerate(want):
        c = int(gc[i])
        assert c == wi.size and np.array_equal(_bits(gd[i, :c]), _bits(wd)) and np.array_equal(gi[i, :c], wi), i


def test_device_entry_point_on_a_caller_stream(int8_tree):
    import torch
    base, rows_q, inv, index = int8_tree
    m, nq = 257, 21
    o = base.opts("txh", m)
    hip.check(hip.load().scann_hip_index_reserve(index.h, nq, K, ctypes.byref(o)))
    with torch.cuda.stream(torch.cuda.Stream(torch.device("cuda:0"))):
        status, gi, gd, gc = H.device_search(index, base.q[:nq], K, o)
    assert status == 0
    _assert_rows((gi, gd, gc), base.model_rows("txh", rows_q, qc.ROWS_INT8, qc.SQUARED_L2, inv, K, m, nq), K, "device")


def test_search_crowded(int8_tree):
    base, rows_q, inv, index = int8_tree
    depth, limit, nq, m = 40, 2, 10, 64
    attrs = (np.arange(base.n, dtype=np.uint64) % np.uint64(5))
    index.set_crowding_attributes(attrs)
    try:
        gi, gd, gc = index.search_crowded(base.q[:nq], K, depth, limit, base.opts("txh", m))
    finally:
        index.set_crowding_attributes(None)
    rows = base.model_rows("txh", rows_q, qc.ROWS_INT8, qc.SQUARED_L2, inv, depth, m, nq)
    for i, (ri, rd) in enumerate(rows):
        wi, wd = CM.apply_fast(ri, rd, attrs, limit, K)
        c = int(gc[i])
        assert c == wi.size and np.array_equal(gi[i, :c], wi) and np.array_equal(_bits(gd[i, :c]), _bits(wd)), i


def test_without_exact_reorder_no_row_is_read(bases):
    """exact_reorder = 0: the k best by approximate distance, as on an f32 handle"""
    base = bases(36)
    elems, inv = QC.quantize(base.rows, qc.ROWS_BF16)
    elems[:] = 0x7FC0    # any row read would show as a NaN
    index = _create(base, "ah", elems, qc.ROWS_BF16, qc.SQUARED_L2, 1.0)
    o = hip.default_opts()
    o.exact_reorder = 0
    gi, gd, gc = index.search_batched(base.q[:8], K, o)
    for i in range(8):
        oi, od = orc.ah_search(base.cb, base.codes, base.q[i], K)
        assert int(gc[i]) == K and np.array_equal(_bits(gd[i]), _bits(od))
        H.assert_topk_equal_up_to_ties(gi[i], gd[i], oi, od, what="approx q%d" % i)


# ---- index files -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(QC.FMTS))
@pytest.mark.parametrize("kind", KINDS)
def test_index_file_round_trip(tmp_path, bases, kind, fmt):
    base = bases(36)
    f = QC.FMTS[fmt]
    elems, inv = QC.quantize(base.rows, f)
    rows_q = QC.with_stride(elems, 36 + 5, seed=9)
    index = _create(base, kind, rows_q, f, qc.DOT_PRODUCT, inv)
    path = str(tmp_path / "q.scannidx")
    hip.index_write_file(index, path)
    info = hip.index_file_info(path)
    assert info["has_data"] == 0 and info["stride"] == 41 and info["distance_measure"] == hip.DOT_PRODUCT
    a = index_file.arrays(path)
    assert "data" not in a and a["fmt"] == f and np.array_equal(a["rows_q"], rows_q)
    assert np.float32(a["inv_multiplier"]) == np.float32(inv if f == qc.ROWS_INT8 else 1.0)
    loaded = hip.load_file(path)
    o = base.opts(kind, 64)
    a0, a1 = index.search_batched(base.q[:20], K, o), loaded.search_batched(base.q[:20], K, o)
    assert np.array_equal(a0[2], a1[2]) and np.array_equal(_bits(a0[1]), _bits(a1[1])) and np.array_equal(a0[0], a1[0])
    _assert_rows(a1, base.model_rows(kind, rows_q, f, qc.DOT_PRODUCT, inv, K, 64, 20), K, "loaded")
    assert loaded.device_bytes() == index.device_bytes()


def test_index_file_with_short_rows_q_is_data_loss(tmp_path, bases):
    base = bases(36)
    elems, inv = QC.quantize(base.rows, qc.ROWS_BF16)
    kw = base.desc("ah", 36, hip.SQUARED_L2)
    S, Kc, dsub = kw["codebook"].shape

    def write(path, rows, meta=None):
        secs = index_file.rows_q_sections(rows, qc.ROWS_BF16)
        if meta is not None:
            secs[1] = ("rows_q_meta", np.asarray(meta, np.uint32))
        index_file.write(path, kind=1, n_rows=base.n, n_local=base.n, dim=36, stride=36, num_subspaces=S,
                         num_codes=Kc, dims_per_subspace=dsub, use_residuals=0, partitions_to_search=1,
                         pre_reorder_multiplier=3.0, sections=secs + [("codebook", kw["codebook"]), ("codes", kw["codes"])])

    good, short, badfmt = (str(tmp_path / n) for n in ("good.scannidx", "short.scannidx", "fmt.scannidx"))
    write(good, elems)
    assert hip.load_file(good).size() == base.n
    write(short, elems[:-1])
    write(badfmt, elems, meta=[9, 0])
    for path in (short, badfmt):
        with pytest.raises(hip.ScannError) as e:
            hip.load_file(path)
        assert e.value.code == DATA_LOSS, path


# ---- refusals ----------------------------------------------------------------------------------------------------
def _code(fn):
    with pytest.raises(hip.ScannError) as e:
        fn()
    return e.value.code, e.value.message


def test_create_refusals(bases):
    base = bases(36)
    elems, inv = QC.quantize(base.rows, qc.ROWS_INT8)
    txh, ah = base.desc("txh", 36, hip.SQUARED_L2), base.desc("ah", 36, hip.SQUARED_L2)
    create = lambda kw, rows=elems, fmt=qc.ROWS_INT8, inv=inv: hip.txh_create_quantized(rows=rows, fmt=fmt,
                                                                                        inv_multiplier=inv, **kw)
    L = hip.load()
    # InvalidArgument: desc.data set, rows NULL, unknown formats, a non-finite int8 inv_multiplier
    d, keep = hip._txh_desc(**dict(ah, data=base.rows))
    h = ctypes.c_void_p()
    assert L.scann_hip_txh_create_quantized(hip.context(), ctypes.byref(d), elems.ctypes.data, qc.ROWS_INT8,
                                            ctypes.c_float(inv), ctypes.byref(h)) == hip.INVALID_ARGUMENT
    assert _code(lambda: create(ah, rows=None))[0] == hip.INVALID_ARGUMENT
    for fmt in (0, 4, 7, -1):
        assert _code(lambda: create(ah, fmt=fmt))[0] == hip.INVALID_ARGUMENT
    for bad in (float("inf"), float("-inf"), float("nan")):
        assert _code(lambda: create(ah, inv=bad))[0] == hip.INVALID_ARGUMENT
        hip.txh_create_quantized(rows=qc.bf16_from_f32(base.rows), fmt=qc.ROWS_BF16, inv_multiplier=bad, **ah)   # ignored
    # ... and what scann_hip_txh_create validates: stride < dim, a leaf id past n_rows, too few rows for the hasher
    assert _code(lambda: create(dict(ah, stride=35)))[0] == hip.INVALID_ARGUMENT
    ids = txh["leaf_ids"].copy()
    ids[5] = base.n
    assert _code(lambda: create(dict(txh, leaf_ids=ids)))[0] == hip.INVALID_ARGUMENT
    assert _code(lambda: create(dict(ah, n_rows=base.n - 1)))[0] == hip.INVALID_ARGUMENT
    # Unimplemented: L1, Cosine, leaf-sharded descriptors, Partitioned descriptors
    for measure in (hip.L1, hip.COSINE):
        assert _code(lambda: create(dict(ah, distance_measure=measure)))[0] == hip.UNIMPLEMENTED
    sizes = (txh["leaf_offsets"][1:] - txh["leaf_offsets"][:-1]).astype(np.uint32)
    assert _code(lambda: create(dict(txh, leaf_sizes_global=sizes)))[0] == hip.UNIMPLEMENTED
    assert _code(lambda: create(dict(txh, data_is_csr_order=True)))[0] == hip.UNIMPLEMENTED
    assert _code(lambda: create(dict(txh, codebook=None, codes=None)))[0] == hip.UNIMPLEMENTED


def test_entry_points_that_refuse_quantized_rows(bases):
    import torch
    base = bases(36)
    elems, inv = QC.quantize(base.rows, qc.ROWS_INT8)
    L = hip.load()
    null = ctypes.c_void_p()

    def named(code_msg, code=hip.UNIMPLEMENTED):
        assert code_msg[0] == code and "quantized rows" in code_msg[1], code_msg

    for kind in KINDS:
        index = _create(base, kind, elems, qc.ROWS_INT8, qc.SQUARED_L2, inv)
        named(_code(lambda: index.search_mmr(base.q[:3], 5, 20, 0.5)))
        named(_code(lambda: hip.Mutable(index, 64)))
        named(_code(lambda: index.debug_rerank_brackets(1, 8)))
        o = hip.default_opts()
        named(_code(lambda: hip.check(L.scann_hip_txh_search_local_device(index.h, null, 1, 36, 5, ctypes.byref(o), null,
                                                                          null, null, null, null))))
    # rebase of a mutable index onto such a base
    f32 = hip.txh_create(**dict(base.desc("txh", 36, hip.SQUARED_L2), data=base.rows))
    mut = hip.Mutable(f32, 64)
    named(_code(lambda: mut.rebase(index)))
    # the leaf-sharded entry point (a one-rank communicator)
    comm = hip.Comm(hip.Comm.unique_id(), 0, 1)
    dev = torch.device("cuda", 0)
    qd = torch.from_numpy(base.q[:2].copy()).to(dev)
    oi = torch.empty((2, 5), dtype=torch.int32, device=dev)
    od = torch.empty((2, 5), dtype=torch.float32, device=dev)
    oc = torch.empty((2,), dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    named(_code(lambda: hip.check(L.scann_hip_txh_search_sharded_device(index.h, comm.h, p(qd), 2, 36, 5, None, 0, p(oi),
                                                                        p(od), p(oc), null))))
    torch.cuda.synchronize()

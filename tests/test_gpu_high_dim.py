"""Every search and build entry point at embedding-sized dimensionalities (768 .. 4096), where no fast path applies
and the generic kernels size their LDS, their queries per tile and their pass counts from `dim`.

The dims come from tests/high_dim_cases.py: both sides of every 64 KB edge (launch.h sets the dynamic-LDS attribute only
above it), of every 160 KB edge (a launcher takes a smaller tile or another kernel) and of every change of the queries
per tile, the common embedding sizes, and one dim that is no multiple of 4 at a tight stride.  Every result is compared
with the CPU oracle or the suite's numpy models by the standard of the entry point's existing tests: distances bit for
bit, indices equal or equal up to ties of the distance.  There is no tolerance anywhere.

The last three tests run dim 6144, above the ceiling of every kernel that stages eight f32 rows in LDS: every entry
point either answers as the oracle does or refuses with ResourceExhausted, never with a launch error, does the same for
1 and for 17 queries, and does what the ceilings of tests/high_dim_cases.py (DESIGN.md "Dimensionality ceilings")
predict.  Those refusals are host-side returns before any launch."""
import numpy as np
import pytest

from oracle import pyoracle as orc
from scann_rust_amd import hip, synth, trainer
from tests import build_model as BM
from tests import crowding_model as CM
from tests import diversify_model as DM
from tests import fold_model as fm
from tests import helpers as H
from tests import high_dim_cases as HC
from tests import high_dim_checks as CK
from tests import mutable_model as mm
from tests import quantized_checker as qc
from tests import quantized_rerank_cases as QC
from tests import scalar_quantizer_model as SQM

pytestmark = pytest.mark.gpu

SQL2, L2, DOT, L1, COS = hip.SQUARED_L2, hip.L2, hip.DOT_PRODUCT, hip.L1, hip.COSINE
MEASURES = (SQL2, L2, DOT, L1, COS)
FMTS = {"bf16": hip.ROWS_BF16, "fp8": hip.ROWS_FP8_E4M3, "int8": hip.ROWS_INT8}
EMPTY = 0xFFFFFFFF
K = 10


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    yield
    _TXH.clear()
    _AH.clear()


# =====================================================================================================================
# 1. brute force over f32 rows
# =====================================================================================================================
class BfCase:
    """one f32 brute-force handle over U[-1, 1) rows with its oracle view; query 2 is a row (distance 0 or a tie)"""

    def __init__(self, dim, measure, n=HC.BF_ROWS, nq=HC.NQ):
        self.dim, self.measure, self.n = dim, measure, n
        self.stride = HC.stride_of(dim)
        self.rows = HC.signed_rows(n, dim, 11)
        self.q = HC.signed_rows(nq, dim, 12)
        self.q[2] = self.rows[17]
        self.data = HC.strided(self.rows, self.stride)
        self.index = hip.bf_create(self.data, n, dim, self.stride, measure)
        self.index.enable_timing(True)
        self.top = orc.bf_search_batched(self.data, n, dim, self.stride, measure, self.q, K)

    def assert_rows(self, idx, dist, cnt, nq, k, what):
        oi, od, oc = self.top
        for i in range(nq):
            assert cnt[i] == k, "%s q%d: count %d" % (what, i, cnt[i])
            H.assert_topk_equal_up_to_ties(idx[i, :k], dist[i, :k], oi[i, :k], od[i, :k], what="%s q%d" % (what, i))


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("dim", HC.BF_F32_DIMS)
def test_bf_f32_search(dim, measure, monkeypatch):
    """host entry with the default knobs (the small-batch pipeline up to 16 queries) and with SCANN_HIP_SMALL=0 (the
    pass kernels at every batch size, named), the device entry, and the dense distance matrix"""
    c = BfCase(dim, measure)
    for small in ("1", "0"):
        monkeypatch.setenv("SCANN_HIP_SMALL", small)
        for nq in HC.BATCHES:
            for k in (1, K):
                what = "dim %d m%d small=%s nq %d k %d" % (dim, measure, small, nq, k)
                idx, dist, cnt = c.index.search_batched(c.q[:nq], k)
                if small == "0" or nq > 16:
                    assert c.index.last_kernel_ms()[1] == HC.bf_pass_kernel(measure, dim, c.stride, nq), what
                c.assert_rows(idx, dist, cnt, nq, k, what)
    monkeypatch.delenv("SCANN_HIP_SMALL")
    for nq in HC.BATCHES:
        for k in (1, K):
            status, di, dd, dc = H.device_search(c.index, c.q[:nq], k, hip.default_opts())
            assert status == hip.OK, "device dim %d m%d nq %d k %d: status %d" % (dim, measure, nq, k, status)
            c.assert_rows(di, dd, dc, nq, k, "device dim %d m%d nq %d k %d" % (dim, measure, nq, k))
    for nq in (3, 17):
        got = hip.bf_distances(c.index, c.q[:nq])
        for i in range(nq):
            want = orc.one_to_many(c.q[i], c.data, c.stride, c.n, measure)
            assert np.array_equal(bits(got[i]), bits(want)), "bf_distances dim %d m%d nq %d q%d" % (dim, measure, nq, i)


@pytest.mark.parametrize("measure", MEASURES)
def test_bf_f32_radius_and_shared_allow_bitmap(measure, monkeypatch):
    """bf_search_radius and a shared allow-bitmap (brute-force handles take no per-query bitmaps: the per-query form
    runs on the tree below) at dim 4096: the filtered passes use the same launchers"""
    c = BfCase(4096, measure, nq=17)
    for i in (0, 2):
        d = orc.one_to_many(c.q[i], c.data, c.stride, c.n, measure)
        radius = float(np.sort(d)[25])
        oi, od = orc.bf_search_radius(c.data, c.n, c.dim, c.stride, measure, c.q[i], radius)
        gi, gd, found = hip.bf_search_radius(c.index, c.q[i], radius)
        assert found == oi.size and np.array_equal(bits(gd), bits(od))
        H.assert_topk_equal_up_to_ties(gi, gd, oi, od, what="radius q%d" % i)
    allowed = np.flatnonzero(np.random.default_rng(5).random(c.n) < 0.3)
    words, cap = H.words_of(allowed, c.n)
    sub = HC.strided(c.rows[allowed], c.stride)
    oi, od, oc = orc.bf_search_batched(sub, allowed.size, c.dim, c.stride, measure, c.q, K)
    for small in ("1", "0"):
        monkeypatch.setenv("SCANN_HIP_SMALL", small)
        for nq in (1, 16, 17):
            idx, dist, cnt = c.index.search_batched(c.q[:nq], K, allow=words, allow_bits=cap)
            for i in range(nq):
                assert cnt[i] == K and np.isin(idx[i], allowed).all()
                H.assert_topk_equal_up_to_ties(idx[i], dist[i], allowed[oi[i].astype(np.int64)], od[i],
                                               what="allow small=%s nq %d q%d" % (small, nq, i))


# =====================================================================================================================
# 2. brute force over quantized rows
# =====================================================================================================================
def quantized_rows(fmt, rows, stride, seed):
    """([n, stride] elements with junk in the padding, inv_multiplier) by the host quantizers"""
    elems, inv = QC.quantize(rows, fmt)
    return QC.with_stride(elems, stride, seed), inv


def assert_quantized_topk(idx, dist, cnt, d, k, what):
    """distances = the oracle TopK's over the checker's distances, bitwise; indices by (distance, index) key"""
    oi, od = orc.topk_run(min(k, d.size), np.arange(d.size, dtype=np.uint32), d)
    c = int(cnt)
    assert c == oi.size, what
    assert np.array_equal(bits(dist[:c]), bits(od)), what
    order = np.lexsort((np.arange(d.size), ordered_key(d)))[:c]
    assert np.array_equal(np.asarray(idx[:c], np.int64), order), what


def ordered_key(d):
    b = bits(d)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))   # common.h f32_to_ordered


@pytest.mark.parametrize("fmt", list(FMTS))
@pytest.mark.parametrize("dim", HC.BF_QUANT_DIMS)
def test_bf_quantized_rows(dim, fmt):
    """bf_create_quantized over host-quantized rows, and quantize_rows of the f32 handle: the dense matrix bitwise
    against the checker at 2 queries (one query pair per workgroup row) and 9 (four pairs), and the top-k"""
    n, f = 1000, FMTS[fmt]
    rows = HC.signed_rows(n, dim, 21)
    q = HC.signed_rows(9, dim, 22)
    stride = HC.stride_of(dim)
    rows_q, inv = quantized_rows(f, rows, stride, 23)
    for measure in (SQL2, DOT, L2):
        index = hip.bf_create_quantized(rows_q, n, dim, stride, f, measure, inv)
        want = qc.distances(q, rows_q, dim, f, measure, inv)
        for nq in (2, 9):
            what = "dim %d %s m%d nq %d" % (dim, fmt, measure, nq)
            got = hip.bf_distances(index, q[:nq])
            assert np.array_equal(bits(got), bits(want[:nq])), what
            idx, dist, cnt = index.search_batched(q[:nq], K)
            for i in range(nq):
                assert_quantized_topk(idx[i], dist[i], cnt[i], want[i], K, "%s q%d" % (what, i))
        index.close()
    # quantize_rows: the device's conversion of an f32 handle answers as the handle over the model's bytes
    src = hip.bf_create(HC.strided(rows, stride), n, dim, stride, SQL2)
    got, _ = src.quantize_rows(f)
    if f == hip.ROWS_INT8:
        codes, params, _ = SQM.rows_int8(rows, stride, 8, hip.SQ_SIGNED, 0.0, 0.0)
        twin_rows, twin_inv = codes, float(params[2])
    else:
        elems = qc.bf16_from_f32(rows) if f == hip.ROWS_BF16 else orc.fp8_quantize(rows, 1.0)
        twin_rows, twin_inv = np.zeros((n, stride), elems.dtype), 1.0
        twin_rows[:, :dim] = elems
    want = qc.distances(q, twin_rows, dim, f, SQL2, twin_inv)
    for nq in (2, 9):
        assert np.array_equal(bits(hip.bf_distances(got, q[:nq])), bits(want[:nq])), "quantize_rows dim %d %s nq %d" % (dim, fmt, nq)


# =====================================================================================================================
# 3. Partitioned mode: centroid_scores_kernel + leaf_exact_scan_kernel
# =====================================================================================================================
def partition_case(n, dim, L, seed):
    rows = HC.signed_rows(n, dim, seed)
    stride = HC.stride_of(dim)
    data = HC.strided(rows, stride)
    centers, assign = trainer.kmeans(rows, L, iters=2, seed=seed)
    order = np.argsort(assign, kind="stable").astype(np.uint32)
    leaf_off = np.zeros(centers.shape[0] + 1, np.uint32)
    leaf_off[1:] = np.cumsum(np.bincount(assign, minlength=centers.shape[0]))
    return rows, data, stride, np.ascontiguousarray(centers, np.float32), leaf_off, order


@pytest.mark.parametrize("measure", MEASURES)
@pytest.mark.parametrize("dim", HC.PARTITIONED_DIMS)
def test_partitioned_mode(dim, measure):
    """search_partitioned: distances bit for bit and identical indices.  70 queries over 5 of 6 leaves: about 58
    queries per leaf, several groups of qpt * 4 queries per tile and a partial one; 3 queries: the small pipeline"""
    n, L, P = 1500, 6, 5
    rows, data, stride, centers, leaf_off, leaf_ids = partition_case(n, dim, L, 31)
    index = hip.txh_create(data=data, n_rows=n, dim=dim, stride=stride, centers=centers, leaf_offsets=leaf_off,
                           leaf_ids=leaf_ids, codebook=None, codes=None, partitions_to_search=P, distance_measure=measure)
    q = HC.signed_rows(HC.NQ, dim, 32)
    q[3] = rows[17]
    want = [orc.scann_search_partitioned(centers, leaf_off, leaf_ids, data, stride, measure, q[i], P, K)
            for i in range(HC.NQ)]
    for nq in (3, 17, HC.NQ):
        idx, dist, cnt = index.search_batched(q[:nq], K)
        for i in range(nq):
            oi, od = want[i]
            what = "dim %d m%d nq %d q%d" % (dim, measure, nq, i)
            assert cnt[i] == oi.size, what
            assert np.array_equal(bits(dist[i, :oi.size]), bits(od)), what
            assert np.array_equal(idx[i, :oi.size], oi), what


@pytest.mark.parametrize("dim", HC.PARTITION4_DIMS + HC.PARTITION16_DIMS + (HC.PARTITION16_TOO_WIDE,))
def test_txh_partition_both_forms_of_centroid_scores(dim):
    """centroid_scores_kernel<4> (a grid that does not fill the chip) at dim 4096 / 4100 and <16> (L = 8192, nq = 1024)
    at dim 1024 / 1040 -- at dim 2564 that grid takes <4>, 16 queries being more than 160 KB: tokens and distance bits
    of a sample of queries against the oracle"""
    wide = dim not in HC.PARTITION4_DIMS
    L, nq, P = (8192, 1024, 3) if wide else (6, HC.NQ, 4)
    assert HC.centroid_qt(dim, L, nq) == (16 if dim in HC.PARTITION16_DIMS else 4)
    centers = HC.signed_rows(L, dim, 41)
    data, stride = orc.to_strided(centers)       # one row per leaf: the partitioner reads the centres and the leaf sizes
    index = hip.txh_create(data=data, n_rows=L, dim=dim, stride=stride, centers=centers,
                           leaf_offsets=np.arange(L + 1, dtype=np.uint32), leaf_ids=np.arange(L, dtype=np.uint32),
                           codebook=None, codes=None, partitions_to_search=P)
    q = HC.signed_rows(nq, dim, 42)
    q[5] = centers[L - 1]
    tok, dist, cnt = hip.txh_partition(index, q, P)
    for i in sorted(set(range(0, nq, max(1, nq // 24))) | {5, nq - 1}):
        ot, od = orc.partition(centers, q[i], P)
        assert cnt[i] == ot.size
        assert np.array_equal(bits(dist[i, :ot.size]), bits(od)), (dim, i)
        assert np.array_equal(tok[i, :ot.size], ot), (dim, i)


# =====================================================================================================================
# 4. tree and flat-hasher indexes
# =====================================================================================================================
_TXH, _AH = {}, {}


def txh_case(name):
    if name not in _TXH:
        n, dim, L, S, Kc, res = HC.TXH_SHAPES[name]
        if Kc == 256:     # byte codes: 256 rows' subvectors as the codebook (training 256 codewords takes ~10 s)
            rows = synth.uniform_f32(n, dim, 50 + S)
            pick = np.random.default_rng(S).choice(n, Kc, replace=False)
            cb = np.ascontiguousarray(rows[pick].reshape(Kc, S, dim // S).transpose(1, 0, 2), np.float32)
            oix, kw = H.txh_from_codes(rows, cb, trainer.encode(cb, rows, chunk=2048), L, HC.TXH_P, HC.TXH_MULT,
                                       seed=50 + S, use_residuals=res)
            data, stride, ix = kw["data"], kw["stride"], dict(codebook=cb, codes=kw["codes"])
        else:
            rows, data, stride, ix, oix, kw = H.make_txh_case(n, dim, L, S, seed=50 + S, K=Kc, use_residuals=res,
                                                              P=HC.TXH_P, mult=HC.TXH_MULT, kmeans_iters=2, pq_iters=2)
        q = synth.uniform_f32(HC.NQ, dim, 60 + S)
        _TXH[name] = dict(rows=rows, data=data, stride=stride, ix=ix, oix=oix, kw=kw, q=q, dim=dim, S=S, K=Kc, n=n, L=L)
    return _TXH[name]


def ah_case(name):
    if name not in _AH:
        n, dim, S = HC.AH_SHAPES[name]
        rows, data, stride, ix, kw = H.make_ah_case(n, dim, S, seed=70 + S, pq_iters=2)
        q = synth.uniform_f32(HC.NQ, dim, 80 + S)
        _AH[name] = dict(rows=rows, data=data, stride=stride, ix=ix, kw=kw, q=q, dim=dim, S=S, n=n)
    return _AH[name]


def txh_opts(k=K):
    o = hip.default_opts()
    o.partitions_to_search, o.pre_reorder_k = HC.TXH_P, orc.pre_reorder_k(k, HC.TXH_MULT)
    return o


def ah_opts(m=40):
    o = hip.default_opts()
    o.pre_reorder_k = m
    return o


def check_staged(kind, c, o, q, k, staged, qs, what):
    idx, dist, cnt, (tok, tokd, ci, cd, cc) = staged
    for i in qs:
        w = "%s q%d" % (what, i)
        if kind == "ah":
            H.check_ah_query(c["ix"]["codebook"], c["ix"]["codes"], c["data"], c["stride"], c["dim"], q[i], k,
                             o.pre_reorder_k, idx[i, :cnt[i]], dist[i, :cnt[i]], ci[i, :cc[i]], cd[i, :cc[i]], what=w)
        else:
            H.check_txh_query(c["oix"], q[i], k, idx[i, :cnt[i]], dist[i, :cnt[i]], tok[i], tokd[i], ci[i, :cc[i]],
                              cd[i, :cc[i]], what=w)


def fast_equals_staged(fast, staged, what):
    idx2, dist2, cnt2 = fast
    idx, dist, cnt = staged[:3]
    assert np.array_equal(cnt2, cnt), what + ": counts"
    assert np.array_equal(bits(dist2), bits(dist)), what + ": distances"
    for i in range(idx.shape[0]):
        H.assert_topk_equal_up_to_ties(idx2[i, :cnt[i]], dist2[i, :cnt[i]], idx[i, :cnt[i]], dist[i, :cnt[i]],
                                       what="%s fast q%d" % (what, i))


def run_scans(kind, c, o, name, monkeypatch):
    """the default scan choice and every forced scan: at these shapes the plan accepts every forced scan, so each must
    run its own kernel (the resident layout holds S <= 32 and byte codes have no prefilter: those take the LDS-gather
    scan); the staged outputs match the oracle stage by stage and the fast path's rows equal the staged ones"""
    q = c["q"]
    ran = {}
    for scan in H.SCANS:
        H.scan_env(monkeypatch, scan)
        monkeypatch.setenv("SCANN_HIP_SMALL", "0")
        index = hip.txh_create(**c["kw"])
        index.enable_timing(True)
        what = "%s %s %s" % (kind, name, scan)
        staged = index.search_batched(q, K, o, stages=True)
        ran[scan] = index.last_kernel_ms()[1]
        forced = H.scan_kernel_name(scan, c["S"]) if c.get("K", 16) == 16 else "adc_scan_kernel"
        if scan != "default":      # (the plan accepts every forced scan at these shapes; the default choice is its own)
            assert ran[scan] == forced, what + ": " + ran[scan]
        check_staged(kind, c, o, q, K, staged, range(0, HC.NQ, 6), what)
        fast = index.search_batched(q, K, o)
        fast_equals_staged(fast, staged, what)
        index.close()
    print(kind, name, ran)
    assert ran["gather"] == "adc_scan_kernel"


@pytest.mark.parametrize("name", list(HC.TXH_SHAPES))
def test_tree_every_scan(name, monkeypatch):
    run_scans("txh", txh_case(name), txh_opts(), name, monkeypatch)


@pytest.mark.parametrize("name", list(HC.AH_SHAPES))
def test_flat_hasher_every_scan(name, monkeypatch):
    run_scans("ah", ah_case(name), ah_opts(), name, monkeypatch)


@pytest.mark.parametrize("kind,name", [("txh", "4096-res"), ("txh", "1024"), ("ah", "2048")])
def test_few_query_pipelines(kind, name, monkeypatch):
    """the small-batch pipeline (three launches and one) and the wide pipeline at 1 and 3 queries: their LDS is
    S kp + dim floats.  Rows bitwise equal to the batched pipeline's, which the scans test checks against the oracle"""
    c = txh_case(name) if kind == "txh" else ah_case(name)
    o = txh_opts() if kind == "txh" else ah_opts()
    H.scan_env(monkeypatch, "default")
    index = hip.txh_create(**c["kw"])
    index.enable_timing(True)
    q = c["q"][:8]
    monkeypatch.setenv("SCANN_HIP_SMALL", "0")
    ref = index.search_batched(q, K, o, stages=True)
    check_staged(kind, c, o, q, K, ref, range(8), "%s %s batched" % (kind, name))
    monkeypatch.delenv("SCANN_HIP_SMALL")

    def same(got, lo, what):
        nq = got[0].shape[0]
        assert np.array_equal(got[2], ref[2][lo:lo + nq]), what + ": counts"
        assert np.array_equal(bits(got[1]), bits(ref[1][lo:lo + nq])), what + ": distances"
        for i in range(nq):
            cn = got[2][i]
            H.assert_topk_equal_up_to_ties(got[0][i, :cn], got[1][i, :cn], ref[0][lo + i, :cn], ref[1][lo + i, :cn], what=what)

    monkeypatch.setenv("SCANN_HIP_WIDE", "0")
    for fused in ("0", "1"):
        monkeypatch.setenv("SCANN_HIP_FUSED", fused)
        for lo, nq in ((0, 1), (2, 3)):
            same(index.search_batched(q[lo:lo + nq], K, o), lo, "small fused=%s q%d+%d" % (fused, lo, nq))
            assert index.last_kernel_ms()[1] == "small_scan_kernel"
    monkeypatch.delenv("SCANN_HIP_FUSED")
    monkeypatch.setenv("SCANN_HIP_WIDE", "2")
    for lo, nq in ((0, 1), (5, 3)):
        same(index.search_batched(q[lo:lo + nq], K, o), lo, "wide q%d+%d" % (lo, nq))
        assert index.last_kernel_ms()[1] == "wide_scan_kernel"
    for lo, nq in ((0, 1), (1, 3)):
        status, di, dd, dc = H.device_search(index, q[lo:lo + nq], K, o)
        assert status == hip.OK, (lo, nq, status)
        same((di, dd, dc), lo, "device q%d+%d" % (lo, nq))


@pytest.mark.parametrize("measure", [L2, L1, COS])
@pytest.mark.parametrize("name", ["768-raw", "1536-raw", "4096-raw"])
def test_tree_ah_mode_with_measured_reorder(name, measure):
    """search_tree_ah: one non-residual table per query, the k best LUT sums re-scored with the configured measure"""
    c = txh_case(name)
    ix, kw = c["ix"], dict(c["kw"])
    kw["distance_measure"] = measure
    index = hip.txh_create(**kw)
    codes_dp = np.empty_like(ix["codes"])
    codes_dp[ix["leaf_ids"]] = ix["codes"]
    o = hip.default_opts()
    o.pre_reorder_k, o.exact_reorder = K, 1
    q = c["q"][:40]
    idx, dist, cnt = index.search_batched(q, K, opts=o)
    for i in range(q.shape[0]):
        oi, od = orc.scann_search_tree_ah(ix["centers"], ix["leaf_off"], ix["leaf_ids"], ix["codebook"], codes_dp,
                                          c["data"], c["stride"], measure, True, q[i], HC.TXH_P, K)
        assert cnt[i] == oi.size
        assert np.array_equal(bits(dist[i, :oi.size]), bits(od)), (name, measure, i)
        assert np.array_equal(idx[i, :oi.size], oi), (name, measure, i)


@pytest.mark.parametrize("name", list(HC.AH_SHAPES))
def test_lut_adc_encode_bit_exact(name):
    """lut_from_query, adc_distances and encode at dsub = 12, 48 and 128"""
    c = ah_case(name)
    ix, S, dim = c["ix"], c["S"], c["dim"]
    index = hip.txh_create(**c["kw"])
    q = c["q"][:5]
    lut = hip.lut_from_query(index, q, S, 16)
    want = np.stack([orc.lut_from_query(ix["codebook"], qq) for qq in q])
    assert np.array_equal(bits(lut.reshape(5, -1)), bits(want.reshape(5, -1))), name
    got = hip.adc_distances(index, want)
    for i in range(5):
        d = np.array([orc.lut_distance(want[i], cd) for cd in ix["codes"]], np.float32)
        assert np.array_equal(bits(got[i]), bits(d)), (name, i)
    rows = c["rows"][:600]
    assert np.array_equal(hip.encode(ix["codebook"], rows), orc.encode_many(ix["codebook"], rows)), name
    centers = synth.uniform_f32(5, dim, 8)
    leaf = (np.arange(600) % 5).astype(np.uint32)
    assert np.array_equal(hip.encode(ix["codebook"], rows, centers=centers, leaf_of_row=leaf),
                          orc.encode_many(ix["codebook"], rows - centers[leaf])), name
    t = txh_case("2048")       # and the residual tables of a tree: dsub 128
    tindex = hip.txh_create(**t["kw"])
    leaves = (np.arange(5) % t["L"]).astype(np.uint32)
    lut = hip.lut_from_query(tindex, t["q"][:5], t["S"], 16, leaf_for_query=leaves)
    for i in range(5):
        res = t["q"][i] - t["ix"]["centers"][leaves[i]]
        assert np.array_equal(bits(lut[i]), bits(orc.lut_from_query(t["ix"]["codebook"], res))), i


def test_tree_per_query_allow_bitmaps():
    """one allow-bitmap per query on the 4096-dim tree, staged outputs against the oracle under each query's bitmap"""
    c = txh_case("4096-res")
    index = hip.txh_create(**c["kw"])
    nq, n, o = 17, c["n"], txh_opts()
    rng = np.random.default_rng(9)
    block = np.stack([H.words_of(np.flatnonzero(rng.random(n) < (0.5 if i % 2 else 0.2)), n)[0] for i in range(nq)])
    q = c["q"][:nq]
    idx, dist, cnt, (tok, tokd, ci, cd, cc) = index.search_batched(q, K, o, stages=True, allow=block, allow_bits=n)
    oix = c["oix"]
    try:
        for i in range(nq):
            oix.allow = block[i]
            assert np.isin(idx[i, :cnt[i]], H.allowed_ids(block[i], n, n)).all()
            H.check_txh_query(oix, q[i], K, idx[i, :cnt[i]], dist[i, :cnt[i]], tok[i], tokd[i], ci[i, :cc[i]],
                              cd[i, :cc[i]], what="per-query allow q%d" % i)
    finally:
        oix.allow = None


# =====================================================================================================================
# 5. tree and hasher indexes over quantized re-rank rows
# =====================================================================================================================
@pytest.fixture(scope="module")
def rerank_bases():
    cache = {}

    def get(dim):
        if dim not in cache:
            cache[dim] = CK.RerankBase(dim, {768: 32, 2048: 16}[dim])
        return cache[dim]

    yield get
    cache.clear()


@pytest.mark.parametrize("fmt", list(FMTS))
@pytest.mark.parametrize("kind", ["txh", "ah"])
@pytest.mark.parametrize("dim", HC.RERANK_DIMS)
def test_quantized_rerank_rows(rerank_bases, dim, kind, fmt):
    """txh_create_quantized: the result rows bitwise against quantized_rerank_model fed with the oracle's merged
    candidates, the device's candidate list against the same list, every distance the quantized brute-force handle's"""
    base = rerank_bases(dim)
    f = FMTS[fmt]
    elems, inv = QC.quantize(base.rows, f)
    for si, stride in enumerate((dim, dim + 5)):
        measure = (SQL2, DOT, L2)[(si + (kind == "ah") + (f == hip.ROWS_INT8)) % 3]
        CK.run_quantized_rerank(base, kind, QC.with_stride(elems, stride, seed=4), f, measure, inv, K, 33, 17,
                                "dim %d %s %s stride %d" % (dim, kind, fmt, stride), stages=(si == 1), bf=(si == 1))


# =====================================================================================================================
# 6. build helpers
# =====================================================================================================================
@pytest.mark.parametrize("dim", HC.BUILD_DIMS)
def test_assign_nearest(dim):
    """bf_assign_nearest with and without distances: 300 rows (two workgroups), 17 centres drawn from the rows with
    duplicates among them (distance 0, ties to the lowest index): two tiles of 16 centres, three of 8 above dim 2560"""
    n, k = 300, 17
    rows = HC.signed_rows(n, dim, 91)
    centers = H.centers_from_rows(rows, k, 92)
    want_tok, want_dist = CK.nearest_reference(rows, centers)
    assert (want_dist == 0).any() and HC.assign_tc(dim) == (16 if dim <= 2560 else 8)
    for stride in (HC.stride_of(dim), dim):
        index = hip.bf_create(HC.strided(rows, stride), n, dim, stride, SQL2)
        CK.check_assign(index, n, centers, want_tok, want_dist, "dim %d stride %d" % (dim, stride))
        index.close()


@pytest.mark.parametrize("dim", HC.BUILD_DIMS)
def test_kmeans_lloyd_and_seeding(dim):
    """kmeans_lloyd on both sides of simd_threshold (the AVX2-order assign with 8 centres per tile, the sequential one
    with 16 or 8) against the oracle; kmeans_init_pp against the seeding reference, in both summation orders"""
    n, k = 300, 5
    rows, _ = synth.clustered_f32(n, dim, 93, n_clusters=k)
    stride = HC.stride_of(dim)
    data = HC.strided(rows, stride)
    index = hip.bf_create(data, n, dim, stride, SQL2)
    init = np.ascontiguousarray(rows[::n // k][:k])
    for thr in (dim, dim + 1):             # sub_dim >= simd_threshold: the AVX2 order; below it: sequential
        CK.check_lloyd(index, data, n, stride, init, thr=thr, max_iterations=2, what="dim %d thr %d" % (dim, thr))
        got = hip.kmeans_init_pp(index, 4, 77, simd_threshold=thr)
        ref = BM.seeding_reference(np.ascontiguousarray(rows), 4, 77, thr, picks=got)
        assert len(ref) == 4
        for c, r in enumerate(ref):
            assert r["rows"].size == 1, "seed %d: band %s" % (c, r["rows"])
            assert np.array_equal(bits(got[c]), bits(rows[r["rows"][0]])), "dim %d thr %d seed %d" % (dim, thr, c)


def test_scalar_quantizer_at_300_by_4096():
    """quantization_stats and scalar_quantize_device over 300 x 4096 rows against the numpy model"""
    import torch
    n, dim = 300, 4096
    rows = (HC.signed_rows(n, dim, 95) * np.float32(3.0)).astype(np.float32)
    stats = SQM.stats_device(rows)
    for stride in (dim, dim + 16):
        index = hip.bf_create(HC.strided(rows, stride), n, dim, stride, SQL2)
        assert np.array_equal(bits(hip.quantization_stats(index)), bits(stats)), stride
    d_rows = torch.from_numpy(HC.strided(rows, dim + 16)).to("cuda:0")
    stream = torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream
    for bits_, mode in ((8, hip.SQ_STDDEV), (4, hip.SQ_SYMMETRIC), (8, hip.SQ_SIGNED)):
        params, _ = SQM.calibrate(stats, bits_, mode, 1.5, 0.0)
        for out_stride in (dim, dim + 3):
            d_out = torch.full((n * out_stride + 64,), 0x5A, dtype=torch.int8, device="cuda:0")
            hip.scalar_quantize_device(d_rows.data_ptr(), n, dim, dim + 16, d_out.data_ptr(), out_stride, params,
                                       bits=bits_, mode=mode, stream=stream)
            torch.cuda.synchronize()
            got = d_out.cpu().numpy()
            assert (got[n * out_stride:] == 0x5A).all(), "guard"
            got = got[:n * out_stride].reshape(n, out_stride)
            assert np.array_equal(got[:, :dim], SQM.quantize(rows, params, bits_, mode)), (bits_, mode, out_stride)
            assert (got[:, dim:] == 0).all(), "pad columns"


# =====================================================================================================================
# 7. mutable indexes
# =====================================================================================================================
def same_as(got, want, k, what):
    idx, dist, cnt = got
    for i, (wi, wd) in enumerate(want):
        c = int(cnt[i])
        assert c == wi.size, "%s q%d: count %d, want %d" % (what, i, c, wi.size)
        assert np.array_equal(bits(dist[i, :c]), bits(wd)), "%s q%d: distances" % (what, i)
        assert np.array_equal(idx[i, :c], wi), "%s q%d: ids\n got %s\nwant %s" % (what, i, idx[i, :c], wi)
        assert np.all(idx[i, c:] == EMPTY) and np.all(np.isposinf(dist[i, c:])), "%s q%d: unused slots" % (what, i)


def up_to_ties(got, want, k, what):
    idx, dist, cnt = got
    for i, (wi, wd) in enumerate(want):
        c = int(cnt[i])
        assert np.all(np.diff(wd) > 0), "the oracle's row has equal adjacent distances"
        assert c == wi.size, "%s q%d: count %d, want %d" % (what, i, c, wi.size)
        H.assert_topk_equal_up_to_ties(idx[i, :c], dist[i, :c], wi, wd, what="%s q%d" % (what, i))


def mutate(mut, model, dim, seed, offset=0.5):
    """add 1080 rows (U[0, 1) - offset) in two batches, remove 27 delta and 30 base ids: the delta spans two tiles of
    1024 rows"""
    new = synth.uniform_f32(1080, dim, seed) - np.float32(offset)
    ids = []
    for part in (new[:700], new[700:]):
        a, b = mut.add(part), model.add(part)
        assert np.array_equal(a, b)
        ids.append(a)
    ids = np.concatenate(ids)
    rm = np.concatenate([ids[3::41], model.base_ids[5::33][:30]])
    mut.remove(rm)
    model.remove(rm)
    assert len(model.delta_ids) > hip.MUTABLE_DELTA_TILE and mut.size() == model.size()


@pytest.mark.parametrize("measure", [SQL2, COS])
@pytest.mark.parametrize("dim", HC.MUTABLE_DIMS)
def test_mutable_brute_force_base(dim, measure):
    """1, 3, 8 and 9 queries: full and partial groups of qt = 8, 7, 4, 3 queries per delta_scan_kernel tile; exact
    ids and bitwise distances against the model; then one fold and the same searches"""
    n = 1000
    rows = synth.uniform_f32(n, dim, 101) - np.float32(0.5)
    data, stride = orc.to_strided(rows)
    base = hip.bf_create(data, n, dim, stride, measure)
    mut, model = hip.Mutable(base, 1100), mm.MutableModel(rows, 1100)
    assert HC.delta_qt(dim) == HC.DELTA_QT[dim]
    mutate(mut, model, dim, 102)
    q = synth.uniform_f32(9, dim, 103) - np.float32(0.5)
    q[1] = model.delta_rows[1000]
    for stage in ("delta", "folded"):
        for nq in (1, 3, 8, 9):
            same_as(mut.search_batched(q[:nq], K), model.search_bf(measure, q[:nq], K), K,
                    "dim %d m%d %s nq %d" % (dim, measure, stage, nq))
        if stage == "delta":
            f = fm.fold(model, dict(kind="bf", measure=measure))
            new_base, base_ids = mut.fold()
            assert np.array_equal(base_ids, f["base_ids"]) and new_base.size() == base_ids.size
            fm.apply(model, f)
            assert mut.pending() == 0 and mut.size() == model.size()
    mut.close()


@pytest.mark.parametrize("dim", HC.MUTABLE_DIMS)
def test_mutable_tree_base(dim):
    """a tree base: the base's filtered answer under the live bitmap merged with the delta scan; the fold assigns and
    encodes the delta rows on the device (assign_nearest_kernel, encode_kernel) and the folded base answers as the
    oracle does on the model's fold.  16 subspaces of 4-bit codes; dim 1540, which no 4-bit subspace count divides, has
    4 subspaces of byte codes (dsub 385) over a codebook taken from the rows"""
    n, L = 1000, 6
    if dim % 16 == 0:
        rows, data, stride, ix, oix, kw = H.make_txh_case(n, dim, L, 16, seed=111, P=HC.TXH_P, mult=HC.TXH_MULT,
                                                          kmeans_iters=2, pq_iters=2)
    else:
        rows = synth.uniform_f32(n, dim, 111)
        pick = np.random.default_rng(111).choice(n, 256, replace=False)
        cb = np.ascontiguousarray(rows[pick].reshape(256, 4, dim // 4).transpose(1, 0, 2), np.float32)
        oix, kw = H.txh_from_codes(rows, cb, trainer.encode(cb, rows, chunk=2048), L, HC.TXH_P, HC.TXH_MULT, seed=111)
        ix = dict(centers=kw["centers"], codebook=cb, leaf_off=kw["leaf_offsets"], leaf_ids=kw["leaf_ids"],
                  codes=kw["codes"])
    base = hip.txh_create(**kw)
    mut, model = hip.Mutable(base, 1100), mm.MutableModel(rows, 1100)
    mutate(mut, model, dim, 112, offset=0.0)       # (rows of the base's distribution: their codes spread like its own)
    q = synth.uniform_f32(9, dim, 113)
    for nq in (1, 3, 8, 9):
        up_to_ties(mut.search_batched(q[:nq], K), model.search_txh(oix, q[:nq], K), K, "dim %d tree nq %d" % (dim, nq))
    fix = dict(kind="txh", centers=ix["centers"], codebook=ix["codebook"], use_residuals=True, leaf_off=ix["leaf_off"],
               leaf_ids=ix["leaf_ids"], codes=ix["codes"])
    f = fm.fold(model, fix)
    new_base, base_ids = mut.fold()
    assert np.array_equal(base_ids, f["base_ids"]) and new_base.size() == base_ids.size
    fm.apply(model, f)
    fdata, fstride = orc.to_strided(f["rows"])
    foix = orc.TxhIndex(fdata, fstride, dim, f["centers"], f["leaf_off"], f["leaf_ids"], f["codebook"], f["codes"],
                        use_residuals=True, partitions_to_search=HC.TXH_P, pre_reorder_multiplier=HC.TXH_MULT)
    # the folded base stage by stage against the oracle on the model's fold (the delta rows now compete as codes: the
    # candidate list may cut a tie of approximate distances), and the mutable handle's rows = the folded base's
    o = txh_opts()
    for nq in (1, 3, 8, 9):
        idx, dist, cnt, (tok, tokd, ci, cd, cc) = new_base.search_batched(q[:nq], K, o, stages=True)
        mi, md, mc = mut.search_batched(q[:nq], K)
        for i in range(nq):
            what = "dim %d folded tree nq %d q%d" % (dim, nq, i)
            H.check_txh_query(foix, q[i], K, idx[i, :cnt[i]], dist[i, :cnt[i]], tok[i], tokd[i], ci[i, :cc[i]],
                              cd[i, :cc[i]], what=what)
            assert mc[i] == cnt[i], what
            H.assert_topk_equal_up_to_ties(mi[i, :cnt[i]], md[i, :cnt[i]], base_ids[idx[i, :cnt[i]].astype(np.int64)],
                                           dist[i, :cnt[i]], what=what + " through the mutable handle")
    mut.close()


# =====================================================================================================================
# 8. MMR and crowding
# =====================================================================================================================
@pytest.mark.parametrize("measure", [SQL2, DOT])
@pytest.mark.parametrize("dim", HC.MMR_DIMS)
def test_mmr(dim, measure):
    """search_mmr (s_row is dimp floats): the model over the handle's own plain row, which is the oracle's"""
    c = BfCase(dim, measure, n=1000, nq=17)
    depth, k, lam = 40, K, 0.5
    for nq in (3, 17):
        plain = c.index.search_batched(c.q[:nq], depth)
        got = c.index.search_mmr(c.q[:nq], k, depth, lam)
        for i in range(nq):
            oi, od = orc.bf_search(c.data, c.n, dim, c.stride, measure, c.q[i], depth)
            pi, pd = plain[0][i, :plain[2][i]], plain[1][i, :plain[2][i]]
            H.assert_topk_equal_up_to_ties(pi, pd, oi, od, what="plain q%d" % i)
            wi, wd = DM.mmr_apply_rows(pi, pd, k, lam, c.data, c.stride, dim, measure)[:2]
            cn = int(got[2][i])
            assert cn == wi.size and np.array_equal(got[0][i, :cn], wi), (dim, measure, nq, i)
            assert np.array_equal(bits(got[1][i, :cn]), bits(wd)), (dim, measure, nq, i)


def test_crowded_search_on_the_2048_dim_tree():
    c = txh_case("2048")
    index = hip.txh_create(**c["kw"])
    attrs = (np.arange(c["n"]) % 7).astype(np.uint64)
    index.set_crowding_attributes(attrs)
    depth, limit = 40, 2
    o = hip.default_opts()
    o.partitions_to_search, o.pre_reorder_k = HC.TXH_P, 3 * depth
    for nq in (3, 17):
        q = c["q"][:nq]
        plain = index.search_batched(q, depth, o)
        got = index.search_crowded(q, K, depth, limit, opts=o)
        for i in range(nq):
            oi, od = orc.txh_search(c["oix"], q[i], depth)      # (pre_reorder_k = 3 depth: the index's multiplier)
            pi, pd = plain[0][i, :plain[2][i]], plain[1][i, :plain[2][i]]
            H.assert_topk_equal_up_to_ties(pi, pd, oi, od, what="plain q%d" % i)
            wi, wd = CM.apply_fast(pi, pd, attrs, limit, K)
            cn = int(got[2][i])
            assert cn == wi.size and np.array_equal(got[0][i, :cn], wi), (nq, i)
            assert np.array_equal(bits(got[1][i, :cn]), bits(wd)), (nq, i)


# =====================================================================================================================
# 9. above the ceiling
# =====================================================================================================================
REFUSALS = (hip.RESOURCE_EXHAUSTED, hip.UNIMPLEMENTED)
OK_ABOVE, REFUSED_ABOVE = "ok", hip.RESOURCE_EXHAUSTED


def outcome(run):
    """"ok" when `run` returns -- it compares its own result with the oracle or a model -- else the refusal's code; a
    launch error, INTERNAL or any other status fails the test"""
    try:
        run()
    except hip.ScannError as e:
        assert e.code in REFUSALS, "refused with %s" % e
        assert "kernel launch:" not in e.message, e.message
        return e.code
    return OK_ABOVE


def one(name, run, want):
    got = outcome(run)
    assert got == want, "%s: %s, the ceilings table says %s" % (name, got, want)


def both(name, run, want):
    """run(nq) at 1 and at 17 queries: the same outcome, the one the ceilings of tests/high_dim_cases.py predict"""
    got = [outcome(lambda: run(1)), outcome(lambda: run(17))]
    assert got[0] == got[1], "%s: %s for 1 query, %s for 17" % (name, got[0], got[1])
    assert got[0] == want, "%s: %s, the ceilings table says %s" % (name, got[0], want)


@pytest.mark.parametrize("measure", [SQL2, L1])
def test_above_the_ceiling_brute_force(measure):
    """dim 6144: every brute-force entry point answers as the oracle does or refuses, the same way for 1 and for 17
    queries and as the ceilings table says; a handle that refused still answers the calls it supports"""
    dim, n, stride = HC.ABOVE, 300, HC.ABOVE
    rows, q = HC.signed_rows(n, dim, 121), HC.signed_rows(17, dim, 122)
    index = hip.bf_create(rows, n, dim, stride, measure)
    top = orc.bf_search_batched(rows, n, dim, stride, measure, q, K)
    f32 = HC.expected_above("bf f32")

    def check_rows(got, nq):
        for i in range(nq):
            assert got[2][i] == K
            H.assert_topk_equal_up_to_ties(got[0][i], got[1][i], top[0][i], top[1][i], what="bf q%d" % i)

    def device(nq):
        status, di, dd, dc = H.device_search(index, q[:nq], K, hip.default_opts())
        if status != hip.OK:
            raise hip.ScannError(status, "device status")
        check_rows((di, dd, dc), nq)

    def distances(nq):
        got = hip.bf_distances(index, q[:nq])
        for i in range(nq):
            assert np.array_equal(bits(got[i]), bits(orc.one_to_many(q[i], rows, stride, n, measure)))

    def radius():
        d = orc.one_to_many(q[0], rows, stride, n, measure)
        r = float(np.sort(d)[25])
        oi, od = orc.bf_search_radius(rows, n, dim, stride, measure, q[0], r)
        gi, gd, found = hip.bf_search_radius(index, q[0], r)
        assert found == oi.size and np.array_equal(bits(gd), bits(od))
        H.assert_topk_equal_up_to_ties(gi, gd, oi, od, what="radius")

    def mmr(nq):
        got = index.search_mmr(q[:nq], 5, 20, 0.5)
        for i in range(nq):
            oi, od = orc.bf_search(rows, n, dim, stride, measure, q[i], 20)
            assert np.all(np.diff(od) > 0), "the oracle's row has equal adjacent distances"
            wi, wd = DM.mmr_apply_rows(oi, od, 5, 0.5, rows, stride, dim, measure)[:2]
            cn = int(got[2][i])
            assert cn == wi.size and np.array_equal(got[0][i, :cn], wi) and np.array_equal(bits(got[1][i, :cn]), bits(wd))

    both("host", lambda nq: check_rows(index.search_batched(q[:nq], K), nq), f32)
    both("device", device, f32)
    both("bf_distances", distances, f32)
    one("bf_search_radius", radius, f32)
    both("search_mmr", mmr, f32)
    mut, model = hip.Mutable(index, 64), mm.MutableModel(rows, 64)
    new = HC.signed_rows(40, dim, 123)
    assert np.array_equal(mut.add(new), model.add(new))
    both("mutable", lambda nq: same_as(mut.search_batched(q[:nq], K), model.search_bf(measure, q[:nq], K), K, "mutable"), f32)
    mut.close()
    # the handle still answers what it supports: the seeding stages no centres
    got = hip.kmeans_init_pp(index, 3, 5)
    ref = BM.seeding_reference(rows, 3, 5, picks=got)
    assert len(ref) == 3 and all(r["rows"].size == 1 and np.array_equal(bits(got[c]), bits(rows[r["rows"][0]]))
                                 for c, r in enumerate(ref))
    if measure == SQL2:      # (the quantizer takes SquaredL2, L2 and DotProduct handles)
        assert np.array_equal(bits(hip.quantization_stats(index)), bits(SQM.stats_device(rows)))
        quant = HC.expected_above("bf quantized")
        qi, _ = index.quantize_rows(hip.ROWS_INT8)
        codes, params, _ = SQM.rows_int8(rows, stride, 8, hip.SQ_SIGNED, 0.0, 0.0)
        b16 = qc.bf16_from_f32(rows)
        qb = hip.bf_create_quantized(b16, n, dim, stride, hip.ROWS_BF16, measure, 1.0)
        for name, handle, want in (("int8", qi, qc.distances(q, codes, dim, qc.ROWS_INT8, measure, float(params[2]))),
                                   ("bf16", qb, qc.distances(q, b16, dim, qc.ROWS_BF16, measure, 1.0))):
            def qdist(nq):
                assert np.array_equal(bits(hip.bf_distances(handle, q[:nq])), bits(want[:nq]))

            def qsearch(nq):
                idx, dist, cnt = handle.search_batched(q[:nq], K)
                for i in range(nq):
                    assert_quantized_topk(idx[i], dist[i], cnt[i], want[i], K, "%s q%d" % (name, i))

            both("quantized bf_distances " + name, qdist, quant)
            both("quantized search " + name, qsearch, quant)
            handle.close()

        def quantize_device():
            import torch
            st = SQM.stats_device(rows)
            p8, _ = SQM.calibrate(st, 8, hip.SQ_STDDEV, 1.5, 0.0)
            d_rows = torch.from_numpy(rows).to("cuda:0")
            d_out = torch.full((n * dim + 64,), 0x5A, dtype=torch.int8, device="cuda:0")
            hip.scalar_quantize_device(d_rows.data_ptr(), n, dim, stride, d_out.data_ptr(), dim, p8, bits=8,
                                       mode=hip.SQ_STDDEV, stream=torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)
            torch.cuda.synchronize()
            got = d_out.cpu().numpy()
            assert (got[n * dim:] == 0x5A).all()
            assert np.array_equal(got[:n * dim].reshape(n, dim), SQM.quantize(rows, p8, 8, hip.SQ_STDDEV))

        one("scalar_quantize_device", quantize_device, OK_ABOVE)
    index.close()


def test_above_the_ceiling_trees_and_hashers():
    """dim 6144 (16 subspaces of 384 dims): Partitioned mode refuses at every batch size, the partitioner, the tree, the
    flat hasher, the measured re-rank, crowding, quantized re-rank rows, the tables and a tree-based mutable index
    answer as the oracle does"""
    dim, n, L = HC.ABOVE, 600, 4
    q17 = HC.signed_rows(17, dim, 122)
    # ---- Partitioned mode and the partitioner
    prow, pdata, pstride, centers, leaf_off, leaf_ids = partition_case(300, dim, L, 123)
    pindex = hip.txh_create(data=pdata, n_rows=300, dim=dim, stride=pstride, centers=centers, leaf_offsets=leaf_off,
                            leaf_ids=leaf_ids, codebook=None, codes=None, partitions_to_search=3)

    def partitioned(nq):
        got = pindex.search_batched(q17[:nq], K)
        for i in range(nq):
            oi, od = orc.scann_search_partitioned(centers, leaf_off, leaf_ids, pdata, pstride, SQL2, q17[i], 3, K)
            assert got[2][i] == oi.size and np.array_equal(got[0][i, :oi.size], oi)
            assert np.array_equal(bits(got[1][i, :oi.size]), bits(od))

    def tokens(nq):
        tok, dist, cnt = hip.txh_partition(pindex, q17[:nq], 3)
        for i in range(nq):
            ot, od = orc.partition(centers, q17[i], 3)
            assert np.array_equal(tok[i, :ot.size], ot) and np.array_equal(bits(dist[i, :ot.size]), bits(od))

    both("partitioned", partitioned, HC.expected_above("partitioned", "centroid scores"))
    both("txh_partition", tokens, HC.expected_above("centroid scores"))       # (after the refusal: the handle answers)
    pindex.close()
    # ---- one codebook, a tree view and a flat-hasher view over it
    base = CK.RerankBase(dim, 16, n=n, nq=17, leaves=L)
    data, stride = orc.to_strided(base.rows)
    q, oix = base.q, base.oix
    tree = HC.expected_above("tree / hasher, batched", "centroid scores")
    tindex = hip.txh_create(data=data, stride=stride, **base.txh_kw)

    def tree_search(nq):
        got = tindex.search_batched(q[:nq], K)
        for i in range(nq):
            oi, od = orc.txh_search(oix, q[i], K)
            assert got[2][i] == oi.size
            H.assert_topk_equal_up_to_ties(got[0][i, :oi.size], got[1][i, :oi.size], oi, od, what="tree q%d" % i)

    both("tree", tree_search, tree)
    attrs = (np.arange(n) % 7).astype(np.uint64)
    tindex.set_crowding_attributes(attrs)
    depth = 20
    o = hip.default_opts()
    o.partitions_to_search, o.pre_reorder_k = base.p, 3 * depth

    def crowded(nq):
        got = tindex.search_crowded(q[:nq], K, depth, 2, opts=o)
        for i in range(nq):
            oi, od = orc.txh_search(oix, q[i], depth)
            assert np.all(np.diff(od) > 0), "the oracle's row has equal adjacent distances"
            wi, wd = CM.apply_fast(oi, od, attrs, 2, K)
            cn = int(got[2][i])
            assert cn == wi.size and np.array_equal(got[0][i, :cn], wi) and np.array_equal(bits(got[1][i, :cn]), bits(wd))

    both("search_crowded", crowded, tree)
    mut, model = hip.Mutable(tindex, 64), mm.MutableModel(base.rows, 64)
    new = synth.uniform_f32(40, dim, 124)
    assert np.array_equal(mut.add(new), model.add(new))
    mutable = lambda nq: up_to_ties(mut.search_batched(q[:nq], K), model.search_txh(oix, q[:nq], K), K, "mutable tree")
    both("mutable tree", mutable, tree)
    one("fold", mut.fold, HC.expected_above("assign nearest"))     # (the delta's assignment stages 8 centres)
    both("mutable tree after the refused fold", mutable, tree)
    mut.close()
    tindex.close()
    o = hip.default_opts()
    o.pre_reorder_k, o.exact_reorder = K, 1
    mindex = hip.txh_create(data=data, stride=stride, **dict(base.txh_kw, distance_measure=L1))

    def tree_ah(nq):
        idx, dist, cnt = mindex.search_batched(q[:nq], K, opts=o)
        for i in range(nq):
            oi, od = orc.scann_search_tree_ah(oix.centers, oix.leaf_off, oix.leaf_ids, base.cb, base.codes, data, stride,
                                              L1, True, q[i], base.p, K)
            assert cnt[i] == oi.size and np.array_equal(bits(dist[i, :oi.size]), bits(od))
            assert np.array_equal(idx[i, :oi.size], oi)

    both("tree-AH, L1 re-rank", tree_ah, tree)
    luts = np.stack([orc.lut_from_query(base.cb, qq) for qq in q])

    def lut(nq):
        got = hip.lut_from_query(mindex, q[:nq], 16, 16)
        assert np.array_equal(bits(got.reshape(nq, -1)), bits(luts[:nq].reshape(nq, -1)))

    both("lut_from_query", lut, HC.expected_above("lut_from_query"))
    mindex.close()
    aindex = hip.txh_create(**H.ah_kwargs_from_codes(base.rows, base.cb, base.codes))

    def hasher(nq):
        got = aindex.search_batched(q[:nq], K, base.opts("ah", 40))
        for i in range(nq):
            oi, od = orc.ah_search_with_reordering(base.cb, base.codes, data, stride, q[i], K, 40)
            assert got[2][i] == oi.size
            H.assert_topk_equal_up_to_ties(got[0][i, :oi.size], got[1][i, :oi.size], oi, od, what="hasher q%d" % i)

    def adc(nq):
        got = hip.adc_distances(aindex, luts[:nq])
        for i in range(min(nq, 3)):
            want = np.array([orc.lut_distance(luts[i], cd) for cd in base.codes], np.float32)
            assert np.array_equal(bits(got[i]), bits(want))

    both("flat hasher", hasher, tree)
    both("adc_distances", adc, OK_ABOVE)
    aindex.close()
    one("encode", lambda: np.testing.assert_array_equal(hip.encode(base.cb, base.rows[:100]),
                                                        orc.encode_many(base.cb, base.rows[:100])), OK_ABOVE)
    # ---- quantized re-rank rows: every batch size takes the staged pipeline
    for kind, fmt in (("txh", hip.ROWS_BF16), ("ah", hip.ROWS_INT8)):
        elems, inv = QC.quantize(base.rows, fmt)
        rows_q = QC.with_stride(elems, dim + 5, seed=4)
        both("quantized re-rank rows " + kind,
             lambda nq: CK.run_quantized_rerank(base, kind, rows_q, fmt, SQL2, inv, K, 33, nq, "%s nq %d" % (kind, nq)), tree)


def test_above_the_ceiling_build_helpers():
    """dim 6144: the assignment kernels stage at least 8 centres and refuse; the seeding stages none"""
    dim, n = HC.ABOVE, 300
    rows = HC.signed_rows(n, dim, 121)
    index = hip.bf_create(rows, n, dim, dim, SQL2)
    cen = H.centers_from_rows(rows, 5, 126)
    want_tok, want_dist = CK.nearest_reference(rows, cen)
    one("bf_assign_nearest", lambda: CK.check_assign(index, n, cen, want_tok, want_dist, "dim %d" % dim),
        HC.expected_above("assign nearest"))
    for thr, row in ((dim, "k-means assign, AVX2 order"), (dim + 1, "assign nearest")):
        one("kmeans_lloyd thr %d" % thr, lambda: CK.check_lloyd(index, rows, n, dim, cen, thr=thr, max_iterations=1),
            HC.expected_above(row))
        got = hip.kmeans_init_pp(index, 3, 5, simd_threshold=thr)          # after the refusal
        ref = BM.seeding_reference(rows, 3, 5, thr, picks=got)
        assert len(ref) == 3 and all(r["rows"].size == 1 and np.array_equal(bits(got[c]), bits(rows[r["rows"][0]]))
                                     for c, r in enumerate(ref))
    index.close()

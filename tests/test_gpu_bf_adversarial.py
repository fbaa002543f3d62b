"""Brute-force kernels on signed, extreme-scale and tie-heavy data (tests/helpers.py adversarial_rows).

Every f32 brute-force path and every quantized one is crossed with the data families, and each case is checked
against an exact oracle: the whole bf_distances matrix bitwise (orc.one_to_many / qc.distances), top-k bitwise up
to distance ties (orc.bf_search_batched / the checker's TopK), and, where the bf16 shortlist ran, bitwise against
bf_exact = 1 plus the device entry's "Ok with the oracle's rows, or Aborted" promise.  Each kernel-specific case
asserts the kernel the library reports (index.last_kernel_ms()[1]); `pass_kernel` mirrors bf.hip's choice.

Non-finite inputs (NaN / inf in rows or queries) are out of scope: the reference's TopK stops replacing its heap
top once a NaN reaches it, and the library has no policy for them yet."""
import numpy as np
import pytest

from oracle import pyoracle as orc
from scann_rust_amd import hip
from tests import helpers as H
from tests import quantized_checker as qc
from tests.test_gpu_quantized_bf import _device_search, assert_topk, same

pytestmark = pytest.mark.gpu

SQL2, L2, DOT, L1, COS = hip.SQUARED_L2, hip.L2, hip.DOT_PRODUCT, hip.L1, hip.COSINE
FAMILIES = list(H.ADVERSARIAL_FAMILIES)
FMTS = [hip.ROWS_BF16, hip.ROWS_FP8_E4M3, hip.ROWS_INT8]
MAX_K = 2048            # kBfMaxK
N_BIG = 20013           # > 8192 (the filter bound samples every 2nd row), not a multiple of 32
N_MID = 10007           # > 8192, one sample per row


def family_n(family, n):
    """sample-adversarial needs a real sample stride (rs >= 2)"""
    return N_BIG if family == "sample-adversarial" else n


def pass_kernel(measure, dim, stride, nq):
    """bf.hip launch_pass / bf_pass_kernel_name for f32 rows (device rows are 16-byte aligned)"""
    aligned = stride % 4 == 0
    if measure in (SQL2, L2, DOT) and aligned and dim >= 8 and nq <= 16:
        return "bf_stream_kernel"
    if measure == DOT and aligned and dim in (32, 64, 96, 128, 192, 256):
        return "bf_mfma_dot_kernel"
    if measure in (SQL2, L2) and aligned and dim in (32, 64, 96, 128) and nq >= 128:
        return "bf_vq_kernel"
    return "bf_generic_kernel"


def norms_finite(x):
    """the largest squared row norm of the (decoded) rows is finite: the overflow family's is not"""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        return bool(np.isfinite(np.max(np.sum(x * x, axis=1, dtype=np.float32))))


def shortlist_taken(k, n, finite):
    """bf.hip bf_shortlist_eligible under the force_shortlist knobs: 4k <= 256, a shortlist of at most n / 8 rows,
    and a finite largest row norm."""
    return finite and 4 * k <= 256 and max(32, 4 * k) * 8 <= n


def strided(rows, stride):
    out = np.zeros((rows.shape[0], stride), np.float32)
    out[:, :rows.shape[1]] = rows
    return out


@pytest.fixture
def no_small(monkeypatch):
    monkeypatch.setenv("SCANN_HIP_SMALL", "0")


@pytest.fixture
def force_shortlist(monkeypatch):
    monkeypatch.setenv("SCANN_HIP_BF_SHORTLIST_MIN_ROWS", "1")
    monkeypatch.setenv("SCANN_HIP_BF_SHORTLIST_MIN_QUERIES", "1")
    monkeypatch.setenv("SCANN_HIP_SMALL", "0")


class F32Case:
    """One f32 index of a family with its oracle view."""

    def __init__(self, family, measure, n, dim, stride, nq, seed):
        self.family, self.measure, self.n, self.dim, self.stride = family, measure, n, dim, stride
        self.rows = H.adversarial_rows(family, n, dim, seed)
        self.q = H.adversarial_queries(family, nq, dim, seed + 1, self.rows)
        self.data = strided(self.rows, stride)
        self.index = hip.bf_create(self.data, n, dim, stride, measure)
        self.index.enable_timing(True)
        self.finite = norms_finite(self.rows)
        self._topk = None

    def what(self, **kw):
        return "%s m%d n%d dim%d stride%d %s" % (self.family, self.measure, self.n, self.dim, self.stride,
                                                 " ".join("%s%s" % kv for kv in kw.items()))

    def check_distances(self, nq, kernel=None):
        """the whole [nq][n] matrix, bitwise; the kernel is the one a search of nq queries reports"""
        q = self.q[:nq]
        got = hip.bf_distances(self.index, q)
        for i in range(nq):
            want = orc.one_to_many(q[i], self.data, self.stride, self.n, self.measure)
            assert same(got[i], want), self.what(nq=nq, q=i, dist="")
        if kernel:
            o = hip.default_opts()
            o.bf_exact = 1
            self.index.search_batched(q, 1, opts=o)
            assert self.index.last_kernel_ms()[1] == kernel, self.what(nq=nq)

    def oracle(self):
        """top-min(n, 2048) of every query; smaller k compare against prefixes (up to ties)"""
        if self._topk is None:
            self._topk = orc.bf_search_batched(self.data, self.n, self.dim, self.stride, self.measure, self.q,
                                               min(self.n, MAX_K))
        return self._topk

    def assert_rows(self, idx, dist, cnt, nq, k, what):
        oi, od, oc = self.oracle()
        m = min(k, self.n)
        for i in range(nq):
            assert cnt[i] == m, "%s q%d count %d" % (what, i, cnt[i])
            H.assert_topk_equal_up_to_ties(idx[i, :m], dist[i, :m], oi[i, :m], od[i, :m], what="%s q%d" % (what, i))

    def check_search(self, nq, ks, kernel=None, shortlist=False):
        q = self.q[:nq]
        for k in ks:
            what = self.what(nq=nq, k=k)
            if min(k, self.n) > MAX_K:
                with pytest.raises(hip.ScannError) as e:
                    self.index.search_batched(q, k)
                assert e.value.code == hip.UNIMPLEMENTED, what
                continue
            idx, dist, cnt = self.index.search_batched(q, k)
            took = shortlist and shortlist_taken(k, self.n, self.finite)
            if took:
                assert self.index.last_kernel_ms()[1] == "bf_bf16_kernel", what
            elif kernel:
                assert self.index.last_kernel_ms()[1] == kernel, what
            self.assert_rows(idx, dist, cnt, nq, k, what)
            if took:
                check_shortlist_against_exact(self.index, q, k, idx, dist, cnt, what)


def check_shortlist_against_exact(index, q, k, idx, dist, cnt, what):
    """The shortlist ran: the host result equals bf_exact = 1 bit for bit, and the device entry returns Ok with
    those rows or Aborted -- never Ok with other rows."""
    o = hip.default_opts()
    o.bf_exact = 1
    idx2, dist2, cnt2 = index.search_batched(q, k, opts=o)
    assert np.array_equal(cnt, cnt2) and np.array_equal(idx, idx2) and same(dist, dist2), what + " vs bf_exact"
    if k > index.size():
        return
    st, di, dd, dc = _device_search(index, q, k, exact=False)
    assert st in (hip.OK, 10), "%s device status %d" % (what, st)
    if st == hip.OK:
        assert np.array_equal(dc, cnt) and np.array_equal(di, idx) and same(dd, dist), what + " device rows"


# ---- f32 rows, one test per path --------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("measure", [SQL2, L2, DOT, L1, COS])
def test_small_batch_pipeline(family, measure):
    """The tree code's small-batch exact pipeline (bf_small_search_host) reports no kernel; it is pinned by its
    conditions: default knobs, nq <= 16, k <= 64, n <= 262144.  n = 50 reaches k = n + 7."""
    for n in (family_n(family, N_MID), 50):
        if family == "sample-adversarial" and n == 50:
            continue
        c = F32Case(family, measure, n, 40, 48, 16, 11)
        for nq in (1, 16):
            c.check_search(nq, [1, 10, 64] + ([n + 7] if n + 7 <= 64 else []))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("measure", [SQL2, L2, DOT])
def test_stream_kernel(no_small, family, measure):
    for dim, stride in ((8, 8), (50, 64), (128, 128)):
        c = F32Case(family, measure, family_n(family, N_MID), dim, stride, 16, 12)
        c.check_distances(16, "bf_stream_kernel")
        for nq in (1, 9, 16):
            c.check_search(nq, [1, 10, MAX_K, c.n + 7], kernel="bf_stream_kernel")


@pytest.mark.parametrize("family", FAMILIES)
def test_mfma_dot_kernel(family):
    for dim in (32, 64, 96, 128, 192, 256):
        c = F32Case(family, DOT, family_n(family, N_MID), dim, dim, 300, 13 + dim)
        c.check_distances(300, "bf_mfma_dot_kernel")
        for nq in (17, 300):
            c.check_search(nq, [1, 10, MAX_K], kernel="bf_mfma_dot_kernel")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("measure", [SQL2, L2])
def test_vq_kernel(family, measure):
    for dim in (32, 64, 96, 128):
        c = F32Case(family, measure, family_n(family, N_MID), dim, dim, 129, 14 + dim)
        for nq in (128, 129):
            c.check_distances(nq, "bf_vq_kernel")
            c.check_search(nq, [1, 10, MAX_K], kernel="bf_vq_kernel")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("measure", [SQL2, L2, DOT, L1, COS])
def test_generic_kernel(no_small, family, measure):
    """stride == dim (not a multiple of 4) for dims 50 and 33, dim < 8, and every layout for L1 / Cosine"""
    shapes = ((50, 50), (33, 33), (5, 5), (5, 16)) + (((128, 128),) if measure in (L1, COS) else ())
    for dim, stride in shapes:
        n = family_n(family, 3001 if measure in (L1, COS) else N_MID)
        c = F32Case(family, measure, n, dim, stride, 40, 15 + dim)
        assert pass_kernel(measure, dim, stride, 40) == "bf_generic_kernel"
        c.check_distances(5 if measure in (L1, COS) else 40, "bf_generic_kernel")
        for nq in (5, 40):
            c.check_search(nq, [1, 10, MAX_K, c.n + 7], kernel="bf_generic_kernel")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("measure", [SQL2, L2, DOT])
def test_f32_shortlist(force_shortlist, family, measure):
    """bf16 shortlist for k <= 64 (asserted by kernel), the exact kernels above it; n % 32 != 0"""
    for dim in (32, 96, 192, 256):
        c = F32Case(family, measure, N_BIG, dim, dim, 129, 16 + dim)
        for nq in (1, 127, 129):
            c.check_search(nq, [1, 10, 64, MAX_K, c.n + 7], kernel=pass_kernel(measure, dim, dim, nq),
                           shortlist=True)


def test_f32_shortlist_split_ties(force_shortlist):
    """Exact ties whose split-bf16 scores differ by 2^-14 |q|^2 / 32 (helpers.bf16_split_ties): far inside the
    error bound, so no query may be accepted -- the shortlist holds none of the tie's smallest indices."""
    n, dim = 6007, 32
    rows, q = H.bf16_split_ties(n, dim, 1)
    index = hip.bf_create(rows, n, dim, dim, DOT)
    index.enable_timing(True)
    for k in (1, 10):
        idx, dist, cnt = index.search_batched(q, k)
        assert index.last_kernel_ms()[1] == "bf_bf16_kernel"
        oi, od, oc = orc.bf_search_batched(rows, n, dim, dim, DOT, q, k)
        for i in range(q.shape[0]):
            assert cnt[i] == k
            H.assert_topk_equal_up_to_ties(idx[i], dist[i], oi[i], od[i], what="k%d q%d" % (k, i))
            assert sorted(idx[i].tolist()) == list(range(k)), (k, i, idx[i])   # the tie's smallest indices
        st, di, dd, dc = _device_search(index, q, k, exact=False)
        assert st == 10, st   # Aborted: the bound cannot separate the tie from the shortlist's edge


# ---- overflow of the candidate buffer ---------------------------------------------------------------------
@pytest.mark.parametrize("measure", [SQL2, L2, DOT])
def test_sample_adversarial_overflow(no_small, measure):
    """Every non-sampled row passes the filter bound, far more than the candidate buffer holds: the host entry
    returns the oracle's rows after its full-buffer retry; the device entry reports ResourceExhausted and no row
    it returns differs from the oracle's."""
    for dim, nq in ((64, 1), (64, 17), (96, 129), (33, 20)):
        stride = dim if dim % 4 else dim + 4
        c = F32Case("sample-adversarial", measure, N_BIG, dim, stride, nq, 17)
        c.check_search(nq, [1, 10, MAX_K], kernel=pass_kernel(measure, dim, stride, nq))
        for k in (10, 300):
            st, di, dd, dc = _device_search(c.index, c.q, k, exact=True)
            assert st == hip.RESOURCE_EXHAUSTED, (dim, nq, k, st)
            oi, od, oc = c.oracle()
            for i in range(nq):
                if dc[i]:
                    assert dc[i] == k
                    H.assert_topk_equal_up_to_ties(di[i], dd[i], oi[i, :k], od[i, :k], what="device q%d" % i)


def test_sample_adversarial_overflow_shortlist(force_shortlist):
    """The same overflow behind the shortlist's own filter: host rows equal the oracle's; the device entry does not
    return Ok."""
    for measure in (SQL2, DOT):
        c = F32Case("sample-adversarial", measure, N_BIG, 64, 64, 40, 18)
        idx, dist, cnt = c.index.search_batched(c.q, 10)
        assert c.index.last_kernel_ms()[1] == "bf_bf16_kernel"
        c.assert_rows(idx, dist, cnt, 40, 10, "shortlist overflow m%d" % measure)
        st, di, dd, dc = _device_search(c.index, c.q, 10, exact=False)
        assert st in (hip.RESOURCE_EXHAUSTED, 10), st


# ---- radius -----------------------------------------------------------------------------------------------
def _ordered(d):
    b = np.asarray(d, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))   # common.h f32_to_ordered


@pytest.mark.parametrize("measure", [DOT, SQL2, L2])
@pytest.mark.parametrize("dim,stride", [(40, 48), (37, 37)])
def test_radius_signed(measure, dim, stride):
    """bf_search_radius on signed data, radius at an exact distance of the matrix; rows 100..103 copy the
    boundary row so the boundary ties.  DotProduct with a negative and a positive radius."""
    n = 5013
    rows = H.adversarial_rows("signed", n, dim, 19)
    q = H.adversarial_queries("signed", 1, dim, 20, rows)[0]
    d0 = orc.one_to_many(q, rows, dim, n, measure)
    order0 = np.argsort(d0, kind="stable")
    picks = [order0[300], order0[n // 2 + 400]] if measure == DOT else [order0[300]]
    for p in picks:
        r = rows.copy()
        r[100:104] = r[p]
        data = strided(r, stride)
        index = hip.bf_create(data, n, dim, stride, measure)
        d = orc.one_to_many(q, data, stride, n, measure)
        radius = float(d[p])
        if measure == DOT:
            assert (radius < 0) == (p == picks[0]), radius
        sel = np.nonzero(_ordered(d) <= _ordered(np.float32(radius)))[0]
        order = sel[np.lexsort((sel, _ordered(d[sel])))]
        assert np.isin(np.arange(100, 104), order).all()
        ri, rd, rc = hip.bf_search_radius(index, q, radius)
        assert rc == order.size and np.array_equal(ri, order) and same(rd, d[order]), (measure, radius)
        ci, cd, cc = hip.bf_search_radius(index, q, radius, capacity=10)
        assert cc == order.size and np.array_equal(ci, order[:10]) and same(cd, d[order[:10]])


# ---- batch isolation --------------------------------------------------------------------------------------
@pytest.mark.parametrize("measure", [SQL2, L2, DOT])
@pytest.mark.parametrize("path", ["small", "stream", "wide", "shortlist"])
def test_batch_isolation(monkeypatch, measure, path):
    """A zero query, a 2^56 query and a duplicate-row query in one batch: each gets the rows it gets alone."""
    if path != "small":
        monkeypatch.setenv("SCANN_HIP_SMALL", "0")
    if path == "shortlist":
        monkeypatch.setenv("SCANN_HIP_BF_SHORTLIST_MIN_ROWS", "1")
        monkeypatch.setenv("SCANN_HIP_BF_SHORTLIST_MIN_QUERIES", "1")
    n, dim, k = N_BIG, 64, 10
    rows = H.adversarial_rows("duplicates", n, dim, 21)
    rows[H.zero_rows(n)] = 0.0
    rows[10:15] *= np.float32(2.0 ** 20)
    nq = {"small": 3, "stream": 16, "wide": 129, "shortlist": 129}[path]
    q = H.adversarial_queries("signed", nq, dim, 22, rows)
    q[0] = 0.0
    q[1] *= np.float32(2.0 ** 56)
    q[2] = rows[H.duplicate_protos(n)[1]]
    index = hip.bf_create(rows, n, dim, dim, measure)
    index.enable_timing(True)
    idx, dist, cnt = index.search_batched(q, k)
    if path == "shortlist":
        assert index.last_kernel_ms()[1] == "bf_bf16_kernel"
    elif path != "small":
        assert index.last_kernel_ms()[1] == pass_kernel(measure, dim, dim, nq)
    oi, od, oc = orc.bf_search_batched(rows, n, dim, dim, measure, q[:3], k)
    for i in range(3):
        ai, ad, ac = index.search_batched(q[i:i + 1], k)
        assert cnt[i] == ac[0] == k
        assert np.array_equal(idx[i], ai[0]) and same(dist[i], ad[0]), (path, i)
        H.assert_topk_equal_up_to_ties(idx[i], dist[i], oi[i], od[i], what="%s q%d" % (path, i))


# ---- quantized rows ---------------------------------------------------------------------------------------
def quantize(family_rows, fmt):
    """(codes, inv_multiplier): bf16 bits, E4M3 codes at a scale mapping the family's largest |x| to 448, or
    symmetric int8"""
    x = family_rows
    if fmt == hip.ROWS_BF16:
        return qc.bf16_from_f32(x), 1.0
    if fmt == hip.ROWS_FP8_E4M3:
        m = float(np.max(np.abs(x)))
        return orc.fp8_quantize(x, float(np.float32(448.0 / m)) if m > 0 else 1.0), 1.0
    return hip.symmetric_int8(x)


def strided_codes(codes, stride):
    out = np.zeros((codes.shape[0], stride), codes.dtype)
    out[:, :codes.shape[1]] = codes
    return out


class QuantCase:
    def __init__(self, codes, inv, fmt, measure, dim, stride, q, what):
        self.fmt, self.measure, self.dim, self.inv, self.what = fmt, measure, dim, inv, what
        self.n = codes.shape[0]
        self.rows = strided_codes(codes, stride)
        self.q = q
        self.index = hip.bf_create_quantized(self.rows, self.n, dim, stride, fmt, measure, inv)
        self.index.enable_timing(True)
        self.finite = norms_finite(qc.decode(codes, fmt, inv))
        self._d = None

    def dmat(self, nq):
        if self._d is None or self._d.shape[0] < nq:
            self._d = qc.distances(self.q[:nq], self.rows, self.dim, self.fmt, self.measure, self.inv)
        return self._d[:nq]

    def check_distances(self, nq):
        got = hip.bf_distances(self.index, self.q[:nq])
        assert same(got, self.dmat(nq)), self.what + " distances"

    def check_search(self, nq, ks, kernel, shortlist=False, check_q=None):
        q = self.q[:nq]
        check_q = nq if check_q is None else check_q
        for k in ks:
            what = "%s nq%d k%d" % (self.what, nq, k)
            if min(k, self.n) > MAX_K:
                with pytest.raises(hip.ScannError) as e:
                    self.index.search_batched(q, k)
                assert e.value.code == hip.UNIMPLEMENTED, what
                continue
            idx, dist, cnt = self.index.search_batched(q, k)
            took = shortlist and shortlist_taken(k, self.n, self.finite)
            assert self.index.last_kernel_ms()[1] == ("bf_bf16_kernel" if took else kernel), what
            d = self.dmat(check_q)
            for i in range(check_q):
                assert_quant_topk(idx[i], dist[i], cnt[i], d[i], k, what="%s q%d" % (what, i))
            if took:
                check_shortlist_against_exact(self.index, q, k, idx, dist, cnt, what)


def assert_quant_topk(idx, dist, cnt, d, k, what):
    """assert_topk (test_gpu_quantized_bf).  Where the result reaches distance 0 and the row holds zeros of both
    signs (int8 products that underflow), the reference's TopK sees one tie of -0.0 and +0.0 and may keep and
    list either sign, so its sequence is compared as floats; the indices must still be exactly the first
    min(k, n) by the library's (distance, index) key (-0.0 before +0.0), and the distances bitwise the
    checker's at those indices."""
    c = int(cnt)
    d = np.asarray(d, np.float32)
    order = np.lexsort((np.arange(d.size), _ordered(d)))[:min(k, d.size)]
    top = d[order]
    zeros = d[d == 0]
    if not ((top == 0).any() and np.signbit(zeros).any() and (~np.signbit(zeros)).any()):
        assert_topk(idx, dist, cnt, d, k, what=what)
        return
    oi, od = orc.topk_run(min(k, d.size), np.arange(d.size, dtype=np.uint32), d)
    assert c == order.size == oi.size, what
    assert np.array_equal(np.asarray(idx[:c], np.int64), order), what
    assert same(dist[:c], top), what
    assert np.array_equal(top, od), what   # float comparison: -0.0 == +0.0


def quant_family_case(family, fmt, measure, n, dim, stride, nq, seed):
    n = family_n(family, n)
    x = H.adversarial_rows(family, n, dim, seed)
    codes, inv = quantize(x, fmt)
    q = H.adversarial_queries(family, nq, dim, seed + 1, x)
    return QuantCase(codes, inv, fmt, measure, dim, stride, q, "%s fmt%d m%d dim%d stride%d" %
                     (family, fmt, measure, dim, stride))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("measure", [SQL2, L2, DOT])
def test_quant_kernel(family, fmt, measure):
    for dim, stride in ((40, 40), (96, 101)):
        c = quant_family_case(family, fmt, measure, 2013, dim, stride, 31, 23 + dim)
        c.check_distances(31)
        for nq in (1, 31):
            c.check_search(nq, [1, 10, MAX_K, c.n + 7], "bf_quant_kernel", check_q=min(nq, 8))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("measure", [SQL2, L2, DOT])
def test_quant_shortlist(force_shortlist, family, fmt, measure):
    """bf_bf16_kernel<FMT> over every shortlist dim, stride = dim and dim + 8, n % 32 != 0 (a partial last tile)"""
    for dim, stride in ((32, 32), (32, 40), (64, 72), (96, 96), (192, 200), (256, 256)):
        c = quant_family_case(family, fmt, measure, 8013, dim, stride, 40, 24 + dim)
        c.check_search(40, [1, 10, 64, MAX_K], "bf_quant_kernel", shortlist=True, check_q=6)


INT8_SCALES = [(-140, 0), (-140, -20), (-100, -20), (-100, -70), (-20, 20), (20, -20), (20, 56)]


@pytest.mark.parametrize("inv_exp,q_exp", INT8_SCALES)
@pytest.mark.parametrize("measure", [SQL2, L2, DOT])
def test_int8_extreme_multipliers(monkeypatch, inv_exp, q_exp, measure):
    """int8 rows with inv_multiplier 2^-140 ... 2^20 and queries signed x 2^q_exp: at the low end the decoded
    values and the products are subnormal.  bf_quant_kernel (5 queries), then the shortlist (40 queries)."""
    n, inv = 8013, float(2.0 ** inv_exp)
    for dim, stride in ((64, 64), (96, 104)):
        rng = np.random.default_rng([inv_exp + 200, q_exp + 200, dim])
        codes = rng.integers(-127, 128, (n, dim)).astype(np.int8)
        q = (rng.uniform(-1, 1, (40, dim)) * 2.0 ** q_exp).astype(np.float32)
        what = "int8 inv2^%d q2^%d m%d dim%d" % (inv_exp, q_exp, measure, dim)
        c = QuantCase(codes, inv, hip.ROWS_INT8, measure, dim, stride, q, what)
        c.check_distances(5)
        c.check_search(5, [1, 10, MAX_K], "bf_quant_kernel")
        monkeypatch.setenv("SCANN_HIP_BF_SHORTLIST_MIN_ROWS", "1")
        monkeypatch.setenv("SCANN_HIP_BF_SHORTLIST_MIN_QUERIES", "1")
        c = QuantCase(codes, inv, hip.ROWS_INT8, measure, dim, stride, q, what + " shortlist")
        c.check_search(40, [1, 10, 64], "bf_quant_kernel", shortlist=True, check_q=40)
        monkeypatch.delenv("SCANN_HIP_BF_SHORTLIST_MIN_ROWS")
        monkeypatch.delenv("SCANN_HIP_BF_SHORTLIST_MIN_QUERIES")

"""Projected Tree-X-Hybrid / AsymmetricHasher handles (scann_hip_txh_create_projected; include/scann_hip.h "projections",
DESIGN.md 3.3i) against an oracle composed from existing pieces: qp = model.project(q); the oracle's staged search of qp
on an oracle index over the host-projected rows; the oracle's re-rank of that candidate list against the ORIGINAL rows
and the original q.  Tokens and token distances compare bitwise, candidate lists and final rows up to exact ties, as in
the other parity tests (helpers.check_txh_query).  Independent of the oracle: a projected handle's stage outputs equal a
plain handle's over host-projected rows and queries, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import pyoracle as orc
from scann_rust_amd import hip, trainer
from tests import crowding_model as CM
from tests import helpers as H
from tests import projection_model as pm

pytestmark = pytest.mark.gpu

K = 10
MULT = 3.0
M_PRE = orc.pre_reorder_k(K, MULT)
NQ = 200
DEV = "cuda:0"

# name: n, in_dim, out_dim, projection, S, K codes, L (0 = AsymmetricHasher), P
CASES = {
    "ortho-96-32": dict(n=5000, in_dim=96, out_dim=32, proj="ortho", S=8, Kc=16, L=24, P=4),
    "pca-200-64": dict(n=4000, in_dim=200, out_dim=64, proj="pca", S=16, Kc=16, L=16, P=4),
    "pca-768-128": dict(n=4000, in_dim=768, out_dim=128, proj="pca", S=32, Kc=16, L=32, P=4),
    "rotation-64-64": dict(n=4000, in_dim=64, out_dim=64, proj="ortho", S=16, Kc=16, L=16, P=4),
    "truncate-128-32": dict(n=4000, in_dim=128, out_dim=32, proj="truncate", start=17, S=8, Kc=16, L=16, P=4),
    "hasher-96-32": dict(n=4000, in_dim=96, out_dim=32, proj="ortho", S=8, Kc=16, L=0, P=1),
    "bytes-96-32": dict(n=4000, in_dim=96, out_dim=32, proj="ortho", S=4, Kc=256, L=16, P=4),
}


def mult_for(k, m):
    """a pre_reorder_multiplier with (k as f32 * multiplier) as usize == m (tree_x_hybrid/mod.rs:263)"""
    mult = np.float32(m) / np.float32(k)
    while int(np.float32(k) * mult) < m:
        mult = np.nextafter(mult, np.float32(np.inf))
    assert orc.pre_reorder_k(k, float(mult)) == m
    return float(mult)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def spectrum_rows(n, dim, seed):
    """rows with a decaying spectrum (component i has standard deviation (1 + i)^-1/2 in a rotated basis) around a
    non-zero mean, and queries near them"""
    rng = np.random.default_rng(seed)
    basis, _ = np.linalg.qr(rng.standard_normal((dim, dim)))
    sd = (1.0 + np.arange(dim)) ** -0.5
    mean = rng.standard_normal(dim)
    rows = ((rng.standard_normal((n, dim)) * sd) @ basis.T + mean).astype(np.float32)
    q = ((rng.standard_normal((NQ, dim)) * sd) @ basis.T + mean).astype(np.float32)
    return rows, q


class Case:
    def __init__(self, name, measure=hip.SQUARED_L2):
        c = CASES[name]
        self.name, self.c, self.measure = name, c, measure
        n, in_dim, out_dim = c["n"], c["in_dim"], c["out_dim"]
        self.n, self.in_dim, self.out_dim = n, in_dim, out_dim
        self.rows, self.q = spectrum_rows(n, in_dim, len(name) * 1000 + in_dim)
        if c["proj"] == "ortho":
            self.kind, self.M, self.mean, self.start = pm.MATRIX, trainer.random_orthogonal(in_dim, out_dim, 5), None, 0
        elif c["proj"] == "pca":
            self.M, self.mean = trainer.pca_projection(self.rows, out_dim)
            self.kind, self.start = pm.PCA, 0
        else:
            self.kind, self.M, self.mean, self.start = pm.TRUNCATE, None, None, c["start"]
        self.rows_p = self.project(self.rows)
        self.q_p = self.project(self.q)
        self.ah = c["L"] == 0
        if self.ah:
            self.ix = trainer.build_ah_index(self.rows_p, c["S"], K=c["Kc"], pq_iters=3)
        else:
            self.ix = trainer.build_txh_index(self.rows_p, c["L"], c["S"], K=c["Kc"], kmeans_iters=3, pq_iters=3)
        self.data, self.stride = orc.to_strided(self.rows)             # the original rows, as the handle holds them
        self.data_p, self.stride_p = orc.to_strided(self.rows_p)       # the projected rows: the oracle index and the plain handle
        if not self.ah:
            self.oix = orc.TxhIndex(self.data_p, self.stride_p, out_dim, self.ix["centers"], self.ix["leaf_off"],
                                    self.ix["leaf_ids"], self.ix["codebook"], self.ix["codes"], use_residuals=True,
                                    partitions_to_search=c["P"], pre_reorder_multiplier=MULT)
        self._oracle = {}

    def project(self, X):
        return pm.project(self.kind, X, self.M, self.mean, start=self.start, out_dim=self.out_dim)

    def projection(self):
        if self.kind == pm.TRUNCATE:
            return hip.Projection(hip.PROJ_TRUNCATE, in_dim=self.in_dim, out_dim=self.out_dim, start=self.start)
        return hip.Projection(self.kind, matrix=self.M, mean=self.mean)

    def desc(self):
        """txh_create's keyword arguments of the index in the projected space, without rows"""
        ix = self.ix
        if self.ah:
            return dict(dim=self.out_dim, centers=None, leaf_offsets=None, leaf_ids=None, codebook=ix["codebook"],
                        codes=ix["codes"], use_residuals=False, partitions_to_search=1, pre_reorder_multiplier=MULT,
                        distance_measure=self.measure)
        return dict(dim=self.out_dim, centers=ix["centers"], leaf_offsets=ix["leaf_off"], leaf_ids=ix["leaf_ids"],
                    codebook=ix["codebook"], codes=ix["codes"], use_residuals=True, partitions_to_search=self.c["P"],
                    pre_reorder_multiplier=MULT, distance_measure=self.measure)

    def create(self, rows=True):
        p = self.projection()
        try:
            return hip.txh_create_projected(projection=p, rows=self.data if rows else None, n_rows=self.n,
                                            row_dim=self.in_dim, row_stride=self.stride, **self.desc())
        finally:
            p.close()   # the handle keeps its own copy

    def create_plain(self):
        """a plain handle over the host-projected rows"""
        return hip.txh_create(data=self.data_p, n_rows=self.n, stride=self.stride_p, **self.desc())

    def opts(self, m=M_PRE, exact=True):
        o = hip.default_opts()
        o.partitions_to_search = self.c["P"]
        o.pre_reorder_k = m
        o.exact_reorder = 1 if exact else 0
        return o

    def oracle(self, i, k=K, m=M_PRE, allow=None):
        """(final idx, final dist, tokens, token dists, cand idx, cand dist) of query i: stages in the projected space,
        the re-rank against the original rows.  Kept per (i, k, m) while no filter is set."""
        key = (i, k, m)
        if allow is None and key in self._oracle:
            return self._oracle[key]
        qp = self.q_p[i]
        if self.ah:
            assert allow is None
            ci, cd = orc.ah_search(self.ix["codebook"], self.ix["codes"], qp, m)
            tok, tokd = np.zeros(0, np.uint32), np.zeros(0, np.float32)
        else:
            self.oix.pre_reorder_multiplier = mult_for(k, m)
            self.oix.allow = allow
            try:
                _, _, tok, tokd, ci, cd = orc.txh_search(self.oix, qp, k, stages=True)
            finally:
                self.oix.allow = None
                self.oix.pre_reorder_multiplier = MULT
        ri, rd = self.rerank(i, ci, k)
        out = (ri, rd, tok, tokd, ci, cd)
        if allow is None:
            self._oracle[key] = out
        return out

    def rerank(self, i, cand_idx, k):
        if cand_idx.size == 0:
            return np.zeros(0, np.uint32), np.zeros(0, np.float32)
        return orc.reorder_measure(self.data, self.stride, self.in_dim, self.measure, self.q[i], cand_idx, k)

    def check_query(self, i, got_idx, got_dist, st=None, row=None, k=K, m=M_PRE, allow=None, what=""):
        """helpers.check_txh_query with the re-rank in the rows' own space.  st: the stage outputs of the batch (row `row`
        of them is query i's)."""
        oi, od, otok, otokd, oci, ocd = self.oracle(i, k, m, allow)
        what = "%s %s q%d" % (self.name, what, i)
        agree = True
        if st is not None:
            tok, tokd, ci, cd, cc = st
            r = i if row is None else row
            if not self.ah:
                P = otok.size
                assert np.array_equal(tok[r, :P], otok), what + " tokens"
                assert np.array_equal(_bits(tokd[r, :P]), _bits(otokd)), what + " token distances"
            c = int(cc[r])
            gci, gcd = ci[r, :c], cd[r, :c]
            assert c == oci.size, "%s candidate count %d vs %d" % (what, c, oci.size)
            assert np.array_equal(_bits(gcd), _bits(ocd)), what + " approximate distances differ"
            H.assert_topk_equal_up_to_ties(gci, gcd, oci, ocd, what=what + " cand")
            agree = sorted(gci.tolist()) == sorted(oci.tolist())
            if not agree:
                oi, od = self.rerank(i, gci, k)
        assert got_idx.size == oi.size, "%s final count %d vs %d" % (what, got_idx.size, oi.size)
        H.assert_topk_equal_up_to_ties(got_idx, got_dist, oi, od, what=what + " final")


_cases = {}


def case_of(name, measure=hip.SQUARED_L2):
    key = (name, measure)
    if key not in _cases:
        _cases[key] = Case(name, measure)
    return _cases[key]


@pytest.fixture(scope="module")
def ortho():
    c = case_of("ortho-96-32")
    return c, c.create()


def search_and_check(case, index, nq, what, staged=True):
    o = case.opts()
    if staged:
        gi, gd, gc, st = index.search_batched(case.q[:nq], K, o, stages=True)
    else:
        gi, gd, gc = index.search_batched(case.q[:nq], K, o)
        st = None
    for i in range(nq):
        case.check_query(i, gi[i, :gc[i]], gd[i, :gc[i]], st, what=what)
    return gi, gd, gc


# ---- every case against the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_case_matches_the_oracle(name):
    case = case_of(name)
    index = case.create()
    assert index.projection_info() == (case.kind, case.in_dim, case.out_dim, case.start)
    assert index.dimensionality() == case.in_dim and index.size() == case.n
    search_and_check(case, index, 64, "staged outputs")
    search_and_check(case, index, 64, "plain call", staged=False)
    index.close()


@pytest.mark.parametrize("nq", [1, 5, 64, 200])
def test_every_batch_size_takes_the_staged_pipeline(ortho, nq):
    case, index = ortho
    index.enable_timing(True)
    try:
        search_and_check(case, index, nq, "nq=%d" % nq, staged=False)
        ms, kernel = index.last_kernel_ms()
    finally:
        index.enable_timing(False)
    assert ms > 0.0 and kernel.startswith("adc_"), (ms, kernel)   # (the few-query pipelines time small_scan_kernel / wide_scan_kernel)
    search_and_check(case, index, nq, "nq=%d staged" % nq)


def test_without_exact_reorder_no_row_is_read():
    """exact_reorder = 0: the oracle's approximate result on the projected index; a handle without rows gives the same"""
    case = case_of("ortho-96-32")
    poisoned = np.full_like(case.data, np.nan)   # any row read would show as a NaN
    p = case.projection()
    with_rows = hip.txh_create_projected(projection=p, rows=poisoned, n_rows=case.n, row_dim=case.in_dim,
                                         row_stride=case.stride, **case.desc())
    no_rows = case.create(rows=False)
    p.close()
    o = case.opts(exact=False)
    for index in (with_rows, no_rows):
        gi, gd, gc = index.search_batched(case.q[:32], K, o)
        for i in range(32):
            case.oix.pre_reorder_multiplier = 1.0   # (pre_reorder_k is ignored: the k best by approximate distance)
            try:
                _, _, _, _, ci, cd = orc.txh_search(case.oix, case.q_p[i], K, stages=True)
            finally:
                case.oix.pre_reorder_multiplier = MULT
            assert int(gc[i]) == ci.size and np.array_equal(_bits(gd[i, :gc[i]]), _bits(cd)), i
            H.assert_topk_equal_up_to_ties(gi[i, :gc[i]], gd[i, :gc[i]], ci, cd, what="approx q%d" % i)
    with pytest.raises(hip.ScannError) as e:   # exact re-ordering needs the rows (build_no_store)
        no_rows.search_batched(case.q[:4], K, case.opts())
    assert e.value.code == hip.FAILED_PRECONDITION
    with_rows.close()
    no_rows.close()


def test_dot_product_rerank():
    case = case_of("ortho-96-32", hip.DOT_PRODUCT)
    index = case.create()
    gi, gd, gc = search_and_check(case, index, 40, "dot")
    assert (gd[:, 0] < 0).any()   # the negated dot product of the ORIGINAL vectors
    index.close()


# ---- independent of the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ortho-96-32", "pca-768-128", "hasher-96-32"])
def test_stage_outputs_equal_a_plain_handle_over_projected_rows(name):
    case = case_of(name)
    proj, plain = case.create(), case.create_plain()
    o = case.opts()
    a = proj.search_batched(case.q[:64], K, o, stages=True)[3]
    b = plain.search_batched(case.q_p[:64], K, o, stages=True)[3]
    tok_a, tokd_a, ci_a, cd_a, cc_a = a
    tok_b, tokd_b, ci_b, cd_b, cc_b = b
    assert np.array_equal(cc_a, cc_b)
    if not case.ah:
        P = case.c["P"]
        assert np.array_equal(tok_a[:, :P], tok_b[:, :P]) and np.array_equal(_bits(tokd_a[:, :P]), _bits(tokd_b[:, :P]))
    for i in range(64):
        c = int(cc_a[i])
        assert np.array_equal(ci_a[i, :c], ci_b[i, :c]) and np.array_equal(_bits(cd_a[i, :c]), _bits(cd_b[i, :c])), i
    proj.close()
    plain.close()


def test_identity_projection_returns_a_plain_handles_rows():
    dim, n = 64, 4000
    rows, q = spectrum_rows(n, dim, 77)
    ix = trainer.build_txh_index(rows, 16, 16, kmeans_iters=3, pq_iters=3)
    data, stride = orc.to_strided(rows)
    desc = dict(dim=dim, centers=ix["centers"], leaf_offsets=ix["leaf_off"], leaf_ids=ix["leaf_ids"], codebook=ix["codebook"],
                codes=ix["codes"], use_residuals=True, partitions_to_search=4, pre_reorder_multiplier=MULT)
    plain = hip.txh_create(data=data, n_rows=n, stride=stride, **desc)
    p = hip.Projection(hip.PROJ_MATRIX, matrix=np.eye(dim, dtype=np.float32))
    proj = hip.txh_create_projected(projection=p, rows=data, n_rows=n, row_dim=dim, row_stride=stride, **desc)
    o = hip.default_opts()
    o.partitions_to_search, o.pre_reorder_k = 4, M_PRE
    for nq in (64,):
        a = plain.search_batched(q[:nq], K, o, stages=True)
        b = proj.search_batched(q[:nq], K, o, stages=True)
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))
        for x, y in zip(a[3], b[3]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert plain.projection_info() == (0, 0, 0, 0)
    plain.close()
    proj.close()
    p.close()


@pytest.mark.parametrize("scan", ["gather", "resident", "dense32", "mfma16", "sp-lanes", "sp-words"])
def test_every_scan_returns_the_same_rows(monkeypatch, scan):
    case = case_of("ortho-96-32")
    H.scan_env(monkeypatch, "default")
    index = case.create()
    want = index.search_batched(case.q[:64], K, case.opts())
    index.close()
    H.scan_env(monkeypatch, scan)   # (before create: SMFMAC = 0 builds no operand planes)
    index = case.create()
    got = index.search_batched(case.q[:64], K, case.opts())
    assert np.array_equal(got[2], want[2]) and np.array_equal(_bits(got[1]), _bits(want[1])) and np.array_equal(got[0], want[0])
    for i in range(0, 64, 8):
        case.check_query(i, got[0][i, :got[2][i]], got[1][i, :got[2][i]], what=scan)
    index.close()


# ---- entry points ------------------------------------------------------------------------------------------------------
def test_device_entry_after_reserve_on_two_streams(ortho):
    case, index = ortho
    nq = 48
    o = case.opts()
    hip.check(hip.load().scann_hip_index_reserve(index.h, nq, K, ctypes.byref(o)))
    dev = torch.device(DEV)
    L = hip.load()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    halves = [(0, nq), (nq, 2 * nq)]
    bufs = []
    for (a, b) in halves:
        bufs.append((torch.from_numpy(case.q[a:b]).to(dev), torch.full((nq, K), -1, dtype=torch.int32, device=dev),
                     torch.zeros((nq, K), dtype=torch.float32, device=dev), torch.zeros((nq,), dtype=torch.int32, device=dev)))
    torch.cuda.synchronize()
    for s, (qd, oi, od, oc) in zip(streams, bufs):   # both enqueued before either is waited for
        hip.check(L.scann_hip_search_batched_device(index.h, vp(qd), nq, case.in_dim, K, ctypes.byref(o), vp(oi), vp(od),
                                                    vp(oc), ctypes.c_void_p(s.cuda_stream)))
    for s in streams:
        assert L.scann_hip_index_last_device_status(index.h, ctypes.c_void_p(s.cuda_stream)) == 0
    torch.cuda.synchronize()
    for (a, b), (qd, oi, od, oc) in zip(halves, bufs):
        gi, gd, gc = oi.cpu().numpy().view(np.uint32), od.cpu().numpy(), oc.cpu().numpy()
        for i in range(a, b):
            case.check_query(i, gi[i - a, :gc[i - a]], gd[i - a, :gc[i - a]], what="device stream")


def test_search_batched_params_mixed_k(ortho):
    case, index = ortho
    ks = np.array([1, 10, 5, 30, 2, 10, 7, 1, 20], np.uint32)
    m = 30
    gi, gd, gc = index.search_batched_with_params(case.q[:ks.size], ks, case.opts(m))
    for i, k in enumerate(ks.tolist()):
        case.check_query(i, gi[i, :gc[i]], gd[i, :gc[i]], k=k, m=m, what="mixed k")


def test_allow_bitmap_per_call_and_per_query(ortho):
    case, index = ortho
    rng = np.random.default_rng(3)
    nq = 12
    allow = hip.allow_bitmap(case.n, rng.choice(case.n, case.n // 3, replace=False))
    gi, gd, gc, st = index.search_batched(case.q[:nq], K, case.opts(), stages=True, allow=allow)
    for i in range(nq):
        case.check_query(i, gi[i, :gc[i]], gd[i, :gc[i]], st, allow=allow, what="allow")
        assert all((int(allow[j >> 6]) >> (j & 63)) & 1 for j in gi[i, :gc[i]].tolist())
    per = np.stack([hip.allow_bitmap(case.n, rng.choice(case.n, 200 + 300 * i, replace=False)) for i in range(nq)])
    gi, gd, gc = index.search_batched(case.q[:nq], K, case.opts(), allow=per)
    for i in range(nq):
        case.check_query(i, gi[i, :gc[i]], gd[i, :gc[i]], allow=per[i], what="allow per query")


def test_token_map_search(ortho):
    case, index = ortho
    nq = 6
    ids = np.arange(case.n, dtype=np.uint32)
    tokens = (ids % 7).astype(np.uint64)
    tm = hip.TokenMap(case.n, ids, tokens)
    lists = [[i % 7, (i + 3) % 7] for i in range(nq)]
    gi, gd, gc = tm.search_batched(index, case.q[:nq], K, lists, case.opts())
    for i in range(nq):
        allow = hip.allow_bitmap(case.n, ids[np.isin(tokens, lists[i])])
        case.check_query(i, gi[i, :gc[i]], gd[i, :gc[i]], allow=allow, what="tokens")
    tm.close()


def test_search_crowded(ortho):
    case, index = ortho
    depth, limit, nq, m = 30, 2, 10, 60
    attrs = (np.arange(case.n, dtype=np.uint64) % np.uint64(5))
    index.set_crowding_attributes(attrs)
    try:
        gi, gd, gc = index.search_crowded(case.q[:nq], K, depth, limit, case.opts(m))
    finally:
        index.set_crowding_attributes(None)
    rows = index.search_batched(case.q[:nq], depth, case.opts(m))
    for i in range(nq):
        oi, od = case.oracle(i, depth, m)[:2]
        H.assert_topk_equal_up_to_ties(rows[0][i, :rows[2][i]], rows[1][i, :rows[2][i]], oi, od, what="depth rows q%d" % i)
        wi, wd = CM.apply_fast(oi, od, attrs, limit, K)
        c = int(gc[i])
        assert c == wi.size and np.array_equal(_bits(gd[i, :c]), _bits(wd)), i
        if np.array_equal(rows[0][i, :rows[2][i]], oi):   # (no exact tie reordered the rows the stage read)
            assert np.array_equal(gi[i, :c], wi), i


# ---- index files -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pca-200-64", "ortho-96-32", "truncate-128-32", "hasher-96-32"])
def test_index_file_round_trip(tmp_path, name):
    from scann_rust_amd import index_file
    case = case_of(name)
    index = case.create()
    path = str(tmp_path / "p.scannidx")
    hip.index_write_file(index, path)
    info = hip.index_file_info(path)
    assert info["has_data"] == 1 and info["dim"] == case.out_dim and info["n_rows"] == case.n   # the index space
    a = index_file.arrays(path)
    assert a["projection"] == dict(kind=case.kind, in_dim=case.in_dim, out_dim=case.out_dim, start=case.start,
                                   row_stride=case.stride)
    assert np.array_equal(a["proj_meta"], np.array([case.kind, case.in_dim, case.out_dim, case.start, case.stride], np.uint32))
    assert np.array_equal(a["data"].view(np.uint32), case.data.reshape(case.n, case.stride).view(np.uint32))
    if case.kind == pm.TRUNCATE:
        assert "proj_matrix" not in a and "proj_mean" not in a
    else:
        assert np.array_equal(a["proj_matrix"].view(np.uint32), case.M.view(np.uint32))
        assert ("proj_mean" in a) == (case.kind == pm.PCA)
        if case.kind == pm.PCA:
            assert np.array_equal(np.asarray(a["proj_mean"]).view(np.uint32), case.mean.view(np.uint32))
    loaded = hip.load_file(path)
    assert loaded.projection_info() == index.projection_info() and loaded.dimensionality() == case.in_dim
    o = case.opts()
    a0, a1 = index.search_batched(case.q[:32], K, o), loaded.search_batched(case.q[:32], K, o)
    assert np.array_equal(a0[2], a1[2]) and np.array_equal(_bits(a0[1]), _bits(a1[1])) and np.array_equal(a0[0], a1[0])
    for i in range(0, 32, 4):
        case.check_query(i, a1[0][i, :a1[2][i]], a1[1][i, :a1[2][i]], what="loaded")
    assert loaded.device_bytes() == index.device_bytes()
    index.close()
    loaded.close()


def test_index_file_without_rows_and_plain_files_still_load(tmp_path):
    import os
    case = case_of("ortho-96-32")
    index = case.create(rows=False)
    path = str(tmp_path / "norows.scannidx")
    hip.index_write_file(index, path)
    assert hip.index_file_info(path)["has_data"] == 0
    loaded = hip.load_file(path)
    assert loaded.projection_info() == index.projection_info()
    o = case.opts(exact=False)
    a0, a1 = index.search_batched(case.q[:8], K, o), loaded.search_batched(case.q[:8], K, o)
    assert np.array_equal(a0[0], a1[0]) and np.array_equal(_bits(a0[1]), _bits(a1[1]))
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "txh_small.scannidx")
    assert hip.load_file(golden).projection_info() == (0, 0, 0, 0)


def test_corrupt_proj_meta_is_data_loss(tmp_path):
    from scann_rust_amd import index_file
    case = case_of("pca-200-64")
    index = case.create()
    good = str(tmp_path / "good.scannidx")
    hip.index_write_file(index, good)
    index.close()
    h, s = index_file.read(good)
    names = list(s)
    DATA_LOSS = 15

    def rewrite(path, change=None, drop=()):
        secs = []
        for nm in names:
            if nm in drop:
                continue
            arr = np.array(s[nm])
            if change and nm in change:
                arr = change[nm](arr)
            secs.append((nm, arr))
        index_file.write(path, kind=1, **{k: h[k] for k in (
            "n_rows", "n_local", "dim", "stride", "num_partitions", "num_subspaces", "num_codes", "dims_per_subspace",
            "distance_measure", "data_is_csr_order", "codes_packed4", "use_residuals", "partitions_to_search",
            "pre_reorder_multiplier")}, sections=secs)

    def meta(i, v):
        def f(a):
            a = a.copy()
            a[i] = v
            return a
        return {"proj_meta": f}

    again = str(tmp_path / "again.scannidx")
    rewrite(again)
    assert hip.load_file(again).projection_info() == (pm.PCA, 200, 64, 0)   # the rewriter itself is sound
    bad = {
        "kind": meta(0, 9), "in_dim": meta(1, 199), "out_dim": meta(2, 32), "start": meta(3, 1),
        "row_stride": meta(4, 100), "short meta": {"proj_meta": lambda a: a[:4]},
        "short matrix": {"proj_matrix": lambda a: a[:-1]}, "short mean": {"proj_mean": lambda a: a[:-1]},
    }
    for what, change in bad.items():
        path = str(tmp_path / "bad.scannidx")
        rewrite(path, change)
        with pytest.raises(hip.ScannError) as e:
            hip.load_file(path)
        assert e.value.code == DATA_LOSS, (what, e.value)
    for drop in ("proj_matrix", "proj_mean"):
        path = str(tmp_path / "drop.scannidx")
        rewrite(path, drop=(drop,))
        with pytest.raises(hip.ScannError) as e:
            hip.load_file(path)
        assert e.value.code == DATA_LOSS, (drop, e.value)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def _raises(code, word, fn, *a, **kw):
    with pytest.raises(hip.ScannError) as e:
        fn(*a, **kw)
    assert e.value.code == code, e.value
    assert word in e.value.message, e.value.message


def test_unimplemented_on_a_projected_handle(ortho, tmp_path):
    case, index = ortho
    un = hip.UNIMPLEMENTED
    _raises(un, "projection", index.search_mmr, case.q[:2], K, 20, 0.5, case.opts())
    _raises(un, "projection", hip.Mutable, index, 16)
    _raises(un, "projection", index.quantize_rows, hip.ROWS_BF16)
    _raises(un, "projection", hip.quantization_stats, index)
    _raises(un, "projection", index.debug_rerank_brackets, 1, M_PRE)
    L = hip.load()
    dev = torch.device(DEV)
    qd = torch.from_numpy(case.q[:2]).to(dev)
    keys = torch.zeros((2, M_PRE), dtype=torch.int64, device=dev)
    idx = torch.zeros((2, M_PRE), dtype=torch.int32, device=dev)
    ex = torch.zeros((2, M_PRE), dtype=torch.float32, device=dev)
    cnt = torch.zeros((2,), dtype=torch.int32, device=dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    o = case.opts()
    s = L.scann_hip_txh_search_local_device(index.h, vp(qd), 2, case.in_dim, K, ctypes.byref(o), vp(keys), vp(idx), vp(ex),
                                            vp(cnt), None)
    assert s == un and b"projection" in L.scann_hip_last_error()
    # rebase of a mutable index onto a projected base: from a plain base of the same index space and size, which the
    # rebase would otherwise accept.  (A fold onto a projected base is unreachable: create and rebase both refuse, so no
    # mutable index ever stands on one.)
    plain = case.create_plain()
    mut = hip.Mutable(plain, 16)
    _raises(un, "projection", mut.rebase, index)
    assert mut.base is plain
    mut.close()
    plain.close()
    # the leaf-sharded entry point (a one-rank communicator)
    comm = hip.Comm(hip.Comm.unique_id(), 0, 1)
    oi = torch.empty((2, K), dtype=torch.int32, device=dev)
    od = torch.empty((2, K), dtype=torch.float32, device=dev)
    oc = torch.empty((2,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    s = L.scann_hip_txh_search_sharded_device(index.h, comm.h, vp(qd), 2, case.in_dim, K, None, 0, vp(oi), vp(od), vp(oc),
                                              None)
    assert s == un and b"projection" in L.scann_hip_last_error()
    torch.cuda.synchronize()
    # the stage functions stay in index space: out_dim queries
    tok, _, cnt = hip.txh_partition(index, case.q_p[:3], case.c["P"])
    assert np.array_equal(tok[0, :cnt[0]], case.oracle(0)[2])
    _raises(hip.INVALID_ARGUMENT, "mismatch", hip.txh_partition, index, case.q[:3], case.c["P"])


def test_create_refusals():
    case = case_of("ortho-96-32")
    p = case.projection()
    kw = dict(projection=p, rows=case.data, n_rows=case.n, row_dim=case.in_dim, row_stride=case.stride)
    d = case.desc()
    un, inv = hip.UNIMPLEMENTED, hip.INVALID_ARGUMENT
    sizes = np.diff(case.ix["leaf_off"]).astype(np.uint32)
    _raises(un, "projection", hip.txh_create_projected, **kw, **dict(d, leaf_sizes_global=sizes))
    _raises(un, "projection", hip.txh_create_projected, **kw, **dict(d, data_is_csr_order=True))
    _raises(un, "projection", hip.txh_create_projected, **kw, **dict(d, codebook=None, codes=None))
    _raises(inv, "out_dim", hip.txh_create_projected, **kw, **dict(d, dim=case.out_dim * 2))
    _raises(inv, "in_dim", hip.txh_create_projected, **dict(kw, row_dim=case.in_dim - 1), **d)
    _raises(inv, "row_stride", hip.txh_create_projected, **dict(kw, row_stride=case.in_dim - 1, rows=None), **d)
    _raises(inv, "projection is null", hip.txh_create_projected, **dict(kw, projection=None), **d)
    _raises(inv, "n_rows", hip.txh_create_projected, **dict(kw, n_rows=case.n - 1), **d)    # a leaf_ids entry past the rows
    # desc.data != NULL: through the raw call (the wrapper refuses data= itself)
    with pytest.raises(ValueError):
        hip.txh_create_projected(**kw, **dict(d, data=case.data_p))
    desc, keep = hip._txh_desc(data=case.data_p, n_rows=case.n, stride=case.stride_p, **d)
    h = ctypes.c_void_p()
    L = hip.load()
    s = L.scann_hip_txh_create_projected(hip.context(0), ctypes.byref(desc), p.h, hip.ptr(case.data, hip.f32p), case.n,
                                         case.in_dim, case.stride, ctypes.byref(h))
    assert s == inv and b"desc.data must be NULL" in L.scann_hip_last_error()
    # queries of the index space are refused by the search entries: q_dim compares against row_dim
    index = hip.txh_create_projected(**kw, **d)
    _raises(inv, "mismatch", index.search_batched, case.q_p[:2], K, case.opts())
    index.close()
    p.close()

"""Checkers shared by the cases of tests/test_gpu_high_dim.py: the standards of tests/test_gpu_build.py (assignment,
Lloyd) and tests/test_gpu_quantized_rerank.py (quantized re-rank rows), restated here so that the high-dim tests do not
reach into other test modules.  Test infrastructure: needs the library, and a GPU only when a checker is called."""
import numpy as np

from oracle import pyoracle as orc
from scann_rust_amd import hip, synth
from tests import helpers as H
from tests import quantized_rerank_cases as QC

SENT = 0xFFFFFFFF


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- scann_hip_bf_assign_nearest, scann_hip_kmeans_lloyd -------------------------------------------------------------
def nearest_reference(rows, centers):
    """(token [n], dist [n] f32) of TreePartitioner::partition(x, 1) for every row"""
    tok = np.empty(rows.shape[0], np.uint32)
    dist = np.empty(rows.shape[0], np.float32)
    for i, r in enumerate(rows):
        t, d = orc.partition(centers, r, 1)
        tok[i], dist[i] = t[0], d[0]
    return tok, dist


def check_assign(index, n, centers, want_tok, want_dist, what):
    """tokens equal, distances bitwise (a row whose every distance is NaN reports +inf), and out_dist = NULL"""
    tok, dist = hip.bf_assign_nearest(index, centers)
    assert np.array_equal(tok, want_tok[:n]), "%s: tokens differ at rows %s" % (what, np.flatnonzero(tok != want_tok[:n])[:8])
    want = np.where(np.isnan(want_dist[:n]), np.float32(np.inf), want_dist[:n])
    assert np.array_equal(bits(dist), bits(want)), "%s: distances differ at rows %s" % (
        what, np.flatnonzero(bits(dist) != bits(want))[:8])
    assert np.array_equal(hip.bf_assign_nearest(index, centers, want_dist=False), tok), "%s: out_dist = NULL" % what


def check_lloyd(index, data, n, stride, init, thr, max_iterations=2, what=""):
    """centres bitwise, assignment, sizes, the f64 inertia bits, the iteration count and the converged flag against
    the oracle"""
    sub = init.shape[1]
    g = hip.kmeans_lloyd(index, init, max_iterations=max_iterations, simd_threshold=thr)
    o = orc.kmeans_lloyd(data, n, stride, sub, init, max_iterations=max_iterations, simd_threshold=thr)
    assert (g[4], g[5]) == (o[4], o[5]), "%s: iterations / converged %s vs %s" % (what, g[4:], o[4:])
    assert np.array_equal(g[1], o[1]), "%s: assignment differs at rows %s" % (what, np.flatnonzero(g[1] != o[1])[:8])
    assert np.array_equal(g[2], o[2]), "%s: sizes" % what
    assert np.array_equal(bits(g[0]), bits(o[0])), what + " centres"
    assert np.float64(g[3]).view(np.uint64) == np.float64(o[3]).view(np.uint64), "%s: inertia %r vs %r" % (what, g[3], o[3])


# ---- scann_hip_txh_create_quantized ------------------------------------------------------------------------------------
class RerankBase(QC.Base):
    """QC.Base at a dim outside its SHAPES table.  QC.Base.__init__ looks the subspace count up there, so this
    constructor does not call it: it builds the same attributes (the candidates / model_rows / desc / opts methods read
    nothing else) with the subspace count given."""

    def __init__(self, dim, S, n=2048, seed=11, nq=17, leaves=8, p=QC.P):
        self.dim, self.n, self.p = dim, n, p
        self.rows, _, _, ix, ah_kw = H.make_ah_case(n, dim, S, seed, K=16, pq_iters=2)
        self.cb, self.codes = ix["codebook"], np.ascontiguousarray(ix["codes"], np.uint8)
        self.ah_kw = {k: v for k, v in ah_kw.items() if k not in ("data", "stride")}
        self.oix, kw = H.txh_from_codes(self.rows, self.cb, self.codes, leaves, p, 3.0, seed=seed, use_residuals=False)
        self.txh_kw = {k: v for k, v in kw.items() if k not in ("data", "stride")}
        self.q = synth.uniform_f32(nq, dim, seed + 100)
        self._cands = {}
        self.csr_of = np.empty(n, np.int64)
        self.csr_of[self.oix.leaf_ids.astype(np.int64)] = np.arange(n)



def run_quantized_rerank(base, kind, rows_q, fmt, measure, inv, k, m, nq, what, stages=True, bf=True):
    """one handle, one batch: the plain call and the staged call bitwise against quantized_rerank_model fed with the
    oracle's merged candidates, the device's candidate list against the same list (approximate distances bitwise,
    membership up to their ties), and every returned distance the quantized brute-force handle's"""
    q = base.q[:nq]
    index = hip.txh_create_quantized(rows=rows_q, fmt=fmt, inv_multiplier=inv, **base.desc(kind, rows_q.shape[1], measure))
    want = base.model_rows(kind, rows_q, fmt, measure, inv, k, m, nq)
    got = index.search_batched(q, k, base.opts(kind, m))
    _assert_rows(got, want, k, what)
    if stages:
        gi, gd, gc, (tok, tokd, ci, cd, cc) = index.search_batched(q, k, base.opts(kind, m), stages=True)
        for i in range(nq):
            oci, ocd = base.candidates(kind, i, m)
            c = int(cc[i])
            assert c == oci.size, (what, i, c, oci.size)
            assert np.array_equal(bits(cd[i, :c]), bits(ocd)), (what, i)
            H.assert_topk_equal_up_to_ties(ci[i, :c], cd[i, :c], oci, ocd, what="%s cand q%d" % (what, i))
        _assert_rows((gi, gd, gc), want, k, what + " staged")
    if bf:
        twin = hip.bf_create_quantized(rows_q, rows_q.shape[0], base.dim, rows_q.shape[1], fmt, measure, inv)
        d = hip.bf_distances(twin, q)
        for i in range(nq):
            c = int(got[2][i])
            assert np.array_equal(bits(got[1][i, :c]), bits(d[i, got[0][i, :c].astype(np.int64)])), (what, i)
        twin.close()
    index.close()


def _assert_rows(got, want, k, what):
    gi, gd, gc = got
    for i, (wi, wd) in enumerate(want):
        c = int(gc[i])
        assert c == wi.size, (what, i, c, wi.size)
        assert np.array_equal(bits(gd[i, :c]), bits(wd)), (what, i, gd[i, :c], wd)
        assert np.array_equal(gi[i, :c], wi), (what, i, gi[i, :c], wi)
        assert np.all(gi[i, c:k] == SENT), (what, i)

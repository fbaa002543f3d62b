"""Indexes over quantized rows for tests/test_quantized_rerank_model.py and tests/test_gpu_quantized_rerank.py: one
trained codebook per (dim, n), a tree view (helpers.txh_from_codes) and a flat-hasher view (helpers.make_ah_case) over
the same codes, the rows quantized to each format on the host, and the oracle's merged candidates per query.

The candidate stages read codes, centres and the query only, so the oracle's candidates of an index over ANY f32 rows
are the candidates of the quantized-row index.  MERGED ORDER is ascending (approximate distance, merge key), the merge
key being the candidate's position in the query's stream: the probed leaves in token order, each in CSR order (a flat
hasher's stream is the datapoints in index order).  The oracle returns candidates of equal approximate distance in
its heap's order, so merged_order() re-sorts those groups by the merge key; everything else it leaves alone."""
import numpy as np

from oracle import pyoracle as orc
from scann_rust_amd import hip, synth
from tests import helpers as H
from tests import quantized_checker as qc
from tests import quantized_rerank_model as QM

LEAVES, P = 16, 4
FMTS = {"bf16": qc.ROWS_BF16, "fp8": qc.ROWS_FP8_E4M3, "int8": qc.ROWS_INT8}
MEASURES = {"sql2": qc.SQUARED_L2, "l2": qc.L2, "dot": qc.DOT_PRODUCT}
DTYPES = {qc.ROWS_BF16: np.uint16, qc.ROWS_FP8_E4M3: np.uint8, qc.ROWS_INT8: np.int8}
# dim -> (S, K): 8 = one dimension per subspace; 12 and 36 = byte codes, the only shapes with dim % 8 != 0 (the int8
# tail); 264 = past one 256-element block
SHAPES = {8: (8, 16), 12: (4, 256), 36: (4, 256), 64: (16, 16), 96: (24, 16), 128: (32, 16), 264: (24, 16)}


def quantize(rows, fmt):
    """(elements [n, dim] of the format's dtype, inv_multiplier) by the host quantizers"""
    x = np.ascontiguousarray(rows, np.float32)
    if fmt == qc.ROWS_BF16:
        return qc.bf16_from_f32(x), 1.0
    if fmt == qc.ROWS_FP8_E4M3:
        mx = float(np.max(np.abs(x[np.isfinite(x)]))) if np.isfinite(x).any() else 0.0
        return orc.fp8_quantize(x, 400.0 / mx if mx > 0 else 1.0), 1.0
    codes, inv = hip.symmetric_int8(x)
    return codes, inv


def with_stride(elems, stride, seed):
    """[n, stride] rows whose padding holds junk (a bf16 NaN pattern among it: a read of it would show)"""
    n, dim = elems.shape
    rng = np.random.default_rng([seed, stride])
    out = rng.integers(0, 1 << (8 * elems.dtype.itemsize), size=(n, stride), dtype=np.uint64).astype(
        np.uint16 if elems.dtype.itemsize == 2 else np.uint8).view(elems.dtype)
    if elems.dtype.itemsize == 2 and stride > dim:
        out[:, dim] = 0x7FC1
    out[:, :dim] = elems
    return np.ascontiguousarray(out)


def strides(dim):
    return (dim, dim + 5, (dim + 16) // 16 * 16)


def merged_order(ci, cd, vpos):
    """candidates (indices, approximate distances) stably sorted by (ordered distance, stream position vpos[i])"""
    key = (QM.f32_to_ordered(cd).astype(np.uint64) << np.uint64(32)) | np.asarray(vpos, np.uint64)
    order = np.argsort(key, kind="stable")
    return np.asarray(ci)[order], np.asarray(cd)[order]


class Base:
    """rows, codebook and codes of one (dim, n), with the tree and the flat-hasher descriptors over them"""

    def __init__(self, dim, n=4096, seed=11, nq=70, leaves=LEAVES, p=P):
        S, K = SHAPES[dim]
        self.dim, self.n, self.p = dim, n, p
        self.rows, _, _, ix, ah_kw = H.make_ah_case(n, dim, S, seed, K=K, pq_iters=2)
        self.cb, self.codes = ix["codebook"], np.ascontiguousarray(ix["codes"], np.uint8)
        self.ah_kw = {k: v for k, v in ah_kw.items() if k not in ("data", "stride")}
        self.oix, kw = H.txh_from_codes(self.rows, self.cb, self.codes, leaves, p, 3.0, seed=seed, use_residuals=False)
        self.txh_kw = {k: v for k, v in kw.items() if k not in ("data", "stride")}
        self.q = synth.uniform_f32(nq, dim, seed + 100)
        self._cands = {}
        self.csr_of = np.empty(n, np.int64)            # CSR position of every datapoint in the tree view
        self.csr_of[self.oix.leaf_ids.astype(np.int64)] = np.arange(n)

    def desc(self, kind, stride, measure):
        return dict(self.ah_kw if kind == "ah" else self.txh_kw, stride=stride, distance_measure=measure)

    def opts(self, kind, m, p=None):
        o = hip.default_opts()
        o.pre_reorder_k = m
        if kind == "txh":
            o.partitions_to_search = p or self.p
        return o

    def candidates(self, kind, qi, m, q=None, p=None, allow=None):
        """the oracle's merged candidates (indices, approximate distances) of query qi at pre-reorder count m; `allow`:
        an allow-bitmap (tree view only)"""
        key = (kind, qi, m, p) if q is None and allow is None else None
        if key is not None and key in self._cands:
            return self._cands[key]
        qv = self.q[qi] if q is None else q
        if kind == "ah":
            assert allow is None
            ci, cd = orc.ah_search(self.cb, self.codes, qv, m)
            out = merged_order(ci, cd, ci)
        else:
            o = self.oix
            oix = orc.TxhIndex(o.data, o.stride, o.dim, o.centers, o.leaf_off, o.leaf_ids, o.codebook, o.codes,
                               use_residuals=False, partitions_to_search=p or self.p,
                               pre_reorder_multiplier=(m + 0.5) / 64)
            assert orc.pre_reorder_k(64, oix.pre_reorder_multiplier) == m
            oix.allow = allow
            _, _, tok, _, ci, cd = orc.txh_search(oix, qv, 64, stages=True)
            # stream position: the sizes of the leaves probed before the candidate's, plus its place in its leaf
            off = o.leaf_off.astype(np.int64)
            start = np.full(off.size - 1, -1, np.int64)
            start[tok.astype(np.int64)] = np.concatenate([[0], np.cumsum(off[tok.astype(np.int64) + 1] - off[tok.astype(np.int64)])[:-1]])
            csr = self.csr_of[ci.astype(np.int64)]
            leaf = np.searchsorted(off, csr, side="right") - 1
            assert (start[leaf] >= 0).all()
            out = merged_order(ci, cd, start[leaf] + csr - off[leaf])
        if key is not None:
            self._cands[key] = out
        return out

    def model_rows(self, kind, rows_q, fmt, measure, inv, k, m, nq, queries=None, p=None, allow=None):
        """[(indices, distances)] of the model for the first nq queries; k: one value or one per query; allow: one
        bitmap or a [nq, words] block of them"""
        out = []
        for i in range(nq):
            qv = self.q[i] if queries is None else queries[i]
            al = None if allow is None else (allow[i] if np.ndim(allow) == 2 else allow)
            ci, _ = self.candidates(kind, i, m, None if queries is None else qv, p, al)
            out.append(QM.rerank(qv, ci, rows_q, self.dim, fmt, measure, inv, int(np.ravel(k)[i % np.size(k)])))
        return out

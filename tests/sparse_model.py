"""numpy model of the sparse brute-force search (scann_hip.h "sparse brute force"): rows and queries densified into
f32 arrays, every (query, row) sum accumulated one dimension at a time in f32 -- the sequential sum over the
dimensions stored in both, ascending, for every pair at once -- lengths and counts taken from the index lists, results
from a sort on the (f32_to_ordered(distance), row) keys.

Only the columns some query stores are densified: in any other column every query holds 0.0, the term is 0 * x with x
finite, and adding +-0 to a sum that started at +0.0 changes nothing (the sum is never -0.0), so dropping those steps is
exact; it keeps D = 2^20 within memory."""
import numpy as np

from scann_rust_amd import hip   # (the measure constants only)

F = np.float32


def csr(lists):
    """(offsets uint64[n + 1], dims uint32[nnz], vals float32[nnz]) of a list of (dims, vals) pairs"""
    off = np.concatenate([[0], np.cumsum([len(d) for d, _ in lists])]).astype(np.uint64)
    return (off, np.concatenate([np.asarray(d, np.uint32) for d, _ in lists] + [np.zeros(0, np.uint32)]),
            np.concatenate([np.asarray(v, F) for _, v in lists] + [np.zeros(0, F)]))


def _lens(off):
    return np.diff(off.astype(np.int64))


def _dense(off, dims, vals, cols):
    """(values [n, C] f32, stored [n, C] bool) over the ascending columns `cols`"""
    n, lens = off.size - 1, _lens(off)
    x, st = np.zeros((n, cols.size), F), np.zeros((n, cols.size), bool)
    row = np.repeat(np.arange(n), lens)
    c = np.searchsorted(cols, dims)
    keep = (c < cols.size) & (cols[np.minimum(c, max(cols.size - 1, 0))] == dims) if cols.size else np.zeros(dims.size, bool)
    x[row[keep], c[keep]] = vals[keep]
    st[row[keep], c[keep]] = True
    return x, st


def squared_norms(off, vals):
    """one sequential f32 sum of v * v per list, in stored order, from 0"""
    lens, start = _lens(off), off[:-1].astype(np.int64) - int(off[0])
    s = np.zeros(lens.size, F)
    for t in range(int(lens.max()) if lens.size else 0):
        m = lens > t
        v = vals[start[m] + t]
        s[m] = s[m] + v * v
    return s


def distances(measure, rows, queries):
    """[nq, n] f32; rows and queries are (offsets, dims, vals)"""
    cols = np.unique(queries[1])
    x, xs = _dense(*rows, cols)
    q, qs = _dense(*queries, cols)
    xl, ql = _lens(rows[0])[None, :], _lens(queries[0])[:, None]
    if measure in (hip.DOT_PRODUCT, hip.COSINE):
        s = np.zeros((q.shape[0], x.shape[0]), F)
        for d in range(cols.size):
            s = (s + q[:, None, d] * x[None, :, d]).astype(F)
        if measure == hip.DOT_PRODUCT:
            return -s
        nq, nx = np.sqrt(squared_norms(queries[0], queries[2]))[:, None], np.sqrt(squared_norms(rows[0], rows[2]))[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            sim = np.where((nq == 0) | (nx == 0), F(0), s / (nq * nx)).astype(F)
        return F(1) - sim
    if measure == hip.SPARSE_NONZERO_INTERSECT:
        c = (qs & (q != 0)).astype(F) @ (xs & (x != 0)).astype(F).T     # exact: counts far below 2^24
        return (-c.astype(np.int64)).astype(F)
    c = (qs.astype(F) @ xs.astype(F).T).astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if measure == hip.SPARSE_JACCARD:
            d = F(1) - c.astype(F) / (ql + xl - c).astype(F)
        else:
            d = F(1) - (F(2) * c.astype(F)) / (ql + xl).astype(F)
    return np.where((ql == 0) & (xl == 0), F(0), d).astype(F)


def ordered(dist):
    b = np.ascontiguousarray(dist, F).view(np.uint32).astype(np.uint64)
    return np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000)


def search(dist, k, allowed=None):
    """(idx [nq, k], dist [nq, k], count [nq]) of a distance matrix: the k smallest (ordered(distance), row) keys of the
    allowed rows, ascending; slots past count hold the halves of the all-ones key: 0xFFFFFFFF, NaN 0x7FFFFFFF"""
    nq, n = dist.shape
    rows = np.arange(n, dtype=np.uint64) if allowed is None else np.flatnonzero(allowed).astype(np.uint64)
    idx, out, cnt = np.full((nq, k), 0xFFFFFFFF, np.uint32), np.full((nq, k), 0x7FFFFFFF, np.uint32).view(F), np.zeros(nq, np.uint32)
    for i in range(nq):
        keys = np.sort((ordered(dist[i, rows.astype(np.int64)]) << np.uint64(32)) | rows, kind="stable")[:k]
        cnt[i] = keys.size
        idx[i, :keys.size] = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        out[i, :keys.size] = dist[i, idx[i, :keys.size].astype(np.int64)]
    return idx, out, cnt

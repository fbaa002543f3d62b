"""numpy statement of the expanded bracket of rerank_i8_kernel (txh_rows.hip, SCANN_HIP_RERANK_EXPAND=1, int8 rows):

    d~ = Q2 - 2 s D + s^2 N,   Q2 = |q|^2 (f32),   D = sum q x8 (f32),   N = sum x8^2 (an exact integer)
    B = (sqrt(Q2) + s sqrt(N))^2 (dim + 8) 1.2e-7          what the three terms' roundings can leave in d~
    slack = (2 sqrt(max(d~, 0) + B) E + E^2) 1.0001 + |d~| (dim + 8) 1.2e-7 + B + 1e-30

and the row families its tests run on: those of tests/helpers.py rerank_rows, and three built for the expanded form.
The model follows the kernel's f32 formulas, not its summation order (tests/rerank_filter_model.py states the
per-dimension bracket, the stores and the selection rules; they are shared).

sqrt(max(d~, 0) + B) rather than sqrt(max(d~, 0)): the triangle inequality needs the REAL d~, which the computed one
only locates to +- B."""
import numpy as np

from tests import helpers as H
from tests import rerank_filter_model as RM

F32 = np.float32
INF = F32(np.inf)
TERMS = RM.TERMS + ("cancel",)   # "cancel" = B
NEW_FAMILIES = ("cancel", "zero-query", "big-norm")
FAMILIES = tuple(H.RERANK_FAMILIES) + NEW_FAMILIES
CANCEL_OFFSET = 30.0


def expand_rows(family, n, dim, nq, seed):
    """H.rerank_rows' dict for its families; the same keys for the three families of the expanded form:

    cancel      queries on the grid {-1.75, -1.5, ..., 1.75} with one coordinate 1.75; row i = query i % nq + noise of
                2^-10; everything + 30.  |q|^2 ~ 900 dim against distances of ~ dim 2^-20 to the row's own query: the
                three terms of the expanded form cancel by seven orders of magnitude.  With the largest element
                31.75 = 127 / 4 the int8 grid of a row is the queries' grid, E ~ sqrt(dim) 2^-10, and the bracket
                would be narrower than the f32 rounding of Q2 if B were left out.
    zero-query  uniform rows; every second query is zero (Q2 = D = 0: d~ = s^2 N), the others are uniform
    big-norm    uniform rows x 2^40, uniform queries of norm 1: d~ ~ s^2 N ~ 2^80 dim / 3, Q2 = 1 vanishes in it
    """
    if family in ("overflow-all", "overflow-most") and dim * 0.36 * 4.0 ** H.RERANK_OVERFLOW_EXP <= H.FLT_MAX:
        return _overflow_rows_few_dims(family, n, dim, nq, seed)
    if family in H.RERANK_FAMILIES:
        return H.rerank_rows(family, n, dim, nq, seed)
    S = H.rerank_subspaces(dim)
    rng = np.random.default_rng([seed, 23, dim])
    cb = rng.uniform(-1.0, 1.0, (S, 16, dim // S)).astype(F32)
    base = rng.uniform(-1.0, 1.0, (n, dim)).astype(F32)
    q = rng.uniform(-1.0, 1.0, (nq, dim)).astype(F32)
    cbr = cb
    if family == "cancel":
        q = (rng.integers(-7, 8, (nq, dim)) * 0.25).astype(F32)
        q[np.arange(nq), rng.integers(0, dim, nq)] = 1.75
        base = (q[np.arange(n) % nq] + rng.uniform(-1.0, 1.0, (n, dim)) * 2.0 ** -10).astype(F32)
        off = F32(CANCEL_OFFSET)
        rows, q, cbr = base + off, q + off, cb + off
        st = RM.i8_store(rows)
        assert (st.E < F32(dim) ** F32(0.5) * F32(2.0 ** -9)).all(), "cancel: the int8 grid is not the queries' grid"
        assert float((q.astype(np.float64) ** 2).sum(1).min()) > 800.0 * dim
    elif family == "zero-query":
        rows = base
        q[::2] = 0.0
    elif family == "big-norm":
        rows = base * F32(2.0 ** 40)
        q = (q / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True)).astype(F32)
    else:
        raise ValueError(family)
    rows = np.ascontiguousarray(rows, F32)
    q = np.ascontiguousarray(q, F32)
    return dict(codebook=np.ascontiguousarray(cbr, F32), codes=H.encode_codes(cb, base), rows=rows, base=base, queries=q)


def _overflow_rows_few_dims(family, n, dim, nq, seed):
    """overflow-all / overflow-most where 2^62 does not overflow: 16 elements of 0.6 x 2^62 and more give squared
    distances under FLT_MAX.  The recipe and premises of H.rerank_rows with the next exponent."""
    S = H.rerank_subspaces(dim)
    rng = np.random.default_rng([seed, 11, dim])
    cb = rng.uniform(-1.0, 1.0, (S, 16, dim // S)).astype(F32)
    base = rng.uniform(-1.0, 1.0, (n, dim)).astype(F32)
    q = np.ascontiguousarray(rng.uniform(-1.0, 1.0, (nq, dim)), F32)
    base = (np.sign(base) * rng.uniform(0.6, 1.0, (n, dim))).astype(F32)
    rows = base * F32(2.0 ** (H.RERANK_OVERFLOW_EXP + 1))
    if family == "overflow-most":
        fin = H.overflow_finite_rows(n)
        base[fin] = rng.uniform(-0.05, 0.05, (fin.size, dim)).astype(F32)
        rows[fin] = base[fin]
    rows = np.ascontiguousarray(rows, F32)
    finite = np.isfinite(H._exact_all(rows, q))
    if family == "overflow-all":
        assert not finite.any(), "overflow-all: an exact distance is finite"
    else:
        assert (finite.sum(1) < 10).all() and (finite.sum(1) > 0).all(), finite.sum(1)
        assert np.isinf(RM.approx_distances(RM.i8_store(rows), q[0])).sum() > n // 2, "overflow-most: d~ does not overflow"
    return dict(codebook=cb, codes=H.encode_codes(cb, base), rows=rows, base=base, queries=q)


def expanded(store, q, rows_idx=None):
    """(acc, B) of the kernel's expanded form for an int8 store, in f32 (sequential sums: not the kernel's order)"""
    assert store.kind == "int8"
    codes = store.codes if rows_idx is None else store.codes[rows_idx]
    s = store.deq if rows_idx is None else store.deq[rows_idx]
    q = np.asarray(q, F32)
    dim = codes.shape[1]
    with np.errstate(all="ignore"):
        Q2 = (q * q).sum(dtype=F32)
        D = (q[None, :] * codes.astype(F32)).sum(axis=1, dtype=F32)
        N = (codes.astype(np.int64) ** 2).sum(axis=1).astype(F32)
        acc = ((Q2 - (F32(2.0) * s) * D).astype(F32) + ((s * s).astype(F32) * N).astype(F32)).astype(F32)
        rt = (np.sqrt(Q2) + (s * np.sqrt(N)).astype(F32)).astype(F32)
        B = ((rt * rt).astype(F32) * (F32(dim + 8) * F32(1.2e-7))).astype(F32)
    return acc, B


def bracket(acc, E, B, dim, terms=TERMS):
    """[L, U] in f32 from the expanded acc; the bracket is unbounded when acc or slack is NaN or infinite"""
    acc = np.asarray(acc, F32)
    E = np.broadcast_to(np.asarray(E, F32), acc.shape)
    B = np.asarray(B, F32) if "cancel" in terms else np.zeros(acc.shape, F32)
    with np.errstate(all="ignore"):
        slack = np.zeros(acc.shape, F32)
        if "error" in terms:
            root = np.sqrt((np.fmax(acc, F32(0.0)) + B).astype(F32))
            slack = ((F32(2.0) * root * E + E * E) * F32(1.0001)).astype(F32)
        if "f32sum" in terms:
            slack = (slack + np.abs(acc) * (F32(dim + 8) * F32(1.2e-7))).astype(F32)
        slack = (slack + B).astype(F32)
        if "floor" in terms:
            slack = (slack + F32(1e-30)).astype(F32)
        L = (acc - slack).astype(F32)
        U = (acc + slack).astype(F32)
    bad = np.isnan(slack) | np.isnan(acc) | ~(slack < INF) | ~(acc < INF)
    return np.where(bad, -INF, L).astype(F32), np.where(bad, INF, U).astype(F32)


def from_ordered(o):
    """inverse of common.h f32_to_ordered (RM.ordered)"""
    o = np.ascontiguousarray(o, np.uint32)
    b = np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32)
    return b.view(F32)

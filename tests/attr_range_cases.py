"""Columns, clause sets and per-query ranges shared by the range-filter tests (host and GPU): edge values on both sides
of every word and tile edge, and bounds that cycle through a point range on an edge row, an empty range, the full range,
a range across a tile edge and NaN bounds."""
import numpy as np

from tests.attr_range_model import ATTR_F32, ATTR_I64, ROW_INDEX

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
EDGE_I64 = [I64_MIN, I64_MAX, 2 ** 53, 2 ** 53 + 1, 0, -1, 1, I64_MAX - 1, I64_MIN + 1]
EDGE_F32 = [0.0, -0.0, 1e-40, -1e-40, np.inf, -np.inf, np.nan, 1.0, -1.0, 1e-41, 3.4028235e38]
# clause columns of a call: columns 0, 2..6 are i64, 1 and 7 are f32
CLAUSE_SETS = {
    "i64": [0],
    "f32": [1],
    "row": [ROW_INDEX],
    "mixed": [0, 1, ROW_INDEX],
    "eight": [0, 2, 3, 4, 5, 6, 1, ROW_INDEX],   # six i64 clauses: the register budget
    "repeat": [0, 0],
    "none": [],
}
KINDS = ("point", "empty", "full", "across", "nan")


def edge_rows(n, tile):
    """rows on both sides of every word and tile edge below n, and the last row"""
    rows = set()
    for e in (0, 64, 128, tile, 2 * tile, n):
        rows.update(r for r in (e - 2, e - 1, e, e + 1) if 0 <= r < n)
    return sorted(rows)


def make_columns(n, tile, seed=0):
    """eight columns (types as in CLAUSE_SETS): small random values, the edge values cycled over the edge rows"""
    rng = np.random.default_rng([n, seed])
    cols = []
    for c in range(8):
        if c in (1, 7):
            v = rng.uniform(-1, 1, n).astype(np.float32)
            edges = np.array(EDGE_F32, np.float32)
        else:
            v = rng.integers(-1000, 1000, n).astype(np.int64)
            edges = np.array(EDGE_I64, np.int64)
        for i, r in enumerate(edge_rows(n, tile)):
            v[r] = edges[(i + c) % edges.size]
        cols.append(v)
    return cols


def column_type(col):
    return 0 if col == ROW_INDEX else (ATTR_F32 if col in (1, 7) else ATTR_I64)


def point_row(n, tile, columns):
    """an edge row (the first of a tile where there is one) whose f32 values are not NaN"""
    for r in (tile, tile - 1, 64, 63, n - 1, 0) + tuple(range(n)):
        if 0 <= r < n and not np.isnan(columns[1][r]) and not np.isnan(columns[7][r]):
            return r
    raise AssertionError("every row holds a NaN")


def make_bounds(n, tile, columns, cols, nq, shift=0):
    """(lo, hi, kinds): lo[q][c] / hi[q][c] as Python / numpy scalars; query q is of kind KINDS[(q + shift) % 5]"""
    pr = point_row(n, tile, columns)
    lo, hi, kinds = [], [], []
    for q in range(nq):
        kind = KINDS[(q + shift) % len(KINDS)]
        ql, qh = [], []
        for c, col in enumerate(cols):
            t = column_type(col)
            full = (-np.inf, np.inf) if t == ATTR_F32 else (I64_MIN, I64_MAX)
            if kind == "point":
                v = pr if col == ROW_INDEX else columns[col][pr]
                b = (v, v)
            elif kind == "empty":
                b = ((5, 4) if t != ATTR_F32 else (0.5, 0.25)) if c == 0 else full
            elif kind == "full":
                b = full
            elif kind == "across":
                if col == ROW_INDEX:
                    b = (tile - 3, tile + 3) if n > tile else (max(n - 3, 0), n + 3)
                else:
                    b = (-0.5, 0.75) if t == ATTR_F32 else (-500, 700)
            else:   # NaN bounds on the f32 clauses (lo for even clauses, hi for odd ones); the others full
                b = ((np.nan, np.inf) if c % 2 == 0 else (-np.inf, np.nan)) if t == ATTR_F32 else full
            ql.append(b[0])
            qh.append(b[1])
        lo.append(ql)
        hi.append(qh)
        kinds.append(kind)
    return lo, hi, kinds


def pack_bounds(hip, cols, lo, hi):
    """hip._range_bounds over the per-query lists of make_bounds: [nq, n_cols, 2] words"""
    nq = len(lo)
    types = [column_type(c) for c in cols]
    per = lambda x, c: np.array([x[q][c] for q in range(nq)], np.float32 if types[c] == ATTR_F32 else np.int64)
    b = hip._range_bounds(types, [per(lo, c) for c in range(len(cols))], [per(hi, c) for c in range(len(cols))])
    return b if len(cols) else np.zeros((nq, 0, 2), np.uint64)


def popcount(words):
    return sum(bin(int(w)).count("1") for w in np.asarray(words).ravel())

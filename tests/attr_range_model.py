"""A plain numpy model of the range filters' semantics: bit j of query q's bitmap is the AND over the call's clauses of
lo <= value(cols[c], j) <= hi, both bounds inclusive.  i64 columns compare as numpy int64 (signed, exact), f32 columns
as numpy float32 (IEEE: -0.0 == 0.0, denormals as stored, a NaN on either side false), the row-index pseudo-column has
the value j.  One boolean expression per clause; nothing here is shared with the library's host form."""
import numpy as np

ATTR_I64, ATTR_F32, ROW_INDEX = 1, 2, 0xFFFFFFFF
AND, OR, ANDNOT = 1, 2, 3


def clause_mask(n, columns, col, lo, hi):
    """bool[n]: rows whose value of clause column `col` lies in [lo, hi]; lo / hi are Python or numpy scalars"""
    if col == ROW_INDEX:
        v = np.arange(n, dtype=np.int64)
        return (np.int64(lo) <= v) & (v <= np.int64(hi))
    v = np.asarray(columns[col])
    if v.dtype == np.int64:
        return (np.int64(lo) <= v) & (v <= np.int64(hi))
    assert v.dtype == np.float32
    with np.errstate(invalid="ignore"):
        return (np.float32(lo) <= v) & (v <= np.float32(hi))


def pack(mask, stride=None):
    """uint64 words of a bool[n] mask, bit j of word j // 64 for row j, zero-padded to `stride` words"""
    n = mask.size
    words = -(-n // 64)
    bits = np.zeros(words * 64, np.uint8)
    bits[:n] = mask
    w = np.packbits(bits.reshape(words, 64), axis=1, bitorder="little").view("<u8").ravel().astype(np.uint64)
    out = np.zeros(words if stride is None else stride, np.uint64)
    out[:words] = w
    return out


def allow_bitmaps(n, columns, cols, lo, hi, stride=None, op=0, out=None):
    """[nq, stride] block.  lo[q][c] / hi[q][c]: the bounds of query q's clause c.  op 0 returns a fresh block with zero
    gap words; AND / OR / ANDNOT return a copy of `out` with words [0, ceil(n / 64)) of each row combined and every
    other word as it was."""
    nq = len(lo)
    words = -(-n // 64)
    stride = words if stride is None else stride
    res = np.zeros((nq, stride), np.uint64) if op == 0 else np.array(out, np.uint64, copy=True)
    for q in range(nq):
        m = np.ones(n, bool)
        for c, col in enumerate(cols):
            m &= clause_mask(n, columns, col, lo[q][c], hi[q][c])
        w = pack(m)
        if op == 0:
            res[q, :words] = w
        elif op == AND:
            res[q, :words] &= w
        elif op == OR:
            res[q, :words] |= w
        elif op == ANDNOT:
            res[q, :words] &= ~w
        else:
            raise ValueError("op")
    return res


def range_filter_is_allowed(start, end, index):
    """RangeFilter::is_allowed (restricts/mod.rs:88-90), restated"""
    return index >= start and index < end


def range_filter_bitmap(n, start, end, stride=None):
    return pack(np.array([range_filter_is_allowed(start, end, j) for j in range(n)], bool), stride)

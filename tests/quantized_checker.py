"""numpy statement of the reference's asymmetric one-to-many kernels over quantized rows
(distance_measures/one_to_many_asymmetric.rs), the checker of tests/test_gpu_quantized_bf.py.

* bf16 / FP8 E4M3 rows: one sequential float32 sum per (query, row), `sum = sum + q*x` or
  `d = q - x; sum = sum + d*d` (:267-377).  numpy rounds every float32 operation and never fuses.
* int8 rows: the AVX2 form (:78-142, :208-257) is the f32 AVX2 arithmetic of the oracle's
  or_one_to_many_* applied to x = float32(i8) * inv_multiplier (one rounded product), so the checker
  is orc.one_to_many on the dequantized rows.
"""
import numpy as np

SQUARED_L2, L2, DOT_PRODUCT = 0, 1, 2
ROWS_BF16, ROWS_FP8_E4M3, ROWS_INT8 = 1, 2, 3


def bf16_from_f32(values):
    """half::bf16::from_f32: NaN -> (bits >> 16) | 0x40, else round to nearest even on bit 15."""
    x = np.ascontiguousarray(values, np.float32).view(np.uint32)
    hi = (x >> np.uint32(16)).astype(np.uint32)
    nan = (x & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    up = ((x & np.uint32(0x8000)) != 0) & ((x & np.uint32(0x17FFF)) != 0)
    out = np.where(nan, hi | np.uint32(0x40), hi + up.astype(np.uint32))
    return out.astype(np.uint16)


def bf16_to_f32(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def _e4m3_table():
    out = np.zeros(256, np.float32)
    for b in range(256):
        e, m = (b >> 3) & 15, b & 7
        if e == 0 and m == 0:
            v = 0.0
        else:
            v = (1.0 + m / 8.0) * 2.0 ** ((e if e else -1) - 7)   # exponent field 0: 2^-8 * (1 + m/8)
        out[b] = -v if b & 0x80 else v
    return out


E4M3 = _e4m3_table()


def e4m3_to_f32(codes):
    return E4M3[np.asarray(codes, np.uint8)]


def decode(rows, fmt, inv_multiplier=1.0):
    """Row elements as the reference's kernels see them (float32)."""
    if fmt == ROWS_BF16:
        return bf16_to_f32(rows)
    if fmt == ROWS_FP8_E4M3:
        return e4m3_to_f32(rows)
    return np.asarray(rows).view(np.int8).astype(np.float32) * np.float32(inv_multiplier)


def sequential(queries, x, measure):
    """[nq][n] distances of the sequential loops: queries [nq][dim] f32, x [n][dim] decoded rows."""
    q = np.ascontiguousarray(queries, np.float32)
    xt = np.ascontiguousarray(np.asarray(x, np.float32).T)   # [dim][n]: one contiguous column per step
    s = np.zeros((q.shape[0], xt.shape[1]), np.float32)
    with np.errstate(all="ignore"):
        for j in range(q.shape[1]):
            if measure == DOT_PRODUCT:
                s = s + q[:, j, None] * xt[None, j]
            else:
                d = q[:, j, None] - xt[None, j]
                s = s + d * d
        if measure == DOT_PRODUCT:
            return -s
        return np.sqrt(s) if measure == L2 else s


def distances(queries, rows, dim, fmt, measure, inv_multiplier=1.0):
    """Checker distances [nq][n] for rows [n][stride] of the given format (first dim columns used)."""
    x = decode(np.asarray(rows)[:, :dim], fmt, inv_multiplier)
    q = np.ascontiguousarray(np.asarray(queries, np.float32)[:, :dim])
    if fmt != ROWS_INT8:
        return sequential(q, x, measure)
    from oracle import pyoracle as orc
    n = x.shape[0]
    out = np.zeros((q.shape[0], n), np.float32)
    for i in range(q.shape[0]):
        out[i] = orc.one_to_many(q[i], np.ascontiguousarray(x), dim, n, measure)
    return out

"""Pins tests/quantized_checker.py, the checker of the quantized brute-force GPU tests, with the reference's
own known answers (distance_measures/one_to_many_asymmetric.rs:411-520, values copied) and against the
oracle.  CPU only."""
import numpy as np

from oracle import pyoracle as orc
from tests import quantized_checker as qc


def _q8():
    return np.array([[1, 2, 3, 4, 5, 6, 7, 8]], np.float32)


def test_int8_dot_product():  # one_to_many_asymmetric.rs:411-430
    db = np.array([[127] * 8, [0] * 8], np.int8)
    d = qc.distances(_q8(), db, 8, qc.ROWS_INT8, qc.DOT_PRODUCT, np.float32(1.0) / np.float32(127.0))[0]
    assert abs(d[0] - -36.0) < 1e-3 and abs(d[1]) < 1e-3


def test_int8_squared_l2():  # :432-450
    db = np.array([[127] * 8, [0] * 8], np.int8)
    d = qc.distances(_q8(), db, 8, qc.ROWS_INT8, qc.SQUARED_L2, np.float32(1.0) / np.float32(127.0))[0]
    assert abs(d[1] - 204.0) < 0.5


def test_bf16_dot_product():  # :452-466
    q = np.array([[1, 2, 3, 4]], np.float32)
    db = qc.bf16_from_f32(np.array([[1, 1, 1, 1], [2, 2, 2, 2]], np.float32))
    d = qc.distances(q, db, 4, qc.ROWS_BF16, qc.DOT_PRODUCT)[0]
    assert d[0] == -10.0 and d[1] == -20.0


def test_bf16_squared_l2():  # :468-482
    q = np.array([[1, 2, 3, 4]], np.float32)
    db = qc.bf16_from_f32(np.array([[1, 2, 3, 4], [2, 3, 4, 5]], np.float32))
    d = qc.distances(q, db, 4, qc.ROWS_BF16, qc.SQUARED_L2)[0]
    assert d[0] == 0.0 and d[1] == 4.0


def test_avx2_vs_portable_int8_data():  # :484-520: dim 128, 50 points, (i % 128) - 64, inv_multiplier 1/64
    """The int8 checker is the f32 AVX2 order of or_one_to_many_* on the dequantized rows.  Reading both: the
    reference's one_to_many_int8_float_*_avx2 keeps one __m256 of 8 lane chains, fmadd(q, x, acc) (dot) or
    d = q - x, fmadd(d, d, acc) over full chunks of 8, reduces with horizontal_sum_avx (lo + hi, hadd, hadd =
    (t0+t1)+(t2+t3)) and adds an unfused scalar tail; the oracle's or_dot_product_avx2 / or_squared_l2_avx2 do
    the same operations in the same order (hsum256 gives the same (t0+t1)+(t2+t3)).  Here: within the
    reference's own tolerance of the portable loop, and bitwise equal to a numpy restatement of the 8 chains.
    The restatement forms each fma as float64 product (exact for two float32) + float64 sum, rounded to float32:
    one rounding only where the float64 sum is exact, which a TwoSum error term of zero proves for every step
    of this data (asserted), so there it is fmaf."""
    dim, n = 128, 50
    inv = np.float32(1.0) / np.float32(64.0)
    q = (np.arange(dim, dtype=np.float32) * np.float32(0.1))[None]
    db = ((np.arange(n * dim) % 128) - 64).astype(np.int8).reshape(n, dim)
    x = db.astype(np.float32) * inv
    for measure in (qc.DOT_PRODUCT, qc.SQUARED_L2):
        got = qc.distances(q, db, dim, qc.ROWS_INT8, measure, inv)[0]
        portable = qc.sequential(q, x, measure)[0]
        assert np.all(np.abs(got - portable) < 0.1)
        # 8 lane chains with a single rounding per fma (float64 holds every product of two float32 exactly)
        acc = np.zeros((n, 8), np.float32)

        def fma_f32(prod, a):
            a = a.astype(np.float64)
            s = prod + a
            bb = s - prod
            err = (prod - (s - bb)) + (a - bb)   # TwoSum: the rounding error of the float64 sum
            assert np.all(err == 0.0)
            return s.astype(np.float32)
        for c in range(dim // 8):
            qa = q[0, 8 * c:8 * c + 8].astype(np.float64)
            xa = x[:, 8 * c:8 * c + 8].astype(np.float64)
            if measure == qc.DOT_PRODUCT:
                acc = fma_f32(qa * xa, acc)
            else:
                d = (q[0, 8 * c:8 * c + 8] - x[:, 8 * c:8 * c + 8]).astype(np.float64)
                acc = fma_f32(d * d, acc)
        s = [acc[:, j] + acc[:, j + 4] for j in range(4)]
        r = (s[0] + s[1]) + (s[2] + s[3])
        if measure == qc.DOT_PRODUCT:
            r = -r
        assert np.array_equal(got.view(np.uint32), r.view(np.uint32))


def test_bf16_from_f32_edges():
    """half::bf16::from_f32: round to nearest even, signed zeros, subnormals, the largest finite values,
    infinities and NaN payloads."""
    cases = {
        0x3F808000: 0x3F80,   # tie, even lsb: down
        0x3F818000: 0x3F82,   # tie, odd lsb: up
        0x3F808001: 0x3F81,   # above the tie: up
        0x3F807FFF: 0x3F80,   # below the tie: down
        0x00000000: 0x0000, 0x80000000: 0x8000,
        0x00000001: 0x0000, 0x00008001: 0x0001, 0x00018000: 0x0002, 0x807FFFFF: 0x8080,
        0x7F7F0000: 0x7F7F, 0x7F7F7FFF: 0x7F7F, 0x7F7FFFFF: 0x7F80, 0xFF7FFFFF: 0xFF80,
        0x7F800000: 0x7F80, 0xFF800000: 0xFF80,
        0x7FC00000: 0x7FC0, 0x7F800001: 0x7FC0, 0xFF812345: 0xFFC1, 0x7FBFFFFF: 0x7FFF,
    }
    x = np.array(list(cases), np.uint32).view(np.float32)
    got = qc.bf16_from_f32(x)
    assert [int(v) for v in got] == list(cases.values())
    # to_f32 is exact: a round trip of bf16-representable values is the identity
    b = np.arange(0, 65536, 257, dtype=np.uint16)
    fin = np.isfinite(qc.bf16_to_f32(b))
    assert np.array_equal(qc.bf16_from_f32(qc.bf16_to_f32(b))[fin], b[fin])


def test_e4m3_checker_matches_oracle_codec():
    """All 256 codes: the checker's table is the oracle's to_f32_e4m3 (quantization/fp8.rs), which is not OCP
    e4m3fn (exponent field 0 -> 2^-8 * (1 + m/8); 0x7F / 0xFF -> +-480)."""
    for b in range(256):
        assert qc.E4M3[b].view(np.uint32) == orc.fp8_to_f32(b).view(np.uint32), b
    assert qc.E4M3[0x7F] == 480.0 and qc.E4M3[0xFF] == -480.0 and qc.E4M3[0x01] == np.float32(2.0 ** -8 * 1.125)


def test_fp8_checker_matches_oracle_one_to_many():
    rng = np.random.default_rng(5)
    for dim in (1, 7, 9, 50, 128):
        n = 40
        db = rng.integers(0, 256, size=(n, dim + 3), dtype=np.uint8)
        q = rng.uniform(-2, 2, size=(2, dim)).astype(np.float32)
        for measure in (qc.SQUARED_L2, qc.DOT_PRODUCT):
            got = qc.distances(q, db, dim, qc.ROWS_FP8_E4M3, measure)
            for i in range(2):
                want = orc.one_to_many_fp8(q[i], db, dim + 3, n, measure)
                assert np.array_equal(got[i].view(np.uint32), want.view(np.uint32))


def _bf16_split(v):
    """round-to-nearest-even bf16 of float32 values, as float32"""
    return qc.bf16_to_f32(qc.bf16_from_f32(v))


def test_shortlist_error_bound_per_format():
    """The quantized shortlist's bound (bf.hip shortlist_quant_err): the row operand is exact in bf16 (checked:
    every decoded value survives the bf16 round trip; INT8 the code itself), the query is split into qh + ql, and
    |exact - (x.qh + x.ql)| <= E |q||x| with E = 1.01 (1.1 2^-16 + (3 dim + 64) 2^-23 [+ 2^-23 for INT8]).  Rows
    span e^-6 .. e^6; the MFMA's sum is taken in float64 here (its f32 rounding is inside the accumulation term).
    Reports the largest observed fraction of E."""
    rng = np.random.default_rng(3)
    dim, n = 128, 3000
    x = (rng.standard_normal((n, dim)) * np.exp(rng.uniform(-6, 6, (n, 1)))).astype(np.float32)
    q = (rng.standard_normal((6, dim)) * 10).astype(np.float32)
    qh = _bf16_split(q)
    ql = _bf16_split(q - qh)
    worst = 0.0
    for fmt in (qc.ROWS_BF16, qc.ROWS_FP8_E4M3, qc.ROWS_INT8):
        if fmt == qc.ROWS_BF16:
            rows, inv = qc.bf16_from_f32(x), 1.0
        elif fmt == qc.ROWS_FP8_E4M3:
            rows, inv = orc.fp8_quantize(x / np.float32(np.abs(x).max()) * np.float32(400)), 1.0
        else:
            s = np.float32(np.abs(x).max() / 127)
            rows, inv = np.clip(np.rint(x / s), -127, 127).astype(np.int8), float(s)
        xv = qc.decode(rows, fmt, inv)
        operand = rows.astype(np.float32) if fmt == qc.ROWS_INT8 else xv
        assert np.array_equal(_bf16_split(operand).view(np.uint32), operand.view(np.uint32))   # exact in bf16
        E = 1.01 * (1.1 / 65536 + (3 * dim + 64) / 2.0 ** 23 + (2.0 ** -23 if fmt == qc.ROWS_INT8 else 0.0))
        exact = -qc.distances(q, rows, dim, fmt, qc.DOT_PRODUCT, inv)   # q.x in the reference's arithmetic
        approx = (qh.astype(np.float64) @ operand.T.astype(np.float64) +
                  ql.astype(np.float64) @ operand.T.astype(np.float64))
        if fmt == qc.ROWS_INT8:
            approx = approx * inv
        scale = np.linalg.norm(q.astype(np.float64), axis=1)[:, None] * np.linalg.norm(xv.astype(np.float64), axis=1)[None]
        live = scale > 0
        ratio = np.abs(exact.astype(np.float64) - approx)[live] / (E * scale[live])
        assert ratio.max() <= 1.0, (fmt, ratio.max())
        worst = max(worst, float(ratio.max()))
    print("largest |exact - approx| / (E |q||x|): %.3g" % worst)

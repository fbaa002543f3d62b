"""Packed int4 rows on the host: the pack / unpack helpers against the reference's own vector, and a numpy model of
the integer shortlist pass (bf_int.hip: int8 digit planes of the query, exact integer sums, one f32 recombination)
held to its bound shortlist_int_err."""
import numpy as np
import pytest

from scann_rust_amd import hip


def test_pack_unpack_reference_vector():
    codes = np.array([-7, 3, 0, 7, -8, 5], np.int8)   # quantization/scalar.rs: Int4PackedData's own test
    packed = hip.pack_int4(codes)
    assert packed.dtype == np.uint8 and packed.tolist() == [0xB1, 0xF8, 0xD0]
    assert np.array_equal(hip.unpack_int4(packed, 6), codes)
    odd = np.array([[7, -8, 1], [-1, 0, -8]], np.int8)
    p = hip.pack_int4(odd)
    assert p.shape == (2, 2) and (p[:, 1] >> 4).tolist() == [0, 0]   # from_int8 leaves the odd byte's high nibble 0
    assert np.array_equal(hip.unpack_int4(p, 3), odd)


def int_err(dim, digits):
    """shortlist_int_err of bf_int.hip"""
    delta = 254.0 ** -digits if digits else 0.0
    return 1.01 * (delta * np.sqrt(dim) + (dim + 64 + 4 + 1) / 8388608.0)


def digit_scores(q, codes, inv, digits):
    """bf_int_q_prep_kernel + bf_i8mfma_kernel: f64 digit split, integer sums, f32 weights and recombination."""
    qmax = np.abs(q).max(axis=1).astype(np.float64)
    s = np.where(qmax > 0, qmax / 127.0, 1.0 / 127.0)
    r = q.astype(np.float64)
    score = None
    for t in range(digits):
        d = np.rint(r / s[:, None])
        assert np.abs(d).max() <= 127
        r = r - d * s[:, None]
        w = (s * np.float64(inv)).astype(np.float32)
        acc = d.astype(np.int64) @ codes.astype(np.int64).T
        assert np.abs(acc).max() < 2 ** 24
        term = acc.astype(np.float32) * w[:, None]
        score = term if score is None else score + term
        s = s / 254.0
    return score, np.sqrt((r * r).sum(axis=1))


@pytest.mark.parametrize("dim", [128, 256])
@pytest.mark.parametrize("digits", [2, 3])
def test_digit_split_bound(dim, digits):
    rng = np.random.default_rng(dim + digits)
    codes = rng.integers(-8, 8, size=(400, dim)).astype(np.int8)
    codes[0], codes[1] = -8, 7
    inv = np.float32(0.0371)
    q = (np.exp(rng.uniform(-6, 6, size=(64, dim))) * rng.choice([-1.0, 1.0], size=(64, dim))).astype(np.float32)
    x = codes.astype(np.float32) * inv                         # the element the reference reads
    exact = q.astype(np.float64) @ x.astype(np.float64).T
    approx, e2 = digit_scores(q, codes, inv, digits)
    scale = np.linalg.norm(q.astype(np.float64), axis=1)[:, None] * np.linalg.norm(x.astype(np.float64), axis=1)[None]
    frac = np.abs(exact - approx.astype(np.float64)) / scale
    print("dim %d D %d: worst |exact - approx| / (|q||x|) = %.3g = %.3f of E" %
          (dim, digits, frac.max(), frac.max() / int_err(dim, digits)))
    assert frac.max() < int_err(dim, digits)
    # the form the pass uses: the residual's own 2-norm per query instead of delta sqrt(dim) |q|
    per_query = int_err(dim, 0) * scale + e2[:, None] * np.linalg.norm(x.astype(np.float64), axis=1)[None]
    assert (np.abs(exact - approx.astype(np.float64)) < per_query).all()

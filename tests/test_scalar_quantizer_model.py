"""The numpy model of the scalar quantizer (tests/scalar_quantizer_model.py) against the reference's own unit tests
(quantization/mod.rs:150-163, quantization/scalar.rs:411-454), and the device's summation order against the
reference's sequential order on every input the GPU parity tests use."""
import numpy as np
import pytest

from tests import scalar_quantizer_cases as SC
from tests import scalar_quantizer_model as M


def bits_of(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_stats_known_answer():
    st = M.stats_reference([[1, 2, 3], [4, 5, 6]])
    assert st[0] == 1.0 and st[1] == 6.0
    assert abs(st[2] - 3.5) < 0.01
    assert np.array_equal(bits_of(st), bits_of(M.stats_device([[1, 2, 3], [4, 5, 6]])))
    # sample variance of 1..6 is 3.5
    assert abs(float(st[3]) - np.sqrt(3.5)) < 1e-6


def test_stats_edges():
    one = M.stats_device([[7.0]])
    assert list(one) == [7.0, 7.0, 7.0, 0.0]                      # count == 1: variance 0
    nan = M.stats_device([[np.nan, 2.0, -3.0]])
    assert nan[0] == -3.0 and nan[1] == 2.0 and np.isnan(nan[2])   # min / max ignore a NaN, the sums do not
    allnan = M.stats_reference([[np.nan]])
    assert allnan[0] == M.F32_MAX and allnan[1] == -M.F32_MAX


def test_calibrate_known_answer():
    # scalar.rs test_scalar_quantizer_int8: stats {-1, 1, 0, 0.5}, the default config clips at 3 sigma = 1.5 -> [-1, 1]
    params, zp = M.calibrate([-1.0, 1.0, 0.0, 0.5])
    assert params[0] == -1.0 and params[1] == 1.0
    assert params[2] == np.float32(2.0) / np.float32(255.0) and params[3] == np.float32(255.0) / np.float32(2.0)
    assert zp == 128
    back = M.dequantize(M.quantize([0.5], params), params)
    assert abs(float(back[0]) - 0.5) < 0.02
    for v in (-1.0, 0.0, 1.0):
        assert abs(float(M.dequantize(M.quantize([v], params), params)[0]) - v) < 0.02


def test_dataset_known_answer():
    # scalar.rs test_quantized_dataset: the values span [-1, 6]; row 1 comes back within 1.0
    rows = np.array([[1, 2, 3], [4, 5, 6], [-1, 0, 1]], np.float32)
    codes, params, _ = M.rows_int8(rows, 3)
    assert params[0] == -1.0 and params[1] == 6.0      # 3 sigma reaches past both ends: the range is [min, max]
    assert np.abs(M.dequantize(codes[1], params) - rows[1]).max() < 1.0
    assert np.array_equal(codes, M.rows_int8(rows, 3, stats=M.stats_reference(rows))[0])


def test_int4_and_constant():
    params, zp = M.calibrate([-1.0, 1.0, 0.0, 0.5], bits=4)
    assert params[2] == np.float32(2.0) / np.float32(15.0)
    assert M.quantize([5.0], params, bits=4)[0] == 15
    params, zp = M.calibrate(M.stats_device(np.full((4, 3), 2.5, np.float32)))
    assert list(params) == [2.5, 2.5, 1.0, 1.0] and zp == 0       # range <= 1e-10
    assert M.calibrate([0, 1, 0, 1], 8, M.SQ_RANGE, 2.0, 1.0) is None      # min > max
    assert M.calibrate([0, 1, 0, 1], 8, M.SQ_RANGE, np.nan, 1.0) is None   # a NaN bound
    assert M.calibrate([0, 1, 0, 1], 5) is None


def test_wrap_and_rounding():
    p = np.array([0.0, 255.0, 1.0, 1.0], np.float32)
    v = np.array([126.5, 127.0, 127.5, 128.0, 254.5, 255.0, 300.0, -1.0, 0.5, 1.5, 2.5, np.nan, -0.0], np.float32)
    # half away from zero; 128 .. 255 wrap to -128 .. -1
    assert list(M.quantize(v, p)) == [127, 127, -128, -128, -1, -1, -1, 0, 1, 2, 3, 0, 0]
    assert list(M.dequantize(np.array([127, -128, -1], np.int8), p)) == [127.0, 128.0, 255.0]
    s = np.array([-127.0, 127.0, 1.0, 1.0], np.float32)
    v = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 126.5, 200.0, -200.0], np.float32)
    assert list(M.quantize(v, s, mode=M.SQ_SIGNED)) == [0, 2, 2, 0, -2, 126, 127, -127]   # half to even


def test_signed_is_symmetric_int8():
    from scann_rust_amd import hip
    for name, rows in SC.parity_cases():
        codes, inv = hip.symmetric_int8(rows)
        got, params, zp = M.rows_int8(rows, rows.shape[1], mode=M.SQ_SIGNED)
        assert np.array_equal(got, codes), name
        assert np.float32(inv) == params[2] and zp == 0, name


@pytest.mark.parametrize("name,rows", SC.parity_cases(), ids=[n for n, _ in SC.parity_cases()])
def test_device_order_equals_reference_order(name, rows):
    """all four statistics bit-equal between the device's summation order and the reference's sequential one"""
    ref, dev = M.stats_reference(rows), M.stats_device(rows)
    assert np.array_equal(bits_of(ref), bits_of(dev)), (name, ref, dev)


def test_cancellation_is_the_documented_exception():
    """100 + 0.01 U at 3000 x 24: the two orders' f64 sums differ in their last bits, and sum_sq - sum^2 / count
    cancels ~13 digits, so those bits reach the f32 std_dev.  min, max and mean still agree; the parity claim of
    DESIGN.md 7 excludes such data."""
    rows = SC.cancellation_rows()
    ref, dev = M.stats_reference(rows), M.stats_device(rows)
    assert np.array_equal(bits_of(ref[:3]), bits_of(dev[:3]))
    s_ref, s2_ref = M.sums_sequential(rows)
    s_dev, s2_dev = M.sums_device(rows)
    assert (s_ref, s2_ref) != (s_dev, s2_dev)
    assert ref[3] != dev[3]
    rel = abs(float(ref[3]) - float(dev[3])) / float(ref[3])
    print("std_dev reference order %r, device order %r, relative difference %.3g" % (ref[3], dev[3], rel))
    assert rel < 1e-2     # both are still estimates of the true 0.00289; neither is "the" value

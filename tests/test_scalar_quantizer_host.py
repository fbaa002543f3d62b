"""The scalar quantizer, the parts that need no GPU: the six symbols (exported, bound, declared),
the stateless host functions scann_hip_scalar_quantizer_calibrate / _quantize / _dequantize bit for bit against the
numpy model (tests/scalar_quantizer_model.py) in all four modes and both bit widths, SQ_SIGNED against
hip.symmetric_int8, refusals that leave the outputs untouched, and the program scalar_quantizer_test."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import scalar_quantizer_cases as SC
from tests import scalar_quantizer_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "scann_rust_amd", "host", "scalar_quantizer_test")
SYMBOLS = ("scann_hip_index_quantization_stats", "scann_hip_scalar_quantizer_calibrate", "scann_hip_scalar_quantize",
           "scann_hip_scalar_dequantize", "scann_hip_scalar_quantize_device", "scann_hip_index_quantize_rows")
MODES = (M.SQ_STDDEV, M.SQ_SYMMETRIC, M.SQ_RANGE, M.SQ_SIGNED)
# stats [min, max, mean, std_dev]: the reference's test, a clipped range, an asymmetric one, a constant dataset,
# a huge one, a subnormal one
STATS = [(-1.0, 1.0, 0.0, 0.5), (-4.0, 9.0, 1.0, 1.0), (0.25, 7.75, 3.0, 10.0), (2.5, 2.5, 2.5, 0.0),
         (-3.0e38, 3.0e38, 0.0, 1.0e38), (-1e-40, 1e-40, 0.0, 1e-41), (0.0, 255.0, 127.5, 74.0)]
RANGES = [(0.0, 255.0), (0.0, 15.0), (-128.0, 127.0), (-1.0, 1.0), (-1.0, 6.0), (3.0, 3.0), (-0.1, 0.7)]


def _hip():
    from scann_rust_amd import build, hip
    build.build()
    return hip


def bits_of(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_symbols_exported_bound_declared_documented():
    hip = _hip()
    lib = ctypes.CDLL(hip.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scann_hip.h")).read(), flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    L = hip.load()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in hip.EXPORTS
        assert getattr(L, name).argtypes is not None, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert re.search(r"\bfn %s\s*\(" % name, doc), "INTEGRATION.md lacks " + name
        assert not name.startswith("scann_hip_mutable_")
    for i, mode in enumerate(("STDDEV", "SYMMETRIC", "RANGE", "SIGNED")):
        assert int(re.search(r"#define SCANN_HIP_SQ_%s (\d+)" % mode, header).group(1)) == i == getattr(hip, "SQ_" + mode)
    assert len(hip.abi_layout()) == 6                          # no new struct
    assert callable(hip.quantization_stats) and callable(hip.scalar_quantize_device) and callable(hip.Index.quantize_rows)
    from scann_rust_amd import build
    assert "scalarq.hip" in build.SOURCES and "scalarq.h" in build.HEADERS and "scalar_quantizer_test" in build.HOST_PROGRAMS


def _calibrate(hip, stats, bits, mode, a, b):
    """(status, params, zero_point) with sentinel-filled outputs"""
    st = np.asarray(stats, np.float32)
    params = np.full(4, -77.0, np.float32)
    zp = ctypes.c_int32(-77)
    s = hip.load().scann_hip_scalar_quantizer_calibrate(hip.ptr(st, hip.f32p), bits, mode, ctypes.c_float(a), ctypes.c_float(b),
                                                       hip.ptr(params, hip.f32p), ctypes.byref(zp))
    return s, params, zp.value


def _configs():
    for bits in (4, 8):
        for mode in MODES:
            for stats in STATS:
                for a, b in (RANGES if mode == M.SQ_RANGE else [(3.0, 0.0), (0.5, 0.0)] if mode == M.SQ_STDDEV else [(0.0, 0.0)]):
                    yield bits, mode, stats, a, b


def test_calibrate_matches_the_model():
    hip = _hip()
    seen = set()
    for bits, mode, stats, a, b in _configs():
        want = M.calibrate(stats, bits, mode, a, b)
        s, params, zp = _calibrate(hip, stats, bits, mode, a, b)
        if want is None:
            assert s == hip.INVALID_ARGUMENT, (bits, mode, stats, a, b)
            assert (params == -77.0).all() and zp == -77            # untouched
            seen.add("refused")
            continue
        assert s == hip.OK, (bits, mode, stats, a, b, hip.load().scann_hip_last_error())
        assert np.array_equal(bits_of(params), bits_of(want[0])), (bits, mode, stats, a, b, params, want[0])
        assert zp == want[1]
        seen.add("constant" if params[2] == 1.0 and params[3] == 1.0 and params[0] == params[1] else "ok")
    assert seen == {"refused", "constant", "ok"}
    # refusals of their own: bad bits, bad mode, min > max, a NaN bound, non-finite stats in the signed mode
    for bits, mode, stats, a, b in [(5, 0, STATS[0], 3, 0), (8, 4, STATS[0], 3, 0), (8, -1, STATS[0], 3, 0),
                                    (8, M.SQ_RANGE, STATS[0], 2.0, 1.0), (8, M.SQ_RANGE, STATS[0], np.nan, 1.0),
                                    (8, M.SQ_RANGE, STATS[0], 0.0, np.nan), (4, M.SQ_SIGNED, STATS[0], 0, 0),
                                    (8, M.SQ_SIGNED, (-np.inf, 1, 0, 1), 0, 0), (8, M.SQ_SIGNED, (-1, 1, np.nan, 1), 0, 0),
                                    (8, M.SQ_STDDEV, (np.nan, np.nan, np.nan, np.nan), 3, 0)]:
        s, params, zp = _calibrate(hip, stats, bits, mode, a, b)
        assert s == hip.INVALID_ARGUMENT, (bits, mode, stats, a, b)
        assert (params == -77.0).all() and zp == -77
    L = hip.load()
    assert L.scann_hip_scalar_quantizer_calibrate(None, 8, 0, 3.0, 0.0, None, None) == hip.INVALID_ARGUMENT


def test_quantize_and_dequantize_match_the_model():
    hip = _hip()
    L = hip.load()
    rng = np.random.default_rng(5)
    checked = 0
    for bits, mode, stats, a, b in _configs():
        want = M.calibrate(stats, bits, mode, a, b)
        if want is None:
            continue
        params = want[0]
        with np.errstate(over="ignore"):
            vals = np.concatenate([SC.adversarial_values(params, bits if mode != M.SQ_SIGNED else 8),
                                   (rng.standard_normal(64) * max(abs(stats[0]), abs(stats[1]), 1e-3)).astype(np.float32)])
        if mode == M.SQ_SIGNED:
            vals = vals[np.isfinite(vals)]
            k = np.arange(-130, 131, dtype=np.float32)
            with np.errstate(all="ignore"):   # x / s = k + 0.5 where the product is exact: ties go to even
                vals = np.concatenate([vals, ((k + np.float32(0.5)) * params[2]).astype(np.float32)])
        out = np.full(vals.size + 8, 99, np.int8)
        assert L.scann_hip_scalar_quantize(hip.ptr(vals, hip.f32p), vals.size, bits, mode, hip.ptr(params, hip.f32p),
                                           hip.ptr(out, hip.i8p)) == hip.OK
        model = M.quantize(vals, params, bits, mode)
        assert np.array_equal(out[:vals.size], model), (bits, mode, stats, a, b, vals[out[:vals.size] != model])
        assert (out[vals.size:] == 99).all()
        codes = np.arange(-128, 128, dtype=np.int8)
        back = np.full(256 + 4, -77.0, np.float32)
        assert L.scann_hip_scalar_dequantize(hip.ptr(codes, hip.i8p), 256, mode, hip.ptr(params, hip.f32p),
                                             hip.ptr(back, hip.f32p)) == hip.OK
        assert np.array_equal(bits_of(back[:256]), bits_of(M.dequantize(codes, params, mode)))
        assert (back[256:] == -77.0).all()
        checked += 1
    assert checked > 40


def test_exact_halves_and_the_wrap():
    hip = _hip()
    q = hip.ScalarQuantizer(bits=8, mode=hip.SQ_RANGE, value_range=(0.0, 255.0))
    assert q.calibrate([0, 1, 0, 1]) == {"min": 0.0, "max": 255.0, "scale": 1.0, "inv_scale": 1.0, "zero_point": 0}
    v = np.array([0.5, 1.5, 2.5, 126.5, 127.0, 127.5, 128.0, 254.5, 255.0, 1e9, -1e9, np.nan, np.inf, -np.inf, -0.0], np.float32)
    assert list(q.quantize(v)) == [1, 2, 3, 127, 127, -128, -128, -1, -1, -1, 0, 0, -1, 0, 0]   # half away from zero
    assert list(q.dequantize(np.array([127, -128, -1], np.int8))) == [127.0, 128.0, 255.0]
    q = hip.ScalarQuantizer(bits=8, mode=hip.SQ_RANGE, value_range=(-128.0, 127.0))
    q.calibrate([0, 1, 0, 1])
    assert list(q.quantize(np.array([-127.5, -0.5, 0.5, -128.0, 127.0], np.float32))) == [1, -128, -127, 0, -1]
    q4 = hip.ScalarQuantizer(bits=4, mode=hip.SQ_RANGE, value_range=(0.0, 15.0))
    q4.calibrate([0, 1, 0, 1])
    assert list(q4.quantize(np.array([6.5, 7.5, 14.5, 15.0, 16.0, -3.0], np.float32))) == [7, 8, 15, 15, 15, 0]
    s = hip.ScalarQuantizer(mode=hip.SQ_SIGNED)
    assert s.calibrate([-127.0, 50.0, 0.0, 1.0])["scale"] == 1.0
    v = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5, 127.0, -127.0], np.float32)
    assert list(s.quantize(v)) == [0, 2, 2, 0, -2, -2, 126, 127, -127]                           # half to even
    assert list(s.dequantize(np.array([-127, 3], np.int8))) == [-127.0, 3.0]


def test_signed_mode_is_symmetric_int8():
    hip = _hip()
    for name, rows in SC.parity_cases() + [("zeros", np.zeros((3, 5), np.float32)), ("tiny", np.full((2, 2), 1e-42, np.float32))]:
        codes, inv = hip.symmetric_int8(rows)
        q = hip.ScalarQuantizer(mode=hip.SQ_SIGNED)
        p = q.calibrate(M.stats_device(rows))
        assert np.float32(p["scale"]) == np.float32(inv) and p["zero_point"] == 0, name
        assert np.array_equal(q.quantize(rows), codes), name


def test_refusals_leave_the_outputs_untouched():
    hip = _hip()
    L = hip.load()
    vals = np.array([0.0, 1.0, np.nan], np.float32)
    out = np.full(3, 99, np.int8)
    good = np.array([-1.0, 1.0, 2.0 / 255.0, 127.5], np.float32)

    def quant(bits, mode, params, v=vals):
        return L.scann_hip_scalar_quantize(hip.ptr(v, hip.f32p), v.size, bits, mode,
                                           None if params is None else hip.ptr(params, hip.f32p), hip.ptr(out, hip.i8p))

    assert quant(5, M.SQ_STDDEV, good) == hip.INVALID_ARGUMENT
    assert quant(8, 7, good) == hip.INVALID_ARGUMENT
    assert quant(8, M.SQ_STDDEV, None) == hip.INVALID_ARGUMENT
    assert quant(8, M.SQ_STDDEV, np.array([1.0, -1.0, 1.0, 1.0], np.float32)) == hip.INVALID_ARGUMENT     # min > max
    assert quant(8, M.SQ_STDDEV, np.array([np.nan, 1.0, 1.0, 1.0], np.float32)) == hip.INVALID_ARGUMENT
    assert quant(8, M.SQ_SIGNED, good) == hip.INVALID_ARGUMENT                                               # a NaN value
    assert quant(8, M.SQ_SIGNED, good, np.array([0.0, np.inf], np.float32)) == hip.INVALID_ARGUMENT
    assert quant(4, M.SQ_SIGNED, good, vals[:2]) == hip.INVALID_ARGUMENT
    assert quant(8, M.SQ_SIGNED, np.array([0, 0, 0.0, 1], np.float32), vals[:2]) == hip.INVALID_ARGUMENT    # scale 0
    assert (out == 99).all()
    assert L.scann_hip_scalar_quantize(hip.ptr(vals, hip.f32p), 3, 8, 0, hip.ptr(good, hip.f32p), None) == hip.INVALID_ARGUMENT
    back = np.full(3, -77.0, np.float32)
    codes = np.zeros(3, np.int8)
    assert L.scann_hip_scalar_dequantize(hip.ptr(codes, hip.i8p), 3, 9, hip.ptr(good, hip.f32p), hip.ptr(back, hip.f32p)) \
        == hip.INVALID_ARGUMENT
    assert L.scann_hip_scalar_dequantize(hip.ptr(codes, hip.i8p), 3, 0, None, hip.ptr(back, hip.f32p)) == hip.INVALID_ARGUMENT
    assert (back == -77.0).all()
    # n == 0 is legal and touches nothing
    assert L.scann_hip_scalar_quantize(None, 0, 8, 0, hip.ptr(good, hip.f32p), None) == hip.OK
    with pytest.raises(hip.ScannError):
        hip.ScalarQuantizer(bits=3).calibrate([0, 1, 0, 1])
    with pytest.raises(ValueError):
        hip.ScalarQuantizer(mode=hip.SQ_RANGE).calibrate([0, 1, 0, 1])


def _compile():
    from scann_rust_amd import build
    build.build_host()
    assert os.path.exists(EXE)
    return EXE


def test_scalar_quantizer_test_compiles_and_fails_loudly_without_gpu():
    exe = _compile()
    import torch
    if torch.cuda.device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 2 and "no HIP device" in r.stdout   # Unavailable, no CPU fallback
        assert "scalar_quantizer_test ok" not in r.stdout and "FAIL" not in r.stdout

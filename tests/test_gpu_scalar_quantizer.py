"""The scalar quantizer on the device (csrc/scalarq.hip) against the numpy model
(tests/scalar_quantizer_model.py) and against the handles the *_create_quantized entry points build from the model's
bytes: statistics, the quantize pass, scann_hip_index_quantize_rows on brute-force, tree and flat-hasher handles, its
refusals, the C++ mirror's program and a recall sanity check.  Everything is compared bit for bit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import pyoracle as orc
from scann_rust_amd import hip
from tests import quantized_checker as qc
from tests import quantized_rerank_cases as QC
from tests import scalar_quantizer_cases as SC
from tests import scalar_quantizer_model as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMTS = {"bf16": hip.ROWS_BF16, "fp8": hip.ROWS_FP8_E4M3, "int8": hip.ROWS_INT8}
MEASURES = {"sql2": hip.SQUARED_L2, "l2": hip.L2, "dot": hip.DOT_PRODUCT}
MODES = (hip.SQ_STDDEV, hip.SQ_SYMMETRIC, hip.SQ_RANGE, hip.SQ_SIGNED)
K = 10
GUARD = 0x5A


def bits_of(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def strides_of(n, dim):
    return SC.STRIDES_257x50 if (n, dim) == (257, 50) else tuple(sorted({dim, hip.compute_stride(dim)}))


@pytest.fixture(scope="module")
def cases():
    return SC.parity_cases()


@pytest.fixture(scope="module")
def base36():
    return QC.Base(36)


def _mode_args(mode, rows):
    """(kwargs of Index.quantize_rows, (a, b) of the model) for a mode"""
    if mode == hip.SQ_RANGE:
        lo, hi = sorted((float(np.float32(rows.min() * 0.5)), float(np.float32(rows.max() * 0.75))))   # clips on both sides
        return dict(value_range=(lo, hi)), (lo, hi)
    if mode == hip.SQ_STDDEV:
        return dict(num_std_devs=1.5), (1.5, 0.0)
    return {}, (0.0, 0.0)


def model_bytes(rows, stride, fmt, mode=hip.SQ_SIGNED, bits=8):
    """([n, stride] elements as quantize_rows stores them: pad columns 0, inv_multiplier, params or None, zero_point)"""
    n, dim = rows.shape
    if fmt == hip.ROWS_INT8:
        a, b = _mode_args(mode, rows)[1]
        codes, params, zp = M.rows_int8(rows, stride, bits, mode, a, b)
        return codes, float(params[2]), params, zp
    elems = qc.bf16_from_f32(rows) if fmt == hip.ROWS_BF16 else orc.fp8_quantize(rows, 1.0)
    out = np.zeros((n, stride), elems.dtype)
    out[:, :dim] = elems
    return out, 1.0, None, 0


# ---- 1. statistics -------------------------------------------------------------------------------------------------
def test_quantization_stats_match_the_model_at_every_stride(cases):
    for name, rows in cases:
        n, dim = rows.shape
        want = M.stats_device(rows)
        for stride in strides_of(n, dim):
            index = hip.bf_create(SC.strided(rows, stride), n, dim, stride, hip.SQUARED_L2)
            got = hip.quantization_stats(index)
            print(name, stride, got, want)
            assert np.array_equal(bits_of(got), bits_of(want)), (name, stride, got, want)
            assert np.array_equal(bits_of(got), bits_of(hip.quantization_stats(index))), (name, "run to run")


def test_quantization_stats_of_a_hasher_handle_equal_the_brute_force_handle(base36):
    base = base36
    rows = base.rows
    want = M.stats_device(rows)
    for stride in (36, 48):
        data = SC.strided(rows, stride)
        ah = hip.txh_create(data=data, **base.desc("ah", stride, hip.SQUARED_L2))
        tree = hip.txh_create(data=data, **base.desc("txh", stride, hip.DOT_PRODUCT))
        bf = hip.bf_create(data, base.n, 36, stride, hip.SQUARED_L2)
        for index in (ah, tree, bf):
            assert np.array_equal(bits_of(hip.quantization_stats(index)), bits_of(want)), stride


# ---- 2. the quantize pass ------------------------------------------------------------------------------------------
def _plant(rows, params, bits):
    """adversarial values at the first and last element of rows and on both sides of every chunk border"""
    x = rows.copy()
    n, dim = x.shape
    adv = SC.adversarial_values(params, bits)
    flat = x.reshape(-1)
    spots = [0, dim - 1, flat.size - dim, flat.size - 1]
    for border in range(M.CHUNK, flat.size, M.CHUNK):
        spots += [border - 1, border]
    for r in range(1, n, max(1, n // 7)):
        spots += [r * dim, r * dim + dim - 1]
    spots = [s for s in dict.fromkeys(spots) if 0 <= s < flat.size]
    for i, s in enumerate(spots):
        flat[s] = adv[i % adv.size]
    if flat.size > adv.size + len(spots):     # and every adversarial value somewhere
        flat[1:1 + adv.size] = adv
    return x


@pytest.mark.parametrize("shape", SC.SHAPES, ids=["%dx%d" % s for s in SC.SHAPES])
def test_scalar_quantize_device_matches_the_model(shape):
    n, dim = shape
    clean = SC.rows_of("gauss37", n, dim, seed=2)
    ran = 0
    for bits in (4, 8):
        for mode in MODES:
            if mode == hip.SQ_SIGNED and bits == 4:
                continue
            a, b = _mode_args(mode, clean)[1]
            stats = M.stats_device(clean) if clean.size > 1 else np.array([-1.0, 2.0, 0.5, 1.0], np.float32)
            params, _ = M.calibrate(stats, bits, mode, a, b)
            rows = _plant(clean, params, bits)
            for stride in strides_of(n, dim):
                outs = sorted({dim, dim + 3, (dim + 15) // 16 * 16 + 16, stride})
                d_rows = torch.from_numpy(SC.strided(rows, stride, fill=777.0)).to(DEV)
                for out_stride in outs:
                    for misalign in ((0, 4) if out_stride == outs[0] else (0,)):
                        total = n * out_stride
                        d_out = torch.full((misalign + total + 64,), GUARD, dtype=torch.int8, device=DEV)
                        hip.scalar_quantize_device(d_rows.data_ptr(), n, dim, stride, d_out.data_ptr() + misalign, out_stride,
                                                   params, bits=bits, mode=mode, stream=_stream())
                        torch.cuda.synchronize()
                        got = d_out.cpu().numpy()
                        assert (got[:misalign] == GUARD).all() and (got[misalign + total:] == GUARD).all(), "guard"
                        got = got[misalign:misalign + total].reshape(n, out_stride)
                        want = M.quantize(rows, params, bits, mode)
                        bad = np.argwhere(got[:, :dim] != want)
                        assert bad.size == 0, (bits, mode, stride, out_stride, bad[:5], rows[tuple(bad[0])])
                        assert (got[:, dim:] == 0).all(), "pad columns"
                        ran += 1
    assert ran >= 7 * 3


def test_scalar_quantize_device_refusals():
    L = hip.load()
    ctx = hip.context(0)
    d = torch.zeros(64, dtype=torch.float32, device=DEV)
    o = torch.full((64,), GUARD, dtype=torch.int8, device=DEV)
    good = np.array([-1.0, 1.0, 2.0 / 255.0, 127.5], np.float32)

    def call(n, dim, stride, bits, mode, params, out_stride, rows=d.data_ptr(), out=o.data_ptr()):
        return L.scann_hip_scalar_quantize_device(ctx, rows, n, dim, stride, bits, mode,
                                                  None if params is None else hip.ptr(params, hip.f32p), out, out_stride, None)

    assert call(4, 4, 3, 8, 0, good, 4) == hip.INVALID_ARGUMENT        # stride < dim
    assert call(4, 4, 4, 8, 0, good, 3) == hip.INVALID_ARGUMENT        # out_stride < dim
    assert call(4, 0, 4, 8, 0, good, 4) == hip.INVALID_ARGUMENT
    assert call(4, 4, 4, 5, 0, good, 4) == hip.INVALID_ARGUMENT
    assert call(4, 4, 4, 8, 9, good, 4) == hip.INVALID_ARGUMENT
    assert call(4, 4, 4, 8, 0, None, 4) == hip.INVALID_ARGUMENT
    assert call(4, 4, 4, 8, 0, np.array([2.0, 1.0, 1.0, 1.0], np.float32), 4) == hip.INVALID_ARGUMENT
    assert call(4, 4, 4, 8, 0, good, 4, rows=None) == hip.INVALID_ARGUMENT
    assert call(4, 4, 4, 8, 0, good, 4, out=None) == hip.INVALID_ARGUMENT
    assert call(0, 4, 4, 8, 0, good, 4) == hip.OK
    torch.cuda.synchronize()
    assert (o.cpu().numpy() == GUARD).all()


# ---- 3. brute force ------------------------------------------------------------------------------------------------
@pytest.fixture
def force_shortlist(monkeypatch):
    monkeypatch.setenv("SCANN_HIP_BF_SHORTLIST_MIN_ROWS", "1")
    monkeypatch.setenv("SCANN_HIP_BF_SHORTLIST_MIN_QUERIES", "1")
    monkeypatch.setenv("SCANN_HIP_SMALL", "0")


def _same_results(a, b, what):
    assert np.array_equal(a[2], b[2]), what
    assert np.array_equal(bits_of(a[1]), bits_of(b[1])), what
    assert np.array_equal(a[0], b[0]), what


def _check_bf_twin(rows, stride, fmt, measure, mode, bits, what):
    n, dim = rows.shape
    data = SC.strided(rows, stride, fill=1.0e30)
    src = hip.bf_create(data, n, dim, stride, measure)
    q = SC.rows_of("centred", 64, dim, seed=9)
    before = src.search_batched(q[:5], K)
    kw = _mode_args(mode, rows)[0] if fmt == hip.ROWS_INT8 else {}
    got, gp = src.quantize_rows(fmt, mode=mode, bits=bits, **kw)
    rows_q, inv, params, zp = model_bytes(rows, stride, fmt, mode, bits)
    twin = hip.bf_create_quantized(rows_q, n, dim, stride, fmt, measure, inv)
    if params is not None:
        assert np.array_equal(bits_of([gp["min"], gp["max"], gp["scale"], gp["inv_scale"]]), bits_of(params)), what
        assert gp["zero_point"] == zp, what
    else:
        assert gp == {"min": 0.0, "max": 0.0, "scale": 1.0, "inv_scale": 1.0, "zero_point": 0}
    assert got.size() == n and got.dimensionality() == dim
    assert got.device_bytes() == twin.device_bytes(), what
    for nq in (1, 5, 64):
        _same_results(got.search_batched(q[:nq], K), twin.search_batched(q[:nq], K), (what, nq))
    d_got, d_twin = hip.bf_distances(got, q[:5]), hip.bf_distances(twin, q[:5])
    assert np.array_equal(bits_of(d_got), bits_of(d_twin)), what
    radius = float(np.sort(d_twin[0])[min(n - 1, 20)])
    r0, r1 = got.search_radius(q[0], radius), twin.search_radius(q[0], radius)
    assert r0[2] == r1[2] and np.array_equal(r0[0], r1[0]) and np.array_equal(bits_of(r0[1]), bits_of(r1[1])), what
    allow = hip.allow_bitmap(n, np.arange(0, n, 3))
    _same_results(got.search_batched(q[:5], K, allow=allow), twin.search_batched(q[:5], K, allow=allow), (what, "filtered"))
    ks = np.array([1, 3, K, 2, 7], np.uint32)
    _same_results(got.search_batched_with_params(q[:5], ks), twin.search_batched_with_params(q[:5], ks), (what, "params"))
    _same_results(src.search_batched(q[:5], K), before, (what, "source"))        # the source still answers as before
    return got


@pytest.mark.parametrize("measure", list(MEASURES))
@pytest.mark.parametrize("fmt", list(FMTS))
def test_bf_quantize_rows_equals_create_quantized(fmt, measure):
    rows = SC.rows_of("centred", 1000, 128, seed=4)
    _check_bf_twin(rows, 128, FMTS[fmt], MEASURES[measure], hip.SQ_SIGNED, 8, (fmt, measure))
    small = SC.rows_of("gauss37", 257, 50, seed=4) * np.float32(0.01)
    _check_bf_twin(small, 52, FMTS[fmt], MEASURES[measure], hip.SQ_STDDEV, 8, (fmt, measure, "257x50"))


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("mode", MODES)
def test_bf_quantize_rows_int8_modes(mode, bits):
    if mode == hip.SQ_SIGNED and bits == 4:
        rows = SC.rows_of("centred", 40, 8)
        src = hip.bf_create(rows, 40, 8, 8, hip.SQUARED_L2)
        with pytest.raises(hip.ScannError) as e:
            src.quantize_rows(hip.ROWS_INT8, mode=mode, bits=bits)
        assert e.value.code == hip.INVALID_ARGUMENT
        return
    rows = SC.rows_of("gauss37", 4099, 33, seed=6)
    _check_bf_twin(rows, 33, hip.ROWS_INT8, hip.SQUARED_L2, mode, bits, (mode, bits))
    _check_bf_twin(rows[:300], 48, hip.ROWS_INT8, hip.DOT_PRODUCT, mode, bits, (mode, bits, "stride 48"))


@pytest.mark.parametrize("fmt", list(FMTS))
def test_bf_quantize_rows_with_the_shortlist(force_shortlist, fmt):
    """the norms path: the converted handle qualifies for the bf16 shortlist exactly as its twin does"""
    rows = SC.rows_of("centred", 1000, 128, seed=8)
    for measure in (hip.SQUARED_L2, hip.DOT_PRODUCT):
        got = _check_bf_twin(rows, 128, FMTS[fmt], measure, hip.SQ_SIGNED, 8, (fmt, measure, "shortlist"))
        assert got.device_bytes() == 1000 * 128 * (2 if fmt == "bf16" else 1) + 1000 * 4      # rows + one norm per row


# ---- 4. tree and flat hasher -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(FMTS))
@pytest.mark.parametrize("kind", ["txh", "ah"])
def test_txh_quantize_rows_equals_create_quantized(tmp_path, base36, kind, fmt):
    base, f = base36, FMTS[fmt]
    stride, measure = 41, hip.DOT_PRODUCT if kind == "ah" else hip.SQUARED_L2
    rows = base.rows
    src = hip.txh_create(data=SC.strided(rows, stride, fill=1.0e30), **base.desc(kind, stride, measure))
    mode = hip.SQ_SIGNED if kind == "ah" else hip.SQ_SYMMETRIC
    o = base.opts(kind, 64)
    before = src.search_batched(base.q[:5], K, o)
    got, gp = src.quantize_rows(f, mode=mode)
    rows_q, inv, params, zp = model_bytes(rows, stride, f, mode)
    twin = hip.txh_create_quantized(rows=rows_q, fmt=f, inv_multiplier=inv, **base.desc(kind, stride, measure))
    if params is not None:
        assert np.array_equal(bits_of([gp["min"], gp["max"], gp["scale"], gp["inv_scale"]]), bits_of(params))
    assert got.device_bytes() == twin.device_bytes() and got.size() == twin.size()
    for exact in (1, 0):
        o = base.opts(kind, 64)
        o.exact_reorder = exact
        for nq in (1, 5, 64):
            _same_results(got.search_batched(base.q[:nq], K, o), twin.search_batched(base.q[:nq], K, o), (kind, fmt, exact, nq))
    _same_results(src.search_batched(base.q[:5], K, base.opts(kind, 64)), before, "source")
    path = str(tmp_path / "converted.scannidx")
    hip.index_write_file(got, path)
    loaded = hip.load_file(path)
    o = base.opts(kind, 64)
    _same_results(loaded.search_batched(base.q[:20], K, o), twin.search_batched(base.q[:20], K, o), "loaded")
    assert loaded.device_bytes() == twin.device_bytes()
    # a converted handle is refused wherever its twin is
    with pytest.raises(hip.ScannError) as e:
        got.quantize_rows(f)
    assert e.value.code == hip.INVALID_ARGUMENT
    with pytest.raises(hip.ScannError) as e:
        got.search_mmr(base.q[:2], 5, 20, 0.5)
    with pytest.raises(hip.ScannError) as e2:
        twin.search_mmr(base.q[:2], 5, 20, 0.5)
    assert e.value.code == e2.value.code == hip.UNIMPLEMENTED
    with pytest.raises(hip.ScannError) as e:
        hip.Mutable(got, 16)
    with pytest.raises(hip.ScannError) as e2:
        hip.Mutable(twin, 16)
    assert e.value.code == e2.value.code


# ---- 5. refusals -------------------------------------------------------------------------------------------------------
def _refused(index, fmt=hip.ROWS_INT8, bits=8, mode=hip.SQ_SIGNED, a=3.0, b=0.0):
    """status of a raw call; the out handle, the params and the zero point must come back untouched"""
    L = hip.load()
    h = ctypes.c_void_p(0xDEAD0)
    params = np.full(4, -77.0, np.float32)
    zp = ctypes.c_int32(-77)
    s = L.scann_hip_index_quantize_rows(index.h, fmt, bits, mode, ctypes.c_float(a), ctypes.c_float(b), ctypes.byref(h),
                                        hip.ptr(params, hip.f32p), ctypes.byref(zp))
    assert s != hip.OK
    assert h.value == 0xDEAD0 and (params == -77.0).all() and zp.value == -77
    return s


def _stats_status(index):
    st = np.full(4, -77.0, np.float32)
    s = hip.load().scann_hip_index_quantization_stats(index.h, hip.ptr(st, hip.f32p))
    if s != hip.OK:
        assert (st == -77.0).all()
    return s


def test_quantize_rows_refusals(base36):
    base = base36
    rows = SC.rows_of("centred", 64, 16)
    f32 = hip.bf_create(rows, 64, 16, 16, hip.SQUARED_L2)
    assert _refused(f32, fmt=9) == hip.INVALID_ARGUMENT
    assert _refused(f32, mode=7) == hip.INVALID_ARGUMENT
    assert _refused(f32, bits=5, mode=hip.SQ_STDDEV) == hip.INVALID_ARGUMENT
    assert _refused(f32, bits=4, mode=hip.SQ_SIGNED) == hip.INVALID_ARGUMENT
    assert _refused(f32, mode=hip.SQ_RANGE, a=2.0, b=1.0) == hip.INVALID_ARGUMENT
    assert _refused(f32, mode=hip.SQ_RANGE, a=float("nan"), b=1.0) == hip.INVALID_ARGUMENT
    assert hip.load().scann_hip_index_quantize_rows(f32.h, hip.ROWS_INT8, 8, 0, 3.0, 0.0, None, None, None) == hip.INVALID_ARGUMENT
    assert hip.load().scann_hip_index_quantize_rows(None, hip.ROWS_INT8, 8, 0, 3.0, 0.0, None, None, None) == hip.INVALID_ARGUMENT
    empty = hip.bf_create(np.zeros((0, 16), np.float32), 0, 16, 16, hip.SQUARED_L2)
    assert _refused(empty) == hip.INVALID_ARGUMENT and _stats_status(empty) == hip.INVALID_ARGUMENT
    assert "Cannot quantize empty dataset" in hip.load().scann_hip_last_error().decode()
    quantized, _ = f32.quantize_rows(hip.ROWS_BF16)
    assert _refused(quantized) == hip.INVALID_ARGUMENT and _stats_status(quantized) == hip.INVALID_ARGUMENT
    for bad in (np.nan, np.inf):
        x = rows.copy()
        x[63, 15] = bad
        nonfinite = hip.bf_create(x, 64, 16, 16, hip.SQUARED_L2)
        assert _refused(nonfinite, mode=hip.SQ_SIGNED) == hip.INVALID_ARGUMENT
        assert _stats_status(nonfinite) == hip.OK
    for measure in (hip.L1, hip.COSINE):
        other = hip.bf_create(rows, 64, 16, 16, measure)
        assert _refused(other) == hip.UNIMPLEMENTED and _stats_status(other) == hip.UNIMPLEMENTED
    norows = hip.txh_create(data=None, **base.desc("txh", 36, hip.SQUARED_L2))
    assert _refused(norows) == hip.FAILED_PRECONDITION and _stats_status(norows) == hip.FAILED_PRECONDITION
    l1 = hip.txh_create(data=base.rows, **base.desc("ah", 36, hip.L1))
    assert _refused(l1) == hip.UNIMPLEMENTED
    kw = dict(base.desc("txh", 36, hip.SQUARED_L2), codebook=None, codes=None)
    partitioned = hip.txh_create(data=base.rows, **kw)
    assert _refused(partitioned) == hip.UNIMPLEMENTED and _stats_status(partitioned) == hip.UNIMPLEMENTED
    assert _stats_status(f32) == hip.OK          # and the source is still good
    assert hip.load().scann_hip_index_quantization_stats(f32.h, None) == hip.INVALID_ARGUMENT


# ---- 6. the C++ mirror -------------------------------------------------------------------------------------------------
def test_scalar_quantizer_test_on_the_device():
    from scann_rust_amd import build
    build.build_host()
    exe = os.path.join(ROOT, "scann_rust_amd", "host", "scalar_quantizer_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scalar_quantizer_test ok" in r.stdout


# ---- 7. recall, as a sanity check ----------------------------------------------------------------------------------------
def test_signed_int8_recall_equals_the_host_route():
    """top-10 of the SQ_SIGNED int8 handle against the f32 handle's on 2000 x 64 centred uniform rows.  No threshold is
    claimed for the quantizer; the bound that means something is that the device route returns exactly the rows of the
    host route (hip.symmetric_int8 + bf_create_quantized), whose recall is computed alongside."""
    n, dim, nq = 2000, 64, 32
    rows = SC.rows_of("centred", n, dim, seed=21)
    q = SC.rows_of("centred", nq, dim, seed=22)
    f32 = hip.bf_create(rows, n, dim, dim, hip.SQUARED_L2)
    truth = f32.search_batched(q, K)[0]
    dev, params = f32.quantize_rows(hip.ROWS_INT8, mode=hip.SQ_SIGNED)
    codes, inv = hip.symmetric_int8(rows)
    host = hip.bf_create_quantized(codes, n, dim, dim, hip.ROWS_INT8, hip.SQUARED_L2, inv)
    a, b = dev.search_batched(q, K), host.search_batched(q, K)
    _same_results(a, b, "device route vs host route")
    assert np.float32(params["scale"]) == np.float32(inv)

    def recall(idx):
        return float(np.mean([len(set(idx[i]) & set(truth[i])) / K for i in range(nq)]))

    print("recall@10 device route %.4f, host route %.4f" % (recall(a[0]), recall(b[0])))
    assert recall(a[0]) == recall(b[0])

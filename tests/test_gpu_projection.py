"""The projection kernel (csrc/project.hip) against the numpy model (tests/projection_model.py), bit for
bit, NaNs comparing as NaN: every kind, dims from 1 to 4096, row counts that end inside a tile, strides above the dims,
data that overflows, cancels and underflows; the host and the device entries; the elements past out_dim; every error
of scann_hip_projection_create / scann_hip_project / scann_hip_project_device."""
import ctypes

import numpy as np
import pytest
import torch

from scann_rust_amd import hip
from tests import projection_model as pm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IN_DIMS = (1, 3, 64, 65, 100, 768, 4096)
OUT_DIMS = (1, 8, 33, 128, 256)
NS = (1, 7, 257, 1000)
SENTINEL = np.float32(-12345.5)


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _make(kind, M=None, mean=None, **kw):
    if kind == pm.TRUNCATE:
        return hip.Projection(hip.PROJ_TRUNCATE, **kw)
    return hip.Projection(kind, matrix=M, mean=mean if kind == pm.PCA else None)


def _strided(X, stride, fill=np.nan):
    """X in the leading columns of an [n, stride] array; the pad columns hold `fill` (NaN: a kernel that read them
    would poison its sums)"""
    out = np.full((X.shape[0], stride), fill, np.float32)
    out[:, :X.shape[1]] = X
    return out


def host_project(p, X, row_stride, out_stride):
    """scann_hip_project through strided arrays: (projected [n, out_dim], pad columns of the output)"""
    n, in_dim = X.shape
    od = p.info()[2]
    out = np.full((n, out_stride), SENTINEL, np.float32)
    p.project(_strided(X, row_stride), row_dim=in_dim, out=out)
    return out[:, :od].copy(), out[:, od:].copy()


def device_project(p, X, row_stride, out_stride):
    """scann_hip_project_device on torch's current stream, same shapes"""
    n = X.shape[0]
    od = p.info()[2]
    dx = torch.from_numpy(_strided(X, row_stride)).to(DEV)
    do = torch.full((n, out_stride), float(SENTINEL), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    p.project_device(dx.data_ptr(), n, row_stride, do.data_ptr(), out_stride, stream=_stream())
    torch.cuda.synchronize()
    out = do.cpu().numpy()
    return out[:, :od].copy(), out[:, od:].copy()


def check_both_entries(p, X, want, row_stride, out_stride, what):
    for name, fn in (("host", host_project), ("device", device_project)):
        got, pad = fn(p, X, row_stride, out_stride)
        assert pm.bits_equal(got, want), "%s, %s entry: %d of %d outputs differ from the model" % (
            what, name, int((got.view(np.uint32) != want.view(np.uint32)).sum()), want.size)
        assert (pad == SENTINEL).all(), "%s, %s entry wrote past out_dim" % (what, name)


@pytest.mark.parametrize("out_dim", OUT_DIMS)
@pytest.mark.parametrize("in_dim", IN_DIMS)
def test_every_shape_matches_the_model(in_dim, out_dim):
    """in_dim x out_dim, MATRIX and PCA, strides above the dims.  The family and the row count rotate with i + j (the
    positions of in_dim and out_dim): every in_dim and every out_dim meets every family, so the order-sensitive ones
    reach several output tiles at every in_dim, and every in_dim meets every n.  One exception, within the n set: at
    in_dim = 4096 the numpy model of more than 257 x 33 outputs takes seconds, so such a case runs n = 7 (4096 still
    meets several row tiles at out_dim 1 and 8)."""
    i, j = IN_DIMS.index(in_dim), OUT_DIMS.index(out_dim)
    case = i * len(OUT_DIMS) + j
    n = NS[(i + j) % len(NS)]
    if in_dim == 4096 and n * out_dim > 257 * 33:
        n = 7
    fam = pm.FAMILIES[(i + j) % len(pm.FAMILIES)]
    X, M, mean = pm.family(fam, n, in_dim, out_dim, 100 + case)
    for kind in (pm.MATRIX, pm.PCA):
        p = _make(kind, M, mean)
        assert p.info() == (kind, in_dim, out_dim, 0)
        want = pm.project(kind, X, M, mean)
        check_both_entries(p, X, want, in_dim + 3, out_dim + 5, "%s %d->%d n=%d kind %d" % (fam, in_dim, out_dim, n, kind))
        p.close()


@pytest.mark.parametrize("fam", pm.FAMILIES)
def test_every_family_at_every_row_count(fam):
    """65 -> 33 (one element past a chunk and a tile edge on both sides) at n = 1, 7, 257, 1000; dense and padded rows"""
    in_dim, out_dim = 65, 33
    for n in NS:
        X, M, mean = pm.family(fam, n, in_dim, out_dim, 7 * n)
        for kind in (pm.MATRIX, pm.PCA):
            p = _make(kind, M, mean)
            want = pm.project(kind, X, M, mean)
            check_both_entries(p, X, want, in_dim, out_dim, "%s n=%d kind %d dense" % (fam, n, kind))
            check_both_entries(p, X, want, in_dim + 7, out_dim + 1, "%s n=%d kind %d padded" % (fam, n, kind))
            p.close()
    if fam == "overflow":   # the family reaches its cases on the device too
        assert np.isinf(want).any() and np.isnan(want).any() and np.isfinite(want).any()
    if fam == "subnormal":
        assert ((want != 0) & (np.abs(want) < np.finfo(np.float32).tiny)).any()


def test_several_row_tiles_and_output_tiles():
    """1000 rows x 256 outputs of 768: 16 row tiles (the last of 40 rows) x 4 output tiles"""
    X, M, mean = pm.family("normal", 1000, 768, 256, 5)
    p = _make(pm.PCA, M, mean)
    check_both_entries(p, X, pm.project(pm.PCA, X, M, mean), 768, 256, "1000 x 768 -> 256")
    p.close()


def test_identity_returns_the_input_with_positive_zero():
    X = np.array([[1.5, -0.0, 0.0, -2.25, 1e-42], [-0.0, -0.0, 3.0, 0.0, -1e-42]], np.float32)
    p = _make(pm.MATRIX, np.eye(5, dtype=np.float32))
    want = X.copy()
    want[want == 0] = 0.0   # 0.0 + (-0.0 * 1) = +0.0
    check_both_entries(p, X, want, 5, 5, "identity")
    assert pm.bits_equal(pm.project(pm.MATRIX, X, np.eye(5, dtype=np.float32)), want)
    p.close()


@pytest.mark.parametrize("in_dim,out_dim,start", [(1, 1, 0), (3, 2, 1), (128, 32, 17), (100, 100, 0), (4096, 256, 3840),
                                                  (65, 1, 64)])
def test_truncate_is_the_window(in_dim, out_dim, start):
    for n in (1, 257):
        X = pm.family("overflow", n, in_dim, 1, start + n)[0]
        X[0, start] = np.nan   # copied as it is
        p = _make(pm.TRUNCATE, in_dim=in_dim, out_dim=out_dim, start=start)
        assert p.info() == (hip.PROJ_TRUNCATE, in_dim, out_dim, start)
        want = pm.project(pm.TRUNCATE, X, start=start, out_dim=out_dim)
        check_both_entries(p, X, want, in_dim + 2, out_dim + 3, "truncate %d[%d:+%d] n=%d" % (in_dim, start, out_dim, n))
        p.close()


def test_untrained_pca_is_truncation_from_zero():
    X = pm.family("normal", 9, 20, 1, 3)[0]
    p = _make(pm.TRUNCATE, in_dim=20, out_dim=6, start=0)
    check_both_entries(p, X, X[:, :6], 20, 6, "untrained pca")
    p.close()


def test_no_rows_is_a_no_op():
    p = _make(pm.MATRIX, np.ones((2, 3), np.float32))
    assert p.project(np.zeros((0, 3), np.float32)).shape == (0, 2)
    p.project_device(0, 0, 3, 0, 2, stream=_stream())
    p.close()


def test_the_object_copies_its_arrays():
    X, M, mean = pm.family("normal", 7, 10, 4, 1)
    want = pm.project(pm.PCA, X, M, mean)
    M2, mean2 = M.copy(), mean.copy()
    p = _make(pm.PCA, M2, mean2)
    M2[:] = 0
    mean2[:] = 0
    assert pm.bits_equal(p.project(X), want)
    p.close()


# ---- errors ------------------------------------------------------------------------------------------------------------
def _create_status(kind, in_dim, out_dim, matrix, mean, start):
    L = hip.load()
    h = ctypes.c_void_p()
    s = L.scann_hip_projection_create(hip.context(0), kind, in_dim, out_dim, hip.ptr(matrix, hip.f32p), hip.ptr(mean, hip.f32p),
                                      start, ctypes.byref(h))
    if s == hip.OK:
        L.scann_hip_projection_destroy(h)
    return s, (L.scann_hip_last_error() or b"").decode()


def test_create_errors():
    M, mean = np.ones((2, 4), np.float32), np.zeros(4, np.float32)
    inv = hip.INVALID_ARGUMENT
    for kind in (hip.PROJ_MATRIX, hip.PROJ_PCA):
        s, msg = _create_status(kind, 4, 2, None, mean, 0)
        assert s == inv and "matrix is null" in msg
    s, msg = _create_status(hip.PROJ_PCA, 4, 2, M, None, 0)
    assert s == inv and "mean is null" in msg
    assert _create_status(hip.PROJ_MATRIX, 4, 2, M, None, 0)[0] == hip.OK   # MATRIX reads no mean
    for kind in (hip.PROJ_MATRIX, hip.PROJ_PCA, hip.PROJ_TRUNCATE):
        assert _create_status(kind, 0, 2, M, mean, 0)[0] == inv
        assert _create_status(kind, 4, 0, M, mean, 0)[0] == inv
    s, msg = _create_status(hip.PROJ_TRUNCATE, 4, 2, None, None, 3)
    assert s == inv and "start + out_dim" in msg
    assert _create_status(hip.PROJ_TRUNCATE, 4, 2, None, None, 2)[0] == hip.OK
    assert _create_status(hip.PROJ_TRUNCATE, 4, 2, None, None, 0xFFFFFFFF)[0] == inv   # (no 32-bit wrap)
    assert _create_status(0, 4, 2, M, mean, 0)[0] == inv and _create_status(4, 4, 2, M, mean, 0)[0] == inv


def test_project_errors():
    L = hip.load()
    p = _make(pm.MATRIX, np.ones((2, 4), np.float32))
    X = np.zeros((3, 6), np.float32)
    out = np.zeros((3, 4), np.float32)
    f = lambda a: hip.ptr(a, hip.f32p)
    inv = hip.INVALID_ARGUMENT
    assert L.scann_hip_project(p.h, f(X), 3, 6, 5, f(out), 4) == inv           # row_dim != in_dim
    assert b"row_dim" in L.scann_hip_last_error()
    assert L.scann_hip_project(p.h, f(X), 3, 6, 3, f(out), 4) == inv
    assert L.scann_hip_project(p.h, f(X), 3, 3, 4, f(out), 4) == inv           # row_stride < row_dim
    assert b"stride" in L.scann_hip_last_error()
    assert L.scann_hip_project(p.h, f(X), 3, 6, 4, f(out), 1) == inv           # out_stride < out_dim
    assert L.scann_hip_project(p.h, None, 3, 6, 4, f(out), 4) == inv
    assert L.scann_hip_project(p.h, f(X), 3, 6, 4, None, 4) == inv
    assert L.scann_hip_project(None, f(X), 3, 6, 4, f(out), 4) == inv
    assert L.scann_hip_project(p.h, f(X), 3, 6, 4, f(out), 4) == hip.OK
    dx = torch.zeros((3, 6), dtype=torch.float32, device=DEV)
    do = torch.zeros((3, 4), dtype=torch.float32, device=DEV)
    vp = ctypes.c_void_p
    st = vp(_stream() or None)
    assert L.scann_hip_project_device(p.h, vp(dx.data_ptr()), 3, 3, vp(do.data_ptr()), 4, st) == inv   # row_stride < in_dim
    assert L.scann_hip_project_device(p.h, vp(dx.data_ptr()), 3, 6, vp(do.data_ptr()), 1, st) == inv   # out_stride < out_dim
    assert L.scann_hip_project_device(p.h, None, 3, 6, vp(do.data_ptr()), 4, st) == inv
    assert L.scann_hip_project_device(p.h, vp(dx.data_ptr()), 3, 6, None, 4, st) == inv
    assert L.scann_hip_project_device(None, vp(dx.data_ptr()), 3, 6, vp(do.data_ptr()), 4, st) == inv
    assert L.scann_hip_project_device(p.h, vp(dx.data_ptr()), 3, 6, vp(do.data_ptr()), 4, st) == hip.OK
    torch.cuda.synchronize()
    assert L.scann_hip_projection_info(None, None) == inv
    p.close()

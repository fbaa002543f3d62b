"""The projection model (tests/projection_model.py) against hand-computed values, the order sensitivity of the data the
GPU tests use, and the trainer's projection helpers.  No GPU."""
import os

import numpy as np
import pytest

import projection_model as pm
from scann_rust_amd import synth, trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_hand_computed_matrix():
    X = np.array([[1.0, 2.0, 3.0]], F)
    M = np.array([[1.0, 0.5, 0.25], [2.0, -1.0, 0.0]], F)
    # row 0: ((0 + 1*1) + 2*0.5) + 3*0.25 = 2.75; row 1: ((0 + 1*2) + 2*-1) + 3*0 = 0
    assert pm.project(pm.MATRIX, X, M).tolist() == [[2.75, 0.0]]


def test_hand_computed_pca_subtracts_the_mean_first():
    X = np.array([[3.0, 5.0], [1.0, 1.0]], F)
    M = np.array([[1.0, 1.0], [1.0, -1.0]], F)
    mean = np.array([1.0, 2.0], F)
    # (3-1)*1 + (5-2)*1 = 5; (3-1)*1 + (5-2)*-1 = -1; (1-1) + (1-2) = -1; 0 - (-1) = 1
    assert pm.project(pm.PCA, X, M, mean).tolist() == [[5.0, -1.0], [-1.0, 1.0]]
    # the mean is PCA's alone
    assert pm.project(pm.MATRIX, X, M, mean).tolist() == [[8.0, -2.0], [2.0, 0.0]]


def test_each_step_rounds_once_in_f32():
    # 2^24 + 1 is not an f32: the chain ((0 + 2^24) + 1) + 1 stays at 2^24, the exact sum is 2^24 + 2
    X = np.array([[16777216.0, 1.0, 1.0]], F)
    M = np.ones((1, 3), F)
    assert pm.project(pm.MATRIX, X, M)[0, 0] == F(16777216.0)
    assert pm.project(pm.MATRIX, X, M, descending=True)[0, 0] == F(16777218.0)
    # a product that a fused multiply-add would keep exact: (1 + 2^-12)^2 - (1 + 2^-11) = 2^-24, but the product rounds
    # to 1 + 2^-11 first, so the separate add gives 0
    a = F(1.0 + 2.0 ** -12)
    X = np.array([[a, F(1.0 + 2.0 ** -11)]], F)
    M = np.array([[a, F(-1.0)]], F)
    assert pm.project(pm.MATRIX, X, M)[0, 0] == F(0.0)


def test_truncate_windows():
    X = np.arange(12, dtype=F).reshape(2, 6)
    assert pm.project(pm.TRUNCATE, X, start=0, out_dim=6).tolist() == X.tolist()
    assert pm.project(pm.TRUNCATE, X, start=2, out_dim=3).tolist() == [[2.0, 3.0, 4.0], [8.0, 9.0, 10.0]]
    assert pm.project(pm.TRUNCATE, X, start=5, out_dim=1).tolist() == [[5.0], [11.0]]


def test_untrained_pca_equals_truncation():
    """PcaProjection before train() copies the leading out_dim values (pca.rs): TRUNCATE with start = 0"""
    X = synth.uniform_f32(5, 9, 1)
    assert np.array_equal(pm.project(pm.TRUNCATE, X, start=0, out_dim=4), X[:, :4])


def test_identity_returns_the_input_with_positive_zero():
    X = np.array([[1.5, -0.0, 0.0, -2.25, 1e-42, np.inf]], F)
    out = pm.project(pm.MATRIX, X[:, :5], np.eye(5, dtype=F))
    want = np.array([[1.5, 0.0, 0.0, -2.25, 1e-42]], F)   # 0.0 + (-0.0) = +0.0; the subnormal survives
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    # an infinite input poisons every other output of the row (inf * 0 = NaN): the chain propagates it
    out = pm.project(pm.MATRIX, X, np.eye(6, dtype=F))
    assert np.isnan(out[0, :5]).all() and out[0, 5] == np.inf


def test_bits_equal_treats_nans_as_equal_and_zeros_as_different():
    a = np.array([np.nan, 1.0, 0.0], F)
    b = a.copy()
    b.view(np.uint32)[0] |= 1   # another NaN payload
    assert pm.bits_equal(a, b)
    b[2] = -0.0
    assert not pm.bits_equal(a, b)
    assert not pm.bits_equal(a, np.array([1.0, 1.0, 0.0], F))


@pytest.mark.parametrize("kind", [pm.MATRIX, pm.PCA])
@pytest.mark.parametrize("name", pm.ORDER_SENSITIVE)
def test_families_are_order_sensitive(name, kind):
    """On the data the GPU tests use, a wrong summation order or a blocked / fused dot product must change at least one
    bit -- otherwise such a kernel could pass them."""
    X, M, mean = pm.family(name, 64, 100, 33, 7)
    want = pm.project(kind, X, M, mean)
    assert np.isfinite(want).all()
    Xc = X - mean if kind == pm.PCA else X
    with np.errstate(all="ignore"):
        blas = (Xc @ M.T).astype(F)
    assert not pm.bits_equal(want, blas), "X @ M.T gives the same bits"
    assert not pm.bits_equal(want, pm.project(kind, X, M, mean, descending=True)), "descending i gives the same bits"
    if kind == pm.PCA:   # and the centring matters
        assert not pm.bits_equal(want, pm.project(pm.MATRIX, X, M))


def test_special_families_reach_their_cases():
    X, M, mean = pm.family("subnormal", 16, 64, 8, 3)
    tiny = np.finfo(F).tiny
    assert (np.abs(X[X != 0]) < tiny).all()
    out = pm.project(pm.MATRIX, X, M)
    assert ((out != 0) & (np.abs(out) < tiny)).any(), "no subnormal output"
    X, M, mean = pm.family("overflow", 64, 64, 8, 3)
    out = pm.project(pm.MATRIX, X, M)
    assert np.isinf(out).any() and np.isnan(out).any() and np.isfinite(out).any(), \
        "the overflow family must reach +-inf, inf - inf and a finite sum"
    X, M, mean = pm.family("big-mean", 16, 64, 8, 3)
    assert np.abs(X - mean).max() < 0.0051 and X.min() >= 100.0


# ---- trainer helpers ---------------------------------------------------------------------------------------------------
def _orthonormal_within(M, in_dim):
    G = M.astype(np.float64) @ M.astype(np.float64).T
    return np.abs(G - np.eye(M.shape[0])).max() <= in_dim * 2.0 ** -23


def test_pca_projection_is_orthonormal_and_ordered():
    rng = np.random.default_rng(5)
    in_dim, out_dim = 48, 12
    scales = np.linspace(4.0, 0.1, in_dim)
    Q, _ = np.linalg.qr(rng.standard_normal((in_dim, in_dim)))
    X = ((rng.standard_normal((3000, in_dim)) * scales) @ Q.T + 3.0).astype(F)
    M, mean = trainer.pca_projection(X, out_dim)
    assert M.dtype == F and mean.dtype == F and M.shape == (out_dim, in_dim) and mean.shape == (in_dim,)
    # unit vectors rounded to f32: each entry is off by at most 2^-24 relative, a Gram entry by at most in_dim * 2^-23
    assert _orthonormal_within(M, in_dim)
    assert np.allclose(mean, X.astype(np.float64).mean(0), atol=1e-5)
    var = pm.project(pm.PCA, X, M, mean).astype(np.float64).var(0)
    assert (np.diff(var) <= 1e-3 * var[:-1]).all(), "component variances do not descend: %s" % var
    assert var[0] > 10.0 and var[-1] < var[0]
    # sampling takes max_samples rows and stays deterministic
    A = trainer.pca_projection(X, out_dim, max_samples=500, seed=9)
    B = trainer.pca_projection(X, out_dim, max_samples=500, seed=9)
    assert np.array_equal(A[0], B[0]) and np.array_equal(A[1], B[1]) and _orthonormal_within(A[0], in_dim)
    with pytest.raises(ValueError):
        trainer.pca_projection(X, in_dim + 1)


def test_random_orthogonal_is_orthonormal():
    for in_dim, out_dim in ((96, 32), (64, 64), (768, 128)):
        M = trainer.random_orthogonal(in_dim, out_dim, 11)
        assert M.dtype == F and M.shape == (out_dim, in_dim)
        assert _orthonormal_within(M, in_dim)
        assert np.array_equal(M, trainer.random_orthogonal(in_dim, out_dim, 11))
    assert not np.array_equal(trainer.random_orthogonal(16, 4, 1), trainer.random_orthogonal(16, 4, 2))
    with pytest.raises(ValueError):
        trainer.random_orthogonal(8, 9, 0)


def test_trainer_project_rows_is_the_model():
    for fam in pm.FAMILIES:   # the product's host loop and the tests' model are written twice on purpose: they must agree
        X, M, mean = pm.family(fam, 50, 37, 9, 2)
        assert pm.bits_equal(trainer.project_rows(X, "matrix", matrix=M), pm.project(pm.MATRIX, X, M)), fam
        assert pm.bits_equal(trainer.project_rows(X, "pca", matrix=M, mean=mean), pm.project(pm.PCA, X, M, mean)), fam
    assert np.array_equal(trainer.project_rows(X, "truncate", start=3, out_dim=5), X[:, 3:8])


def test_build_projected_txh_index_shapes():
    n, in_dim, out_dim, L, S = 1500, 40, 16, 6, 8
    X = synth.uniform_f32(n, in_dim, 4)
    M = trainer.random_orthogonal(in_dim, out_dim, 3)
    ix = trainer.build_projected_txh_index(X, dict(kind="matrix", matrix=M), L, S, kmeans_iters=2, pq_iters=2)
    assert ix["out_dim"] == out_dim and ix["projected"].shape == (n, out_dim)
    assert pm.bits_equal(ix["projected"], pm.project(pm.MATRIX, X, M))
    assert ix["centers"].shape == (L, out_dim) and ix["codebook"].shape == (S, 16, out_dim // S)
    assert ix["codes"].shape == (n, S) and ix["leaf_off"].shape == (L + 1,) and ix["leaf_off"][-1] == n
    assert sorted(ix["leaf_ids"].tolist()) == list(range(n))
    # a caller-supplied projector (hip.Projection(...).project on a GPU) replaces the host loop
    calls = []
    ix2 = trainer.build_projected_txh_index(X, dict(kind="truncate", start=2, out_dim=out_dim), 0, S, pq_iters=2,
                                            project=lambda r: calls.append(1) or r[:, 2:2 + out_dim])
    assert calls == [1] and "centers" not in ix2 and ix2["codes"].shape == (n, S)


def test_new_symbols_are_declared_bound_and_built():
    import re
    from scann_rust_amd import build, hip
    names = ["scann_hip_projection_create", "scann_hip_projection_destroy", "scann_hip_projection_info", "scann_hip_project",
             "scann_hip_project_device", "scann_hip_txh_create_projected", "scann_hip_index_projection_info"]
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scann_hip.h")).read(), flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    build.build()
    L = hip.load()
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in hip.EXPORTS and hasattr(L, name)
        assert re.search(r"\bfn %s\s*\(" % name, doc), "INTEGRATION.md lacks " + name
    assert "project.hip" in build.SOURCES and "project.h" in build.HEADERS
    assert (hip.PROJ_MATRIX, hip.PROJ_PCA, hip.PROJ_TRUNCATE) == (pm.MATRIX, pm.PCA, pm.TRUNCATE)
    text = open(os.path.join(ROOT, "scann_rust_amd", "csrc", "project.hip")).read()
    assert "fmaf" not in text and "__builtin_amdgcn_mfma" not in text and "launch(" in text


def test_host_projection_program_passes_without_a_gpu():
    """host/projection_test: the C++ mirror's CPU project() against hand-computed values (its own main, no GPU)"""
    import subprocess
    from scann_rust_amd import build
    assert "projection_test" in build.HOST_PROGRAMS
    exe = [e for e in build.build_host() if e.endswith("projection_test")][0]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "projection_test ok" in r.stdout, r.stdout + r.stderr

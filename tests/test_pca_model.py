"""tests/pca_model.py on the CPU: its sample rule is trainer.pca_projection's, its sign rule is what the header states,
and the tolerances tests/test_gpu_pca_train.py asks of the device hold between two f64 evaluation orders of the same
rule (chunked sums and a Jacobi solve against numpy's product and eigh) -- and are missed by the two shortcuts they are
there to catch."""
import numpy as np
import pytest

from scann_rust_amd import synth, trainer
from tests import pca_model as PM

EIG_BOUND = 2.0 ** -36      # of lambda_max: tests/test_gpu_pca_train.py


def test_sample_rule_is_the_trainers():
    X = PM.rows(5000, 48, 8, 7)
    sel = PM.sample_indices(5000, 700, 42)
    assert sel.shape == (700,) and np.array_equal(
        sel, (synth.splitmix64(42 ^ 0x9CA, 0, 700) % np.uint64(5000)).astype(np.int64))
    assert np.unique(sel).size < 700          # with replacement
    assert PM.sample_indices(5000, 0, 42) is None and PM.sample_indices(5000, 5000, 42) is None
    assert PM.sample_indices(5000, 6000, 42) is None
    for ms in (700, 0, 5000):
        m = PM.train(X, 8, ms, 42)
        M, mean = trainer.pca_projection(X, 8, max_samples=ms or None, seed=42)
        assert np.array_equal(m["mean"], mean)
        same = np.all(np.abs(m["matrix"] - M) <= 2.0 ** -23, axis=1)
        flipped = np.all(np.abs(m["matrix"] + M) <= 2.0 ** -23, axis=1)
        assert np.all(same | flipped), ms       # the trainer fixes no sign


def test_sign_rule():
    V = np.array([[0.1, -0.9, 0.9], [-0.5, 0.5, 0.1], [0.0, 0.0, -1.0], [0.2, 0.3, 0.4]])
    F = PM.fix_signs(V)
    assert np.array_equal(F[0], -V[0])      # |-0.9| == |0.9|: the lower index decides, it was negative
    assert np.array_equal(F[1], -V[1])
    assert np.array_equal(F[2], -V[2])
    assert np.array_equal(F[3], V[3])
    m = PM.train(PM.rows(300, 33, 12, 3), 12)
    at = np.argmax(np.abs(m["matrix64"]), axis=1)
    assert np.all(m["matrix64"][np.arange(12), at] > 0.0)


def test_generator_has_the_gap():
    """every one of the first r eigenvalues is separated from the next: the smallest ratio lambda_j / lambda_{j+1}, j < r,
    is 1.24 .. 1.48 at the shapes of tests/test_gpu_pca_train.py (sampling noise of the 0.05 block included), so an
    eigenvector moves by about 1e-16 lambda_max / (lambda_j - lambda_{j+1}) < 1e-12 between two f64 solvers"""
    for n, dim, r, seed in ((1500, 96, 16, 1), (37, 20, 8, 2), (300, 33, 12, 3), (5000, 48, 8, 5)):
        w = PM.train(PM.rows(n, dim, r, seed), r)["eigenvalues"]
        assert (w[:r] / w[1:r + 1]).min() >= 1.2, (n, dim, r, (w[:r] / w[1:r + 1]).min())


CASES = [dict(n=1500, dim=96, r=16, seed=1), dict(n=1500, dim=96, r=16, seed=1, scale=0.01, offset=100.0),
         dict(n=1500, dim=96, r=16, seed=1, scale=1e4), dict(n=37, dim=20, r=8, seed=2), dict(n=300, dim=33, r=12, seed=3)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-%s-%s" % (c["n"], c["dim"], c.get("scale", 1), c.get("offset", 0)))
def test_tolerances_hold_between_two_f64_orders(case):
    X = PM.rows(**case)
    m = PM.train(X, case["r"])
    mean2, cov2 = PM.chunked_mean_cov(X, 128)
    assert PM.ulp_distance_f32(mean2.astype(np.float32), m["mean"]).max() <= 1
    w2, sweeps, converged = PM.jacobi_eigenvalues(cov2)
    assert converged and sweeps <= 30, sweeps
    lmax = m["eigenvalues"][0]
    assert np.abs(w2 - m["eigenvalues"]).max() <= EIG_BOUND * lmax, np.abs(w2 - m["eigenvalues"]).max() / lmax


def test_the_eigenvalue_bound_catches_the_shortcuts():
    """uncentred second moments at offset 100, scale 0.01, and f32 accumulation, both miss 2^-36 lambda_max"""
    X = PM.rows(1500, 96, 16, 1, scale=0.01, offset=100.0)
    m = PM.train(X, 16)
    X64 = X.astype(np.float64)
    mu = X64.mean(0)
    uncentred = (X64.T @ X64 - len(X) * np.outer(mu, mu)) / (len(X) - 1)
    w = np.sort(np.linalg.eigvalsh(uncentred))[::-1]
    assert np.abs(w - m["eigenvalues"]).max() > EIG_BOUND * m["eigenvalues"][0]
    Y = PM.rows(1500, 96, 16, 1)
    my = PM.train(Y, 16)
    Yc = Y - Y.mean(0, dtype=np.float32)
    w32 = np.sort(np.linalg.eigvalsh(((Yc.T @ Yc) / np.float32(len(Y) - 1)).astype(np.float64)))[::-1]
    assert np.abs(w32 - my["eigenvalues"]).max() > EIG_BOUND * my["eigenvalues"][0]


def test_integer_rows_are_exact():
    for dim in (16, 17, 40, 65, 130):
        X = PM.integer_rows(501, dim, dim)
        mean, cov, ns = PM.mean_cov(X)
        assert ns == 1002 and np.all(mean == 0.0)
        mean2, cov2 = PM.chunked_mean_cov(X, 100)
        assert np.array_equal(cov.view(np.uint64), cov2.view(np.uint64))

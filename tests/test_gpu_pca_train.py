"""scann_hip_pca_train against the rule of tests/pca_model.py (include/scann_hip.h "PCA training on the device").

A  the mean, every eigenvalue, orthonormality, the residual of every component against the model's covariance, and --
   where the spectrum is separated -- the components themselves, each within the bound the header's rule allows two f64
   evaluation orders (tests/test_pca_model.py holds the same bounds between two orders on the CPU);
B  the covariance kernel's f64 MFMA lane map and its tile and row tails, bit for bit on integer data;
C  two calls give the same bits;
D  every refusal, with the source still searching; Projection.arrays() of host-created projections."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as orc
from scann_rust_amd import hip, trainer
from tests import helpers as H
from tests import pca_model as PM

pytestmark = pytest.mark.gpu

EIG_BOUND = 2.0 ** -36        # of lambda_max, per eigenvalue
ORTHO_BOUND = 2.0 ** -22      # max |M M^T - I|, evaluated in f64: f32 rounding of unit vectors gives 2 * 2^-24
RESIDUAL_BOUND = 2.0 ** -22   # of lambda_max: ||C m_j - lambda_j m_j||_2, the same argument
COMPONENT_BOUND = 2.0 ** -23  # absolute, per element, up to the sign rule

# n, dim, stride, out_dim, r (leading columns of the generator; None: no separated spectrum to compare components on)
CASES = {
    "1500x96": dict(n=1500, dim=96, stride=96, out_dim=16, r=16, seed=1),
    "1500x96-stride100-nan": dict(n=1500, dim=96, stride=100, out_dim=16, r=16, seed=1),
    "1500x96-offset100-scale0.01": dict(n=1500, dim=96, stride=96, out_dim=16, r=16, seed=1, scale=0.01, offset=100.0),
    "1500x96-scale1e4": dict(n=1500, dim=96, stride=96, out_dim=16, r=16, seed=1, scale=1e4),
    "37x20": dict(n=37, dim=20, stride=20, out_dim=8, r=8, seed=2),                  # no multiple of 16
    "300x33-stride36": dict(n=300, dim=33, stride=36, out_dim=12, r=12, seed=3),     # odd dim: the Jacobi bye
    "2x20": dict(n=2, dim=20, stride=20, out_dim=1, r=1, seed=6),
    "1x5-zero-covariance": dict(n=1, dim=5, stride=5, out_dim=2, r=None, seed=7),
    "300x1": dict(n=300, dim=1, stride=1, out_dim=1, r=1, seed=8),
    "4096x64-full": dict(n=4096, dim=64, stride=64, out_dim=64, r=None, seed=4),     # out_dim == in_dim
    "5000x48-sampled700": dict(n=5000, dim=48, stride=48, out_dim=8, r=8, seed=5, max_samples=700),
    "5000x48-samples-above-n": dict(n=5000, dim=48, stride=48, out_dim=8, r=8, seed=5, max_samples=6000),
    # the covariance kernel's panel edge (64 columns) from above, and three panels (six panel pairs)
    "700x65-stride68": dict(n=700, dim=65, stride=68, out_dim=10, r=10, seed=9),
    "400x130": dict(n=400, dim=130, stride=130, out_dim=12, r=12, seed=10),
    # the ceiling itself (2052 is refused below): 32 panels, 528 panel pairs, 2047 rounds per sweep
    "200x2048-ceiling": dict(n=200, dim=2048, stride=2048, out_dim=4, r=4, seed=12),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    c = CASES[name]
    r = c["r"] if c["r"] is not None else c["dim"]
    X = PM.rows(c["n"], c["dim"], r, c["seed"], scale=c.get("scale", 1.0), offset=c.get("offset", 0.0))
    data = PM.strided(X, c["stride"])
    m = PM.train(X, c["out_dim"], c.get("max_samples", 0), 42)
    for a in (X, data) + tuple(v for v in m.values() if isinstance(v, np.ndarray)):
        a.setflags(write=False)
    return X, data, m


def train(name, **kw):
    c = CASES[name]
    X, data, m = reference(name)
    src = hip.bf_create(data, c["n"], c["dim"], c["stride"], hip.SQUARED_L2)
    try:
        proj, info = hip.pca_train(src, c["out_dim"], c.get("max_samples", 0), 42, want_eigenvalues=True,
                                   want_covariance=True, **kw)
    finally:
        src.close()
    try:
        M, mu = proj.arrays()
        assert proj.info() == (hip.PROJ_PCA, c["dim"], c["out_dim"], 0)
    finally:
        proj.close()
    return M, mu, info


def assert_sign_rule(M):
    M64 = M.astype(np.float64)
    at = np.argmax(np.abs(M64), axis=1)       # the first of equal maxima
    assert np.all(M64[np.arange(M.shape[0]), at] > 0.0), "a component's largest-magnitude entry is not positive"


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_model(name):
    c = CASES[name]
    X, data, m = reference(name)
    M, mu, info = train(name)
    d, od = c["dim"], c["out_dim"]
    assert M.shape == (od, d) and mu.shape == (d,)
    assert info["converged"], "the Jacobi solve did not converge in %d sweeps" % info["sweeps"]
    print("%s: %d sweeps" % (name, info["sweeps"]))
    # mean: two f64 summation orders, rounded to f32
    ulps = PM.ulp_distance_f32(mu, m["mean"]).max()
    print("mean: %d ulp" % ulps)
    assert ulps <= 1
    # eigenvalues, all in_dim of them, descending
    eig, lmax = info["eigenvalues"], m["eigenvalues"][0]
    assert np.all(np.diff(eig) <= 0.0)
    err = np.abs(eig - m["eigenvalues"]).max()
    print("eigenvalues: max error %.3g lambda_max (bound %.3g)" % (err / lmax if lmax else err, EIG_BOUND))
    assert err <= EIG_BOUND * lmax
    # the covariance the solve started from is symmetric to the bit
    cov = info["covariance"]
    assert np.array_equal(cov.view(np.uint64), cov.T.copy().view(np.uint64))
    # orthonormality and residuals of the f32 components, in f64 against the model's covariance
    M64 = M.astype(np.float64)
    ortho = np.abs(M64 @ M64.T - np.eye(od)).max()
    resid = np.linalg.norm(m["cov"] @ M64.T - M64.T * eig[:od], axis=0).max()
    print("orthonormality %.3g (bound %.3g), residual %.3g lambda_max (bound %.3g)"
          % (ortho, ORTHO_BOUND, resid / lmax if lmax else resid, RESIDUAL_BOUND))
    assert ortho <= ORTHO_BOUND
    assert resid <= RESIDUAL_BOUND * lmax
    assert_sign_rule(M)
    if c["r"] is not None:      # the separated part of the spectrum: the components themselves
        j = min(od, c["r"])
        cerr = np.abs(M64[:j] - m["matrix64"][:j]).max()
        print("components: max error %.3g (bound %.3g)" % (cerr, COMPONENT_BOUND))
        assert cerr <= COMPONENT_BOUND
    if name == "1x5-zero-covariance":
        assert np.all(eig == 0.0) and np.array_equal(M, np.eye(5, dtype=np.float32)[:2]) and info["sweeps"] == 0


@pytest.mark.parametrize("dim", [16, 17, 40, 65, 130])
def test_covariance_is_exact_on_integer_rows(dim):
    """rows [R; -R], R integer in [-8, 8], 1002 rows (2 mod 4): the mean is exactly 0 and every partial sum of the
    covariance is an integer below 2^53, so any correct lane map and any tail handling gives the model's bits.  Dims 65
    and 130 cross the 64-column panel edge: off-diagonal panel pairs, which a transposed C/D map would get wrong."""
    X = PM.integer_rows(501, dim, dim)
    mean, cov, ns = PM.mean_cov(X)
    src = hip.bf_create(X, 1002, dim, dim, hip.SQUARED_L2)
    try:
        proj, info = hip.pca_train(src, 1, want_covariance=True)
        M, mu = proj.arrays()
        proj.close()
    finally:
        src.close()
    assert np.all(mu == 0.0)
    got = info["covariance"]
    bad = np.argwhere(got.view(np.uint64) != cov.view(np.uint64))
    assert bad.size == 0, "covariance differs at %d entries, first %s: %r vs %r" % (
        len(bad), bad[0], got[tuple(bad[0])], cov[tuple(bad[0])])


@pytest.mark.parametrize("name", ["1500x96-stride100-nan", "300x33-stride36", "5000x48-sampled700"])
def test_two_calls_give_the_same_bits(name):
    a, b = train(name), train(name)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert np.array_equal(a[2]["eigenvalues"].view(np.uint64), b[2]["eigenvalues"].view(np.uint64))
    assert np.array_equal(a[2]["covariance"].view(np.uint64), b[2]["covariance"].view(np.uint64))
    assert a[2]["sweeps"] == b[2]["sweeps"] and a[2]["converged"] == b[2]["converged"]


def test_refusals_leave_the_rows_searchable():
    n, dim = 300, 16
    rows = np.random.default_rng(99).uniform(-1, 1, (n, dim)).astype(np.float32)
    st = hip.compute_stride(dim)
    data = PM.strided(rows, st, fill=0.0)
    src = hip.bf_create(data, n, dim, st, hip.SQUARED_L2)

    def refused(index, code, out_dim=4, needle=None):
        with pytest.raises(hip.ScannError) as e:
            hip.pca_train(index, out_dim)
        assert e.value.code == code, e.value
        assert needle is None or needle in e.value.message, e.value

    def still_searches():
        q = rows[:2] + np.float32(0.01)
        idx, dist, cnt = src.search_batched(q, 4)[:3]
        for i in range(2):
            oi, od = orc.bf_search(data, n, dim, st, hip.SQUARED_L2, q[i], 4)
            H.assert_topk_equal_up_to_ties(idx[i, :cnt[i]], dist[i, :cnt[i]], oi, od, what="source q%d" % i)

    for od in (0, dim + 1):
        refused(src, hip.INVALID_ARGUMENT, out_dim=od)
        still_searches()
    # not an f32 brute-force handle: a tree handle, a quantized brute-force handle
    tree, _ = hip.txh_build(src, num_partitions=4, num_subspaces=8, num_codes=16)
    refused(tree, hip.INVALID_ARGUMENT)
    tree.close()
    bf16 = (np.ascontiguousarray(data).view(np.uint32) >> 16).astype(np.uint16)
    qix = hip.bf_create_quantized(bf16, n, dim, st, hip.ROWS_BF16, hip.SQUARED_L2)
    refused(qix, hip.INVALID_ARGUMENT)
    qix.close()
    still_searches()
    empty = hip.bf_create(np.zeros((0, st), np.float32), 0, dim, st, hip.SQUARED_L2)
    refused(empty, hip.INVALID_ARGUMENT)
    empty.close()
    # in_dim above the ceiling: ResourceExhausted, the message naming the limit
    wide = hip.bf_create(np.zeros((4, 2056), np.float32), 4, 2052, 2056, hip.SQUARED_L2)
    refused(wide, hip.RESOURCE_EXHAUSTED, needle="2048")
    wide.close()
    # ... and the source trains after all of that
    proj, info = hip.pca_train(src, 4)
    assert info["converged"] and proj.info() == (hip.PROJ_PCA, dim, 4, 0)
    proj.close()
    still_searches()
    src.close()


def test_arrays_of_host_created_projections():
    rng = np.random.default_rng(5)
    M = trainer.random_orthogonal(24, 8, 3)
    mu = rng.standard_normal(24).astype(np.float32)
    p = hip.Projection(hip.PROJ_PCA, matrix=M, mean=mu)
    gm, gmu = p.arrays()
    assert np.array_equal(gm.view(np.uint32), M.view(np.uint32)) and np.array_equal(gmu.view(np.uint32), mu.view(np.uint32))
    p.close()
    p = hip.Projection(hip.PROJ_MATRIX, matrix=M)
    gm, gmu = p.arrays()
    assert np.array_equal(gm.view(np.uint32), M.view(np.uint32)) and gmu is None
    p.close()
    p = hip.Projection(hip.PROJ_TRUNCATE, in_dim=24, out_dim=8, start=3)
    assert p.arrays() == (None, None)
    p.close()


def test_a_trained_projection_is_a_created_one():
    """the trained object projects as a projection created from its own arrays does, bit for bit"""
    X, data, m = reference("300x33-stride36")
    c = CASES["300x33-stride36"]
    src = hip.bf_create(data, c["n"], c["dim"], c["stride"], hip.SQUARED_L2)
    proj, _ = hip.pca_train(src, c["out_dim"])
    src.close()
    M, mu = proj.arrays()
    twin = hip.Projection(hip.PROJ_PCA, matrix=M, mean=mu)
    a, b = proj.project(X), twin.project(X)
    proj.close()
    twin.close()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))

"""scann_hip_opq_train and its two primitives (include/scann_hip.h "OPQ training on the device").

1  the fused-decode cross-covariance kernel, bit for bit on integer data: lane map, decode, panel and row tails;
2  the one-sided Jacobi polar factor against numpy.linalg.svd;
3  the alternation: a non-increasing distortion that drops as tests/opq_model.py's does, the stop rule, a projected
   build with the trained rotation;
4  every refusal, with the source still searching and training afterwards."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as orc
from scann_rust_amd import hip, trainer
from tests import helpers as H
from tests import opq_model as OM

pytestmark = pytest.mark.gpu

ELEMENT_BOUND = 2.0 ** -23    # |R - U V^T| per element: f32 rounding of entries below 1 (tests/test_gpu_pca_train.py)
ORTHO_BOUND = 2.0 ** -22      # max |R R^T - I| in f64: the same argument, two factors
SIGMA_BOUND = 2.0 ** -36      # of sigma_max, per singular value


def bf(X):
    X = np.ascontiguousarray(X, np.float32)
    return hip.bf_create(X, X.shape[0], X.shape[1], X.shape[1], hip.SQUARED_L2)


def ortho_error(P):
    P64 = P.astype(np.float64)
    return np.abs(P64 @ P64.T - np.eye(P.shape[0])).max()


# ---- 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,S,K,packed4,n", [
    (16, 4, 16, 1, 1002),     # basic, 4-bit packed codes
    (17, 1, 16, 0, 1002),     # d and dsub = 17 divide nothing
    (40, 8, 256, 0, 1002),    # byte codes
    (65, 13, 16, 1, 1002),    # odd S: a padded nibble; crosses a panel edge
    (130, 26, 32, 0, 403),    # three panels; a panel cuts a subspace
    (96, 8, 16, 1, 37),       # dsub = 12 across 16-wide tiles; n below one LDS stage
])
def test_cross_covariance_is_exact_on_integer_rows(d, S, K, packed4, n):
    """X, the codebook: integers in [-8, 8]; every partial sum is an integer below 2^53, so any correct lane map, decode
    and tail handling gives numpy's bits"""
    rng = np.random.default_rng(d * 1000 + n)
    X = rng.integers(-8, 9, (n, d)).astype(np.float32)
    cb = rng.integers(-8, 9, (S, K, d // S)).astype(np.float32)
    codes = rng.integers(0, K, (n, S)).astype(np.uint8)
    Yhat = np.concatenate([cb[s][codes[:, s]] for s in range(S)], 1).astype(np.float64)
    want = X.astype(np.float64).T @ Yhat
    src = bf(X)
    try:
        got = hip.opq_cross_covariance(src, cb, trainer.pack4(codes) if packed4 else codes, packed4=bool(packed4))
    finally:
        src.close()
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, "M differs at %d entries, first %s: %r vs %r" % (
        len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


# ---- 2 ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conditioned(d, log2_min):
    """M = A diag(sigma) B, A and B random orthogonal, sigma log-uniform in [2^log2_min, 1] with both ends present"""
    rng = np.random.default_rng(d)
    A, B = (np.linalg.qr(rng.standard_normal((d, d)))[0] for _ in range(2))
    sigma = np.exp2(rng.uniform(log2_min, 0.0, d))
    sigma[0], sigma[-1] = 1.0, 2.0 ** log2_min
    M = (A * sigma) @ B
    U, sv, Vt = np.linalg.svd(M)
    for a in (M, sv):
        a.setflags(write=False)
    return M, U @ Vt, sv


@pytest.mark.parametrize("d", [1, 2, 20, 33, 96, 130, 2048])
def test_polar_factor_well_conditioned(d):
    M, want, sv = conditioned(d, -10.0 if d > 1 else 0.0)
    R, info = hip.opq_polar(M)
    err, ortho = np.abs(R.astype(np.float64) - want).max(), ortho_error(R)
    serr = np.abs(info["singular"] - sv).max() / sv[0]
    print("d=%d: %d sweeps, element %.3g (bound %.3g), orthonormality %.3g (bound %.3g), sigma %.3g sigma_max (bound %.3g)"
          % (d, info["sweeps"], err, ELEMENT_BOUND, ortho, ORTHO_BOUND, serr, SIGMA_BOUND))
    assert info["converged"], "the Jacobi solve did not converge in %d sweeps" % info["sweeps"]
    assert err <= ELEMENT_BOUND and ortho <= ORTHO_BOUND and serr <= SIGMA_BOUND


def test_polar_factor_ill_conditioned():
    d = 32
    M, want, sv = conditioned(d, -20.0)
    R, info = hip.opq_polar(M)
    R2, info2 = hip.opq_polar(M)
    ortho, trace = ortho_error(R), np.trace(R.astype(np.float64).T @ M)
    print("orthonormality %.3g (bound %.3g), trace %.17g of %.17g" % (ortho, ORTHO_BOUND, trace, sv.sum()))
    assert ortho <= ORTHO_BOUND
    assert trace >= (1.0 - d * 2.0 ** -23) * sv.sum()
    assert np.array_equal(R.view(np.uint32), R2.view(np.uint32))
    assert np.array_equal(info["singular"].view(np.uint64), info2["singular"].view(np.uint64))


@pytest.mark.parametrize("what", ["zero", "zero-column"])
def test_polar_reports_a_singular_matrix(what):
    M = np.zeros((12, 12)) if what == "zero" else np.array(conditioned(20, -10.0)[0])
    if what == "zero-column":
        M[:, 7] = 0.0
    R, info = hip.opq_polar(M)
    assert info["singular"][-1] == 0.0 and np.all(np.isfinite(R))
    assert (info["singular"][0] == 0.0) == (what == "zero")


# ---- 3 ---------------------------------------------------------------------------------------------------------------
# (n, d, S, K).  The second case was written down as (1500, 24, 6, 16); 6 LUT16 subspaces is a shape scann_hip_txh_build
# refuses, and so, by its own rule, does scann_hip_opq_train (test_refusals below).  It runs at an accepted shape with n,
# d and T as given and the model's premise intact: (S, K) = (4, 32), the byte-code route (the model's ratio is 0.66; at
# (8, 16), dsub = 3, it is 0.86 after 8 iterations, above the 0.8 the check asks of its inputs).
ALTERNATION = [(2000, 32, 8, 16), (1500, 24, 4, 32)]
T, TRAINING_ITERATIONS, DATA_SEED = 8, 10, 7


@functools.lru_cache(maxsize=None)
def model_ratio(n, d, S, K):
    _, dist, smallest = OM.opq_model(OM.near_copy_rows(n, d, DATA_SEED), S, K, T, TRAINING_ITERATIONS)
    assert smallest > 0 and dist[-1] / dist[0] <= 0.8    # the inputs' own premise (0.59 and 0.66 when they were chosen)
    return dist[-1] / dist[0]


@pytest.mark.parametrize("n,d,S,K", ALTERNATION)
def test_alternation_lowers_the_distortion(n, d, S, K):
    src = bf(OM.near_copy_rows(n, d, DATA_SEED))
    try:
        proj, rep = hip.opq_train(src, num_subspaces=S, num_codes=K, opq_iterations=T,
                                  training_iterations=TRAINING_ITERATIONS)
    finally:
        src.close()
    P = proj.arrays()[0]
    assert proj.info() == (hip.PROJ_MATRIX, d, d, 0)
    proj.close()
    dist, rho = np.array(rep["distortion"]), model_ratio(n, d, S, K)
    print("distortion %s, ratio %.4f (model %.4f), sweeps %s, sigma_min/max %s, stage_ms %s"
          % (np.round(dist, 4), dist[-1] / dist[0], rho, rep["sweeps"], rep["sigma_min_over_max"], hip.opq_last_stage_ms()))
    assert rep["iterations_run"] == T and not rep["stopped_singular"] and all(rep["converged"])
    assert np.all(dist[1:] <= dist[:-1] * (1.0 + 2.0 ** -16))
    assert ortho_error(P) <= ORTHO_BOUND
    assert dist[-1] / dist[0] <= (1.0 + rho) / 2.0


def test_a_singular_cross_covariance_stops_the_training():
    X = np.array(OM.near_copy_rows(600, 16, 3))
    X[:, 5] = 0.0
    init = hip.Projection(hip.PROJ_MATRIX, matrix=trainer.random_orthogonal(16, 16, 1))
    src = bf(X)
    try:
        proj, rep = hip.opq_train(src, init=init, num_subspaces=8, num_codes=16, opq_iterations=4, training_iterations=5)
    finally:
        src.close()
    assert rep["stopped_singular"] and rep["iterations_run"] == 0 and rep["sigma_min_over_max"][0] <= 2.0 ** -40
    assert np.array_equal(proj.arrays()[0].view(np.uint32), init.arrays()[0].view(np.uint32))
    proj.close()
    init.close()


def test_a_projected_build_takes_the_trained_rotation():
    n, d = 1500, 24
    X = OM.near_copy_rows(n, d, DATA_SEED)
    src = bf(X)
    proj, _ = hip.opq_train(src, num_subspaces=8, num_codes=16, opq_iterations=3, training_iterations=5, max_samples=1000)
    twin = hip.Projection(hip.PROJ_MATRIX, matrix=proj.arrays()[0])
    assert np.array_equal(proj.project(X).view(np.uint32), twin.project(X).view(np.uint32))
    twin.close()
    index, _ = hip.txh_build_projected(src, proj, num_partitions=8, num_subspaces=8, num_codes=16, partitions_to_search=8)
    proj.close()
    src.close()
    o = hip.default_opts()
    o.pre_reorder_k = 100
    idx, dist, cnt = index.search_batched(X, 1, o)[:3]
    index.close()
    assert np.all(cnt == 1) and np.all(dist[:, 0] == 0.0)
    assert np.array_equal(idx[:, 0], np.arange(n, dtype=np.uint32))


# ---- 4 ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_rows_searchable():
    n, dim = 300, 16
    rows = np.random.default_rng(99).uniform(-1, 1, (n, dim)).astype(np.float32)
    src = bf(rows)
    good = dict(num_subspaces=8, num_codes=16, opq_iterations=2, training_iterations=3)

    def refused(index, code, needle=None, init=None, **cfg):
        with pytest.raises(hip.ScannError) as e:
            hip.opq_train(index, init=init, **dict(good, **cfg))
        assert e.value.code == code, e.value
        assert needle is None or needle in e.value.message, e.value

    def still_searches():
        q = rows[:2] + np.float32(0.01)
        idx, dist, cnt = src.search_batched(q, 4)[:3]
        for i in range(2):
            oi, od = orc.bf_search(rows, n, dim, dim, hip.SQUARED_L2, q[i], 4)
            H.assert_topk_equal_up_to_ties(idx[i, :cnt[i]], dist[i, :cnt[i]], oi, od, what="source q%d" % i)

    # not an f32 brute-force handle, an empty one, one above the ceiling: scann_hip_pca_train's refusals
    tree, _ = hip.txh_build(src, num_partitions=4, num_subspaces=8, num_codes=16)
    refused(tree, hip.INVALID_ARGUMENT)
    tree.close()
    bf16 = (rows.view(np.uint32) >> 16).astype(np.uint16)
    qix = hip.bf_create_quantized(bf16, n, dim, dim, hip.ROWS_BF16, hip.SQUARED_L2)
    refused(qix, hip.INVALID_ARGUMENT)
    qix.close()
    empty = hip.bf_create(np.zeros((0, dim), np.float32), 0, dim, dim, hip.SQUARED_L2)
    refused(empty, hip.INVALID_ARGUMENT)
    empty.close()
    wide = hip.bf_create(np.zeros((4, 2056), np.float32), 4, 2056, 2056, hip.SQUARED_L2)
    refused(wide, hip.RESOURCE_EXHAUSTED, needle="2048")
    wide.close()
    still_searches()
    # the shapes the build refuses, with the build's status
    refused(src, hip.INVALID_ARGUMENT, num_subspaces=5)          # dim % S
    refused(src, hip.INVALID_ARGUMENT, num_subspaces=0)
    refused(src, hip.UNIMPLEMENTED, num_subspaces=4)             # LUT16 wants a multiple of 8
    six = bf(rows[:, :12])
    refused(six, hip.UNIMPLEMENTED, num_subspaces=6)
    six.close()
    refused(src, hip.UNIMPLEMENTED, num_subspaces=2, num_codes=256)
    refused(src, hip.UNIMPLEMENTED, num_codes=257)
    for it in (0, 65):
        refused(src, hip.INVALID_ARGUMENT, opq_iterations=it)
    still_searches()
    # init: not a MATRIX projection, not d x d
    for bad in (hip.Projection(hip.PROJ_TRUNCATE, in_dim=dim, out_dim=dim, start=0),
                hip.Projection(hip.PROJ_PCA, matrix=np.eye(dim, dtype=np.float32), mean=np.zeros(dim, np.float32)),
                hip.Projection(hip.PROJ_MATRIX, matrix=trainer.random_orthogonal(dim, 8, 1)),
                hip.Projection(hip.PROJ_MATRIX, matrix=np.eye(dim + 8, dtype=np.float32))):
        refused(src, hip.INVALID_ARGUMENT, init=bad)
        bad.close()
    still_searches()
    # ... and the source trains after all of that
    proj, rep = hip.opq_train(src, **good)
    assert rep["iterations_run"] == 2 and proj.info() == (hip.PROJ_MATRIX, dim, dim, 0)
    proj.close()
    still_searches()
    src.close()

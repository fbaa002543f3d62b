"""Numpy restatement of the reference's projections (include/scann_hip.h "projections"): every dense
projection is one loop (pca.rs:156-180, random.rs:82-92, 157-167, opq.rs:179-194)

    out[j] = 0.0f;  for i in 0..in_dim (ascending):  out[j] += (in[i] - mean[i]) * M[(i, j)]

an f32 sum whose every step is a multiply and then an add.  Below the multiply and the add are separate ufunc calls on
float32 arrays, so each step rounds once, as the reference does; the subtraction is applied for PCA alone; TRUNCATE
(and an untrained PcaProjection) is a slice.  The checker of tests/test_gpu_projection.py and
tests/test_gpu_projected_search.py, and the data families they share."""
import numpy as np

MATRIX, PCA, TRUNCATE = 1, 2, 3   # SCANN_HIP_PROJ_*


def project(kind, X, M=None, mean=None, start=0, out_dim=None, descending=False):
    """X [n, in_dim] f32 -> [n, out_dim] f32.  M [out_dim, in_dim] (row j = column j of the reference's DMatrix).
    descending: walk i from in_dim - 1 down (NOT the reference's order: the order-sensitivity tests use it)."""
    X = np.ascontiguousarray(X, np.float32)
    if kind == TRUNCATE:
        return np.ascontiguousarray(X[:, start:start + out_dim])
    M = np.ascontiguousarray(M, np.float32)
    assert M.shape[1] == X.shape[1]
    if kind == PCA:
        mean = np.ascontiguousarray(mean, np.float32)
    acc = np.zeros((X.shape[0], M.shape[0]), np.float32)
    order = range(X.shape[1] - 1, -1, -1) if descending else range(X.shape[1])
    with np.errstate(all="ignore"):
        for i in order:
            x = X[:, i:i + 1]
            if kind == PCA:
                x = np.subtract(x, mean[i])
            p = np.multiply(x, M[:, i])
            acc = np.add(acc, p)
    assert acc.dtype == np.float32
    return acc


def bits_equal(a, b):
    """bitwise equality of two f32 arrays, NaNs comparing as NaN (any payload)"""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


# ---- data families of the GPU tests ------------------------------------------------------------------------------------
FAMILIES = ("normal", "mixed-scale", "subnormal", "overflow", "big-mean")
ORDER_SENSITIVE = ("normal", "mixed-scale", "big-mean")   # families on which a wrong summation order must show


def family(name, n, in_dim, out_dim, seed):
    """(X [n, in_dim], M [out_dim, in_dim], mean [in_dim]) of one family, float32.
    normal       signed standard normal rows, a standard normal matrix with per-row magnitudes 2^-3 .. 2^3
    mixed-scale  column i of X scaled by 10^e, e spread over -20 .. 20; the matrix unscaled normal
    subnormal    rows in the f32 subnormal range (products flush nowhere: subnormals are kept)
    overflow     rows of 1e36 with up to two elements of 3e38, a matrix of +-(1..2): finite sums, +-inf, and inf - inf = NaN
    big-mean     100 + 0.01 U rows and the mean 100 + 0.005: the centring cancels seven digits"""
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((out_dim, in_dim)).astype(np.float32)
    mean = rng.standard_normal(in_dim).astype(np.float32)
    if name == "normal":
        X = rng.standard_normal((n, in_dim)).astype(np.float32)
        M = M * np.exp2(rng.integers(-3, 4, (out_dim, 1))).astype(np.float32)
    elif name == "mixed-scale":
        e = np.linspace(-20.0, 20.0, in_dim) if in_dim > 1 else np.zeros(1)
        scale = 10.0 ** rng.permutation(e)
        X = (rng.standard_normal((n, in_dim)) * scale).astype(np.float32)
        mean = (mean * scale).astype(np.float32)   # (a mean of the columns' own magnitudes: an O(1) one would vanish)
    elif name == "subnormal":
        X = (rng.standard_normal((n, in_dim)) * 1e-41).astype(np.float32)
        mean = (mean * np.float32(1e-41)).astype(np.float32)
    elif name == "overflow":
        X = (rng.standard_normal((n, in_dim)) * 1e36).astype(np.float32)
        M = (np.where(M < 0, -1.0, 1.0) * rng.uniform(1.0, 2.0, M.shape)).astype(np.float32)
        # row r carries r % 3 elements of 3e38: none (a large finite sum), one (+-inf), two (inf - inf where the signs
        # of the two products differ)
        for r in range(n):
            for c in rng.choice(in_dim, min(r % 3, in_dim), replace=False):
                X[r, c] = np.float32(3.0e38)
    elif name == "big-mean":
        X = (100.0 + 0.01 * rng.random((n, in_dim))).astype(np.float32)
        mean = np.full(in_dim, 100.005, np.float32)
    else:
        raise ValueError(name)
    return X, np.ascontiguousarray(M, np.float32), mean

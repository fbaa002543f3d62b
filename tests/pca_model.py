"""The rule of scann_hip_pca_train (include/scann_hip.h "PCA training on the device") in f64 numpy, and the data its
tests train on.  The solver here is numpy.linalg.eigh, not the device's Jacobi sweep: eigenvalues, the invariant
subspace and -- where the spectrum is separated -- the sign-fixed components are properties of the covariance, not of the
solver, and the tests compare those."""
import numpy as np

from scann_rust_amd import synth

SAMPLE_SALT = 0x9CA


def sample_indices(n, max_samples, seed):
    """None: every row in order (max_samples == 0 or >= n); else the ns = max_samples indices, with replacement"""
    if max_samples == 0 or max_samples >= n:
        return None
    return (synth.splitmix64(seed ^ SAMPLE_SALT, 0, max_samples) % np.uint64(n)).astype(np.int64)


def fix_signs(V):
    """rows of V: each sign such that the largest-magnitude entry (lowest index on ties) is positive"""
    V = np.array(V, np.float64)
    for v in V:
        at = int(np.argmax(np.abs(v)))      # argmax returns the first of equal maxima
        if v[at] < 0.0:
            v *= -1.0
    return V


def mean_cov(X, max_samples=0, seed=42):
    """(mean f64 [d], covariance f64 [d, d], ns) of the sampled rows: two passes, centred with the unrounded mean"""
    X = np.ascontiguousarray(X, np.float32)
    sel = sample_indices(X.shape[0], max_samples, seed)
    if sel is not None:
        X = X[sel]
    X64 = X.astype(np.float64)
    mean = X64.sum(0) / X64.shape[0]
    Xc = X64 - mean
    return mean, (Xc.T @ Xc) / max(1, X64.shape[0] - 1), X64.shape[0]


def train(X, out_dim, max_samples=0, seed=42):
    """dict(mean64, mean f32, cov, eigenvalues f64 [d] descending, matrix f32 [out_dim, d], matrix64)"""
    mean, cov, ns = mean_cov(X, max_samples, seed)
    w, V = np.linalg.eigh(cov)
    order = np.argsort(-w, kind="stable")           # ties: lower column first
    comps = fix_signs(V[:, order[:out_dim]].T)
    return dict(mean64=mean, mean=mean.astype(np.float32), cov=cov, eigenvalues=w[order], matrix64=comps,
                matrix=comps.astype(np.float32), ns=ns)


def chunked_mean_cov(X, chunk):
    """another f64 evaluation order of mean_cov over all rows: per-chunk sums added in ascending order (what a device
    that splits the rows into runs does)"""
    X64 = np.ascontiguousarray(X, np.float32).astype(np.float64)
    n, d = X64.shape
    s = np.zeros(d)
    for r in range(0, n, chunk):
        s = s + X64[r:r + chunk].sum(0)
    mean = s / n
    C = np.zeros((d, d))
    for r in range(0, n, chunk):
        Xc = X64[r:r + chunk] - mean
        C = C + Xc.T @ Xc
    return mean, C / max(1, n - 1)


def jacobi_eigenvalues(C, max_sweeps=30):
    """cyclic Jacobi (row-cyclic order) on a copy of C until off(A) <= 2^-46 ||C||_F, the off-diagonal norm summed from
    the off-diagonal entries: (eigenvalues descending, sweeps, converged).  The second evaluation order of the
    eigenvalue tolerance; small dims only."""
    A = np.array(C, np.float64)
    d = A.shape[0]
    tol = np.ldexp(np.sqrt((A * A).sum()), -46)

    def off():
        return np.sqrt(2.0 * (np.triu(A, 1) ** 2).sum())

    sweeps = 0
    while off() > tol and sweeps < max_sweeps:
        for p in range(d - 1):
            for q in range(p + 1, d):
                if A[p, q] == 0.0:
                    continue
                tau = (A[q, q] - A[p, p]) / (2.0 * A[p, q])
                t = np.copysign(1.0, tau) / (abs(tau) + np.sqrt(1.0 + tau * tau))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = t * c
                rp, rq = A[p].copy(), A[q].copy()           # J^T A, J = [[c, s], [-s, c]] in (p, q)
                A[p], A[q] = c * rp - s * rq, s * rp + c * rq
                cp, cq = A[:, p].copy(), A[:, q].copy()     # (J^T A) J
                A[:, p], A[:, q] = c * cp - s * cq, s * cp + c * cq
                A[p, q] = A[q, p] = 0.0
        sweeps += 1
    return np.sort(np.diag(A))[::-1], sweeps, bool(off() <= tol)


def rows(n, dim, r, seed, scale=1.0, offset=0.0):
    """N(0, 1) rows, column i scaled by 2 * 0.8^i for i < r and by 0.05 after, rotated by a seeded random orthogonal
    matrix, then scaled and offset, cast to f32: a spectral gap lambda_r / lambda_{r+1} >= 1.38 at the tests' shapes"""
    rng = np.random.default_rng(seed)
    sd = np.full(dim, 0.05)
    sd[:r] = 2.0 * 0.8 ** np.arange(r)
    Q, _ = np.linalg.qr(rng.standard_normal((dim, dim)))
    X = (rng.standard_normal((n, dim)) * sd) @ Q.T
    return (X * scale + offset).astype(np.float32)


def strided(X, stride, fill=np.nan):
    """[n, stride] f32 with X in the leading columns and `fill` in the padding"""
    X = np.ascontiguousarray(X, np.float32)
    out = np.full((X.shape[0], stride), fill, np.float32)
    out[:, :X.shape[1]] = X
    return out


def integer_rows(half, dim, seed):
    """[R; -R] with R integer-valued in [-8, 8]: the mean is exactly 0 and every sum of the covariance is exact in f64"""
    R = np.random.default_rng(seed).integers(-8, 9, (half, dim)).astype(np.float32)
    return np.concatenate([R, -R], 0)


def ulp_distance_f32(a, b):
    """|a - b| in units in the last place of f32, per element (finite values)"""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))

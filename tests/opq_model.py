"""The rule of scann_hip_opq_train in numpy f64 (include/scann_hip.h "OPQ training on the device"), with a k-means
seeding of its own: the device's distortion trace is compared with this one by its overall drop, never element-wise."""
import numpy as np


def near_copy_rows(n, d, seed):
    """g ~ N(0, I_{d/2}), row = [g, g + 0.05 noise]: every dimension has a near-copy in another subspace."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, d // 2))
    return np.concatenate([g, g + 0.05 * rng.standard_normal((n, d // 2))], 1).astype(np.float32)


def _assign(ys, c):
    return ((ys[:, None, :] - c[None]) ** 2).sum(2).argmin(1)


def _lloyd_step(ys, c):
    """one Lloyd step in place; returns the smallest cluster size it saw"""
    a = _assign(ys, c)
    cnt = np.bincount(a, minlength=c.shape[0])
    sums = np.zeros_like(c)
    np.add.at(sums, a, ys)
    c[cnt > 0] = sums[cnt > 0] / cnt[cnt > 0, None]
    return int(cnt.min())


def opq_model(X, S, K, T, training_iterations, inner_iterations=1, seed=42):
    """(R f64 [d, d], distortion [T], smallest cluster any Lloyd step or encode saw)"""
    X = np.asarray(X, np.float64)
    n, d = X.shape
    dsub, R, cb, dist, smallest = d // S, np.eye(d), None, [], n
    for t in range(T):
        Y, Yhat = X @ R, np.empty((n, d))
        if cb is None:
            rng = np.random.default_rng(seed)
            cb = [Y[rng.choice(n, K, replace=False), s * dsub:(s + 1) * dsub].copy() for s in range(S)]
        for s in range(S):
            ys = Y[:, s * dsub:(s + 1) * dsub]
            for _ in range(inner_iterations if t else training_iterations):
                smallest = min(smallest, _lloyd_step(ys, cb[s]))
            a = _assign(ys, cb[s])
            smallest = min(smallest, int(np.bincount(a, minlength=K).min()))
            Yhat[:, s * dsub:(s + 1) * dsub] = cb[s][a]
        dist.append(float(((Y - Yhat) ** 2).sum() / n))
        U, sv, Vt = np.linalg.svd(X.T @ Yhat)
        if sv[-1] <= np.ldexp(sv[0], -40):
            break
        R = U @ Vt
    return R, dist, smallest

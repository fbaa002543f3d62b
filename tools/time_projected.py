#!/usr/bin/env python3
"""Times the projection kernel and a projected index against a plain one (scann_hip_txh_create_projected).

    python tools/time_projected.py                       # 1M x 768 -> 128, batch 1024, k = 10
    python tools/time_projected.py --num-points 50000 --leaves 100     # a quick look

Data (stated because recall depends on it): rows and queries are N(0, diag(sd^2)) with sd_i = (1 + i)^-1/2, rotated by
one orthonormal basis (the QR of a Gaussian matrix), generated on the GPU by torch with seeds 42 (basis), 43 (rows) and
44 (queries): a decaying spectrum, 75 % of the variance (H_128 / H_768) in the 128 leading components at dim 768.

(a) scann_hip_project_device, PCA dim -> out_dim, on all n rows and on 1024 rows: medians of repeated calls, with the
    arithmetic next to them (n * dim * out_dim multiply-adds as separate mul and add on the f32 VALU; the rows read once).
(b) search, one process, interleaved rounds through the device entry point:
      plain      the index over the original rows: S = 64 (the LUT16 ceiling), K = 16, L leaves, P probed;
      projected  PCA dim -> out_dim, S = 32, the same L / P / m, re-rank at dim.
    Each with recall10@10 against the exact ground truth of the original rows.
One JSON line per measurement.  Index building uses torch on the GPU as harness plumbing (k-means assignment GEMMs);
the projection and the searches are libscann_hip.so only."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def spectrum(n, dim, basis, seed, dev):
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    sd = (1.0 + torch.arange(dim, device=dev, dtype=torch.float32)) ** -0.5
    out = torch.empty((n, dim), dtype=torch.float32, device=dev)
    for r0 in range(0, n, 131072):
        r1 = min(n, r0 + 131072)
        out[r0:r1] = (torch.randn((r1 - r0, dim), generator=g, device=dev) * sd) @ basis.T
    return out


def build_index(Xs, S, L, P, iters):
    """txh_create's keyword arguments (without rows) of an index over the device rows Xs"""
    import torch
    from scann_rust_amd import hip, trainer
    from sweep_txh import kmeans_torch
    n, dim = Xs.shape
    C, assign = kmeans_torch(Xs, L, iters, 42)
    order = torch.argsort(assign, stable=True)
    leaf_off = np.zeros(L + 1, np.uint32)
    leaf_off[1:] = np.cumsum(torch.bincount(assign, minlength=L).cpu().numpy())
    centers = C.cpu().numpy().astype(np.float32)
    leaf_of_row = assign[order].cpu().numpy().astype(np.uint32)
    csr = Xs[order]
    step = max(1, n // 32768)
    res = (csr[::step] - C[assign[order][::step]]).cpu().numpy()
    cb = trainer.train_codebook(res, S, 16, iters=8, seed=42, sample=1 << 30)
    codes = hip.encode(cb, np.ascontiguousarray(csr.cpu().numpy()), stride=dim, centers=centers, leaf_of_row=leaf_of_row)
    return dict(dim=dim, centers=centers, leaf_offsets=leaf_off, leaf_ids=order.cpu().numpy().astype(np.uint32),
                codebook=cb, codes=codes, use_residuals=True, partitions_to_search=P, pre_reorder_multiplier=3.0)


def median_ms(fn, steps, rounds):
    import torch
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / steps * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-points", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--out-dim", type=int, default=128)
    ap.add_argument("--leaves", type=int, default=1000)
    ap.add_argument("--P", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--m", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--kmeans-iters", type=int, default=6)
    ap.add_argument("--json", default="", help="also append the lines to this file")
    a = ap.parse_args()
    import torch
    from scann_rust_amd import hip, trainer
    Lh = hip.load()
    dev = torch.device("cuda", 0)
    n, dim, od, L, Q, k = a.n, a.dim, a.out_dim, a.leaves, a.batch, a.k
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    t0 = time.time()
    g = torch.Generator(device=dev)
    g.manual_seed(42)
    basis, _ = torch.linalg.qr(torch.randn((dim, dim), generator=g, device=dev))
    X = spectrum(n, dim, basis, 43, dev)
    qd = spectrum(Q, dim, basis, 44, dev)
    rows, qs = X.cpu().numpy(), qd.cpu().numpy()
    bf = hip.bf_create(rows, n, dim, dim, hip.SQUARED_L2)
    ne = min(256, Q)
    truth, _, _ = bf.search_batched(qs[:ne], k)
    bf.close()
    M, mean = trainer.pca_projection(rows[:: max(1, n // 32768)], od)
    proj = hip.Projection(hip.PROJ_PCA, matrix=M, mean=mean)
    print("data, ground truth, PCA %.1fs" % (time.time() - t0), file=sys.stderr, flush=True)

    # ---- (a) the projection kernel --------------------------------------------------------------------------------
    sptr = torch.cuda.current_stream().cuda_stream
    Xp = torch.empty((n, od), dtype=torch.float32, device=dev)
    for rows_n in (n, min(n, 1024)):
        fn = lambda: proj.project_device(X.data_ptr(), rows_n, dim, Xp.data_ptr(), od, stream=sptr)
        for _ in range(3):
            fn()
        med, lo, hi = median_ms(fn, 10 if rows_n == n else 200, a.rounds)
        macs = rows_n * dim * od
        emit({"what": "project_device", "kind": "pca", "n": rows_n, "in_dim": dim, "out_dim": od, "ms": round(med, 4),
              "ms_min": round(lo, 4), "ms_max": round(hi, 4), "mul_add_pairs": macs,
              "valu_tflops": round(2.0 * macs / (med * 1e-3) / 1e12, 2), "rows_gb": round(rows_n * dim * 4 / 1e9, 3),
              "rows_gb_per_s": round(rows_n * dim * 4 / (med * 1e-3) / 1e9, 1)})
    proj.project_device(X.data_ptr(), n, dim, Xp.data_ptr(), od, stream=sptr)
    torch.cuda.synchronize()

    # ---- (b) plain against projected ------------------------------------------------------------------------------
    t0 = time.time()
    plain = hip.txh_create(data=rows, n_rows=n, stride=dim, **build_index(X, 64, L, a.P, a.kmeans_iters))
    del X
    projected = hip.txh_create_projected(projection=proj, rows=rows, n_rows=n, row_dim=dim, row_stride=dim,
                                         **build_index(Xp, 32, L, a.P, a.kmeans_iters))
    print("index builds %.1fs" % (time.time() - t0), file=sys.stderr, flush=True)
    o = hip.default_opts()
    o.pre_reorder_k = a.m
    o.partitions_to_search = a.P
    oi = torch.empty((Q, k), dtype=torch.int32, device=dev)
    odist = torch.empty((Q, k), dtype=torch.float32, device=dev)
    oc = torch.empty((Q,), dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(sptr)
    handles = [("plain", 64, plain), ("projected", 32, projected)]

    def run(ix):
        hip.check(Lh.scann_hip_search_batched_device(ix.h, p(qd), Q, dim, k, ctypes.byref(o), p(oi), p(odist), p(oc), st))

    for _, _, ix in handles:
        hip.check(Lh.scann_hip_index_reserve(ix.h, Q, k, ctypes.byref(o)))
        for _ in range(5):
            run(ix)
        torch.cuda.synchronize()
        hip.check(Lh.scann_hip_index_last_device_status(ix.h, st))
    times = {name: [] for name, _, _ in handles}
    for _ in range(a.rounds):          # interleaved: every round times every handle
        for name, _, ix in handles:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                run(ix)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    for name, S, ix in handles:
        gi, _, _ = ix.search_batched(qs[:ne], k, o)
        rec = sum(len(set(gi[i].tolist()) & set(truth[i].tolist())) for i in range(ne)) / (ne * float(k))
        t = sorted(times[name])
        emit({"what": "search", "index": name, "n": n, "dim": dim, "index_dim": od if name == "projected" else dim, "S": S,
              "leaves": L, "P": a.P, "nq": Q, "k": k, "m": a.m, "step_ms": round(t[len(t) // 2], 4),
              "step_ms_min": round(t[0], 4), "step_ms_max": round(t[-1], 4), "qps": round(Q / (t[len(t) // 2] * 1e-3), 1),
              "recall10at10": round(rec, 4), "device_bytes": ix.device_bytes()})
    if a.json:
        with open(a.json, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the re-rank over quantized rows (scann_hip_txh_create_quantized): an f32 handle and bf16, FP8
E4M3 and int8 handles over the same rows, quantized by the library's own quantizers, searched in one process with
interleaved rounds through the device entry point.

    python tools/time_rerank_quantized.py                                  # 1M x 128 uniform flat hasher, m = 5000
    python tools/time_rerank_quantized.py --num-points 10000000 --leaves 1000 --P 10 --m 8192 --dist clustered
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/time_rerank_quantized.py --trace   # kernel times

One JSON line per handle: step time (median, min and max over the rounds), QPS, device_bytes, recall10@10 against the
exact f32 ground truth, and the gather floor's bytes nq * m * row bytes (divide by rerank_quant_kernel's time from the
kernel trace).  Then one line per handle for one query per call through the host entry point (the f32 handle takes the
wide few-query pipeline there, the quantized ones the staged pipeline).  --trace: a short run of every handle, for the
kernel trace (rerank_i8_kernel + rerank_short_kernel against rerank_quant_kernel + final_topk_kernel)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-points", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--S", type=int, default=32)
    ap.add_argument("--leaves", type=int, default=0, help="0: flat hasher")
    ap.add_argument("--P", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--m", type=int, default=5000)
    ap.add_argument("--dist", default="uniform", choices=["uniform", "clustered"])
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--single-steps", type=int, default=200)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    import torch
    from scann_rust_amd import hip, synth, trainer
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    Lh = hip.load()
    dev = torch.device("cuda", 0)
    n, dim, S, L, Q, k, m = a.n, a.dim, a.S, a.leaves, a.batch, a.k, a.m
    if a.dist == "uniform":
        rows = synth.uniform_f32(n, dim, 42)
        qs = synth.uniform_f32(Q, dim, 123)
    else:
        rows, _ = synth.clustered_f32(n, dim, 7, n_clusters=1000)
        qs, _ = synth.clustered_f32(Q, dim, 8, n_clusters=1000)
    rows = np.ascontiguousarray(rows, np.float32)
    t0 = time.time()
    if L == 0:
        cb = trainer.train_codebook(rows[:: max(1, n // 32768)], S, 16, iters=8, seed=42, sample=1 << 30)
        codes = hip.encode(cb, rows, stride=dim)
        desc = dict(n_rows=n, dim=dim, stride=dim, centers=None, leaf_offsets=None, leaf_ids=None, codebook=cb,
                    codes=codes, use_residuals=False, partitions_to_search=1, pre_reorder_multiplier=1.0)
    else:
        from sweep_txh import kmeans_torch
        X = torch.from_numpy(rows).to(dev)
        C, assign = kmeans_torch(X, L, 8, 42)
        order = torch.argsort(assign, stable=True)
        leaf_off = np.zeros(L + 1, np.uint32)
        leaf_off[1:] = np.cumsum(torch.bincount(assign, minlength=L).cpu().numpy())
        centers = C.cpu().numpy().astype(np.float32)
        leaf_of_row = assign[order].cpu().numpy().astype(np.uint32)
        csr = X[order]
        res = (csr - C[assign[order]]).cpu().numpy()
        cb = trainer.train_codebook(res[:: max(1, n // 32768)], S, 16, iters=8, seed=42, sample=1 << 30)
        codes = hip.encode(cb, np.ascontiguousarray(csr.cpu().numpy()), stride=dim, centers=centers,
                           leaf_of_row=leaf_of_row)
        desc = dict(n_rows=n, dim=dim, stride=dim, centers=centers, leaf_offsets=leaf_off,
                    leaf_ids=order.cpu().numpy().astype(np.uint32), codebook=cb, codes=codes, use_residuals=True,
                    partitions_to_search=a.P, pre_reorder_multiplier=3.0)
        del X, csr, res
    print("index build %.1fs" % (time.time() - t0), file=sys.stderr, flush=True)
    bf = hip.bf_create(rows, n, dim, dim, hip.SQUARED_L2)
    ne = min(256, Q)
    ti, _, _ = bf.search_batched(qs[:ne], k)
    bf.close()

    i8, inv8 = hip.symmetric_int8(rows)
    handles = [("f32", 4, hip.txh_create(data=rows, **desc)),
               ("bf16", 2, hip.txh_create_quantized(rows=hip.bf16_quantize(rows), fmt=hip.ROWS_BF16, **desc)),
               ("fp8_e4m3", 1, hip.txh_create_quantized(
                   rows=hip.fp8_quantize(rows, 400.0 / float(np.abs(rows).max())), fmt=hip.ROWS_FP8_E4M3, **desc)),
               ("int8", 1, hip.txh_create_quantized(rows=i8, fmt=hip.ROWS_INT8, inv_multiplier=inv8, **desc))]
    o = hip.default_opts()
    o.pre_reorder_k = m
    if L:
        o.partitions_to_search = a.P
    qd = torch.from_numpy(qs).to(dev)
    oi = torch.empty((Q, k), dtype=torch.int32, device=dev)
    od = torch.empty((Q, k), dtype=torch.float32, device=dev)
    oc = torch.empty((Q,), dtype=torch.int32, device=dev)
    sptr = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def run(ix):
        hip.check(Lh.scann_hip_search_batched_device(ix.h, p(qd), Q, dim, k, ctypes.byref(o), p(oi), p(od), p(oc), sptr))

    for _, _, ix in handles:
        hip.check(Lh.scann_hip_index_reserve(ix.h, Q, k, ctypes.byref(o)))
        for _ in range(3 if a.trace else 10):
            run(ix)
        torch.cuda.synchronize()
        hip.check(Lh.scann_hip_index_last_device_status(ix.h, sptr))
    if a.trace:
        for _, _, ix in handles:
            for _ in range(10):
                run(ix)
        torch.cuda.synchronize()
        return
    times = {name: [] for name, _, _ in handles}
    for _ in range(a.rounds):          # interleaved: every round times every handle
        for name, _, ix in handles:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                run(ix)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / a.steps)
    for name, bpe, ix in handles:
        gi, _, _ = ix.search_batched(qs[:ne], k, o)
        rec = sum(len(set(gi[i].tolist()) & set(ti[i].tolist())) for i in range(ne)) / (ne * float(k))
        t = sorted(times[name])
        print(json.dumps({"rows": name, "n": n, "dim": dim, "leaves": L, "P": a.P if L else 1, "nq": Q, "k": k, "m": m,
                          "step_ms": round(t[len(t) // 2] * 1e3, 4), "step_ms_min": round(t[0] * 1e3, 4),
                          "step_ms_max": round(t[-1] * 1e3, 4), "qps": round(Q / t[len(t) // 2], 1),
                          "device_bytes": ix.device_bytes(), "recall10at10": round(rec, 4),
                          "gather_floor_bytes": Q * m * dim * bpe}), flush=True)
    # one query per call, host entry point
    single = {name: [] for name, _, _ in handles}
    for name, _, ix in handles:
        for i in range(5):
            ix.search_batched(qs[i:i + 1], k, o)
    for _ in range(a.rounds):
        for name, _, ix in handles:
            t0 = time.perf_counter()
            for i in range(a.single_steps):
                ix.search_batched(qs[i % Q:i % Q + 1], k, o)
            single[name].append((time.perf_counter() - t0) / a.single_steps)
    for name, _, _ in handles:
        t = sorted(single[name])
        print(json.dumps({"rows": name, "nq": 1, "call_ms": round(t[len(t) // 2] * 1e3, 4),
                          "call_ms_min": round(t[0] * 1e3, 4), "call_ms_max": round(t[-1] * 1e3, 4)}), flush=True)


if __name__ == "__main__":
    main()

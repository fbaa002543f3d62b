#!/usr/bin/env python3
"""Times PCA training on the device (scann_hip_pca_train) and the one-call projected build
(scann_hip_txh_build_projected) against the host route they replace.

    python tools/time_pca_build.py                          # 1M x 768 -> 128, profiles/pca_build_1m768_time.jsonl
    python tools/time_pca_build.py --num-points 50000 --leaves 100 --reps 2 --out /tmp/t.jsonl     # a quick look

Data: the decaying spectrum of tools/time_projected.py (sd_i = (1 + i)^-1/2 in a rotated basis), generated on the GPU by
torch, copied to the host once and uploaded into the f32 brute-force handle both routes start from.

device route, per max_samples (100 000, the reference's default, and n):
    pca_train            stage times of scann_hip_pca_last_stage_ms: sample + mean, covariance, eigen-solve, components
    projection           scann_hip_project_device of all n rows on its own (the build's stage 0 includes this pass)
    txh_build_projected  the report's stage_ms: build = stages 0..5 less the projection, assembly = stage 6
  and the covariance stage as f64 FLOP/s, twice: the MFMA work issued (whole 64 x 64 panels of the upper panel triangle)
  and the useful half (ns * d * (d + 1) multiply-adds).  The stage is host-clocked around the kernel, its reduce pass and a
  synchronisation, so the figures are lower bounds of the kernel's own rate.
host route (max_samples 100 000 only: at n it would move and centre 1M x 768 f64 on the host):
    fetch the same sample rows, trainer.pca_projection (f64 eigh), hip.Projection, then the chained build: project on the
    device, download, second brute-force handle, scann_hip_txh_build without rows, read every array back through an index
    file in /dev/shm, scann_hip_txh_create_projected with the original rows.
The routes alternate in one process after a warm-up round; medians of --reps with the spread (min .. max).  One JSON line
per measurement, rewritten after each so that a run cut short keeps what it measured."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def stats(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-points", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--out-dim", type=int, default=128)
    ap.add_argument("--leaves", type=int, default=1000)
    ap.add_argument("--subspaces", type=int, default=32)
    ap.add_argument("--kmeans-iters", type=int, default=100)
    ap.add_argument("--pq-iters", type=int, default=25)
    ap.add_argument("--max-samples", default="100000,0", help="comma separated; 0 = every row")
    ap.add_argument("--host-max-samples", type=int, default=100000, help="the one setting the host route runs at")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pca_build_1m768_time.jsonl"))
    a = ap.parse_args()
    import torch
    from scann_rust_amd import hip, index_file, synth, trainer
    from time_projected import spectrum
    dev = "cuda:0"
    n, dim, od = a.n, a.dim, a.out_dim
    stride = hip.compute_stride(dim)
    g = torch.Generator(device=dev)
    g.manual_seed(42)
    basis, _ = torch.linalg.qr(torch.randn((dim, dim), generator=g, device=dev))
    Xd = spectrum(n, dim, basis, 43, dev)
    data = np.zeros((n, stride), np.float32)
    data[:, :dim] = Xd.cpu().numpy()
    d_rows = torch.from_numpy(data).to(dev) if stride != dim else Xd
    src = hip.bf_create(data, n, dim, stride, hip.SQUARED_L2)
    cfg = dict(num_partitions=a.leaves, num_subspaces=a.subspaces, num_codes=16, kmeans_iterations=a.kmeans_iters,
               training_iterations=a.pq_iters)
    d_out = torch.empty((n, od), dtype=torch.float32, device=dev)
    lines = []

    def emit(line):
        lines.append(line)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for done in lines:
                f.write(json.dumps(done) + "\n")
        print(json.dumps(line), flush=True)

    def device_route(ms):
        t0 = time.perf_counter()
        proj, info = hip.pca_train(src, od, max_samples=ms)
        t1 = time.perf_counter()
        stages = hip.pca_last_stage_ms()
        torch.cuda.synchronize()
        tp = time.perf_counter()
        proj.project_device(d_rows.data_ptr(), n, stride, d_out.data_ptr(), od)
        torch.cuda.synchronize()
        stages["projection"] = (time.perf_counter() - tp) * 1e3
        t2 = time.perf_counter()
        ix, rep = hip.txh_build_projected(src, proj, **cfg)
        t3 = time.perf_counter()
        b = rep["stage_ms"]
        stages["build"] = sum(v for k, v in b.items() if k != "finish") - stages["projection"]
        stages["assembly"] = b["finish"]
        ix.close()
        proj.close()
        return stages, t1 - t0, t3 - t2, info

    def host_route(ms, scratch):
        t0 = time.perf_counter()
        sel = (synth.splitmix64(42 ^ 0x9CA, 0, ms) % np.uint64(n)).astype(np.int64)
        X = d_rows[torch.from_numpy(sel).to(dev), :dim].cpu().numpy()
        t1 = time.perf_counter()
        M, mean = trainer.pca_projection(X, od)
        t2 = time.perf_counter()
        proj = hip.Projection(hip.PROJ_PCA, matrix=M, mean=mean)
        proj.project_device(d_rows.data_ptr(), n, stride, d_out.data_ptr(), od)
        torch.cuda.synchronize()
        projected = d_out.cpu().numpy()
        bfp = hip.bf_create(projected, n, od, od, hip.SQUARED_L2)
        built, _ = hip.txh_build(bfp, store_rows=0, **cfg)
        bfp.close()
        path = os.path.join(scratch, "chain.scannidx")
        hip.index_write_file(built, path)
        built.close()
        f = index_file.arrays(path)
        ix = hip.txh_create_projected(
            projection=proj, rows=data, n_rows=n, row_dim=dim, row_stride=stride, dim=od, centers=f["centers"],
            leaf_offsets=f["leaf_offsets"], leaf_ids=f["leaf_ids"], codebook=f["codebook"], codes=f["codes"],
            codes_packed4=bool(f["codes_packed4"]), use_residuals=bool(f["use_residuals"]),
            partitions_to_search=f["partitions_to_search"], pre_reorder_multiplier=f["pre_reorder_multiplier"])
        t3 = time.perf_counter()
        ix.close()
        proj.close()
        os.remove(path)
        return dict(fetch_sample=(t1 - t0) * 1e3, train_host=(t2 - t1) * 1e3, chained_build=(t3 - t2) * 1e3), t3 - t0

    scratch = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    settings = [int(v) for v in a.max_samples.split(",")]
    for ms in settings:
        ns = n if ms == 0 or ms >= n else ms
        with_host = ms == a.host_max_samples and 0 < ms < n
        dev_stages, dev_train, dev_build, host_stages, host_total, info = [], [], [], [], [], None
        for rep in range(a.reps + 1):          # round 0 is the warm-up
            st, tt, tb, info = device_route(ms)
            if with_host:
                hs, ht = host_route(ms, scratch)
            if rep == 0:
                continue
            dev_stages.append(st); dev_train.append(tt); dev_build.append(tb)
            if with_host:
                host_stages.append(hs); host_total.append(ht)
        npanels = (dim + 63) // 64
        cov_s = np.array([s["covariance"] for s in dev_stages]) * 1e-3
        issued = 2.0 * ns * (npanels * (npanels + 1) // 2) * 64 * 64
        useful = 2.0 * ns * dim * (dim + 1) / 2
        line = dict(route="device", n=n, dim=dim, out_dim=od, max_samples=ms, samples=ns, reps=a.reps, cfg=cfg,
                    sweeps=info["sweeps"], converged=info["converged"],
                    stage_ms={k: stats([s[k] for s in dev_stages]) for k in dev_stages[0]},
                    pca_train_seconds=stats(dev_train), build_projected_seconds=stats(dev_build),
                    total_seconds=stats([x + y for x, y in zip(dev_train, dev_build)]),
                    covariance_f64_tflops_issued=stats(list(issued / cov_s * 1e-12)),
                    covariance_f64_tflops_useful=stats(list(useful / cov_s * 1e-12)))
        emit(line)
        if with_host:
            emit(dict(route="host", n=n, dim=dim, out_dim=od, max_samples=ms, samples=ns, reps=a.reps, cfg=cfg,
                      stage_ms={k: stats([s[k] for s in host_stages]) for k in host_stages[0]},
                      total_seconds=stats(host_total)))
        else:
            emit(dict(route="host", n=n, dim=dim, out_dim=od, max_samples=ms, samples=ns, not_run=True,
                      reason="the host route is timed at --host-max-samples only"))
    os.rmdir(scratch)
    src.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times OPQ training on the device (scann_hip_opq_train) against the host route it replaces.

    python tools/time_opq.py                       # 1M x 128 (S 32, K 16) and 1M x 768 (S 96, K 256), 262 144 samples
    python tools/time_opq.py --shapes 50000x64x8x16 --max-samples 20000 --reps 1 --out-prefix /tmp/opq   # a quick look

Data: the decaying spectrum of tools/time_projected.py (sd_i = (1 + i)^-1/2 in a rotated basis), generated on the GPU by
torch and uploaded once into the f32 brute-force handle both routes start from.  Per shape, one JSON line each, written
to <out-prefix><n>x<d>_time.jsonl (default profiles/opq_train_*_time.jsonl) and rewritten after every measurement:
  device   the report's stage_ms (sample, project, codebook + encode, cross-covariance, polar; summed over the
           iterations), the wall time of the call, the distortion trace and the solves' sweeps; the cross-covariance
           stage as f64 FLOP/s (2 ns d^2 useful; the MFMA work issued covers whole 64 x 64 panels).  The stage is
           host-clocked around the kernel, its reduce pass and a synchronisation: a lower bound of the kernel's rate.
  host     fetch the same sample, trainer.opq_rotation (numpy f64, numpy.linalg.svd) with --host-iterations
           iterations, scaled to the device's count in "seconds_scaled".
  recall   recall10@10 (exact neighbours by the brute-force handle, --queries held-out rows) of a flat-hasher
           scann_hip_txh_build_projected with the trained rotation against the same build with the identity.
Nothing here is asserted: the figures are reported."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def stats(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1000000x128x32x16,1000000x768x96x256", help="comma separated n x d x S x K")
    ap.add_argument("--max-samples", type=int, default=262144)
    ap.add_argument("--opq-iterations", type=int, default=20)
    ap.add_argument("--host-iterations", type=int, default=2, help="0: skip the host route")
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out-prefix", default=os.path.join(ROOT, "profiles", "opq_train_"))
    a = ap.parse_args()
    import torch
    from scann_rust_amd import hip, synth, trainer
    from time_projected import spectrum
    dev = "cuda:0"
    for shape in a.shapes.split(","):
        n, dim, S, K = (int(v) for v in shape.split("x"))
        out = "%s%dx%d_time.jsonl" % (a.out_prefix, n, dim)
        lines = []

        def emit(line):
            lines.append(line)
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            with open(out, "w") as f:
                for done in lines:
                    f.write(json.dumps(done) + "\n")
            print(json.dumps(line), flush=True)

        g = torch.Generator(device=dev)
        g.manual_seed(42)
        basis, _ = torch.linalg.qr(torch.randn((dim, dim), generator=g, device=dev))
        rows = spectrum(n + a.queries, dim, basis, 43, dev).cpu().numpy()
        data, queries = np.ascontiguousarray(rows[:n]), np.ascontiguousarray(rows[n:])
        src = hip.bf_create(data, n, dim, dim, hip.SQUARED_L2)
        ns = n if a.max_samples == 0 or a.max_samples >= n else a.max_samples
        cfg = dict(num_subspaces=S, num_codes=K, opq_iterations=a.opq_iterations, max_samples=a.max_samples)
        walls, stages, rep, proj = [], [], None, None
        for r in range(a.reps + 1):              # round 0 is the warm-up
            if proj is not None:
                proj.close()
            t0 = time.perf_counter()
            proj, rep = hip.opq_train(src, **cfg)
            if r:
                walls.append(time.perf_counter() - t0)
                stages.append(rep["stage_ms"])
        cross_s = np.array([s["cross_covariance"] for s in stages]) * 1e-3 / max(1, len(rep["distortion"]))
        npanels = (dim + 63) // 64
        emit(dict(route="device", n=n, dim=dim, samples=ns, reps=a.reps, cfg=cfg, iterations_run=rep["iterations_run"],
                  stopped_singular=rep["stopped_singular"], distortion=rep["distortion"], sweeps=rep["sweeps"],
                  converged=rep["converged"], stage_ms={k: stats([s[k] for s in stages]) for k in stages[0]},
                  seconds=stats(walls),
                  cross_f64_tflops_useful=stats(list(2.0 * ns * dim * dim / cross_s * 1e-12)),
                  cross_f64_tflops_issued=stats(list(2.0 * ns * (npanels * 64) ** 2 / cross_s * 1e-12))))
        if a.host_iterations:
            t0 = time.perf_counter()
            sel = (synth.splitmix64(42 ^ 0x0B9, 0, ns) % np.uint64(n)).astype(np.int64) if ns < n else slice(None)
            X = data[sel]
            t1 = time.perf_counter()
            _, hd = trainer.opq_rotation(X, S, K, iterations=a.host_iterations)
            t2 = time.perf_counter()
            emit(dict(route="host", n=n, dim=dim, samples=ns, iterations=a.host_iterations, distortion=hd,
                      fetch_seconds=t1 - t0, train_seconds=t2 - t1,
                      seconds_scaled=(t2 - t1) * a.opq_iterations / a.host_iterations))
        # recall10@10 of a flat-hasher projected build: the trained rotation against the identity
        truth = src.search_batched(queries, 10)[0]
        recalls = {}
        ident = hip.Projection(hip.PROJ_MATRIX, matrix=np.eye(dim, dtype=np.float32))
        for name, p in (("opq", proj), ("identity", ident)):
            ix, _ = hip.txh_build_projected(src, p, num_partitions=0, num_subspaces=S, num_codes=K)
            o = hip.default_opts()
            o.pre_reorder_k = 10                 # no re-rank margin: the codes' own ranking
            idx = ix.search_batched(queries, 10, o)[0]
            recalls[name] = float(np.mean([len(set(idx[i]) & set(truth[i])) / 10.0 for i in range(len(queries))]))
            ix.close()
        ident.close()
        proj.close()
        emit(dict(route="recall", n=n, dim=dim, S=S, K=K, queries=len(queries), pre_reorder_k=10, recall10_at_10=recalls))
        src.close()


if __name__ == "__main__":
    main()

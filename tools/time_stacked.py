#!/usr/bin/env python3
"""Times a stacked-quantizer handle (hip.StackedIndex) at n x 128 rows, L = 2, S = (16, 16), K = 256; one JSON line each.

  (a) encode: scann_hip_stacked_set_rows (every level in one launch per batch, codes and norms stay on the device)
      against what the library offered before: one scann_hip_encode call per level with the residual formed on the host
      between them.  Host clocks around whole calls (both upload the rows), alternating, `repeats` times; for the fused
      call also the encode kernels' own device-event time.
  (b) scan: searches of 1, 64 and 1024 queries, k = 10: QPS from a host clock around whole calls; the table-build, scan
      and merge kernels' device-event times (median of the timed calls); beside the scan time the bytes of codes it must
      read (every query group streams all of them) over HBM peak, and the ds_read_b128 lane reads it must issue (rows x
      padded code positions x query quads) over the LDS rate of 256 CUs x 128 B/clk x 2.4 GHz.

    python tools/time_stacked.py [n] [seconds per timed window] [repeats of (a)]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scann_rust_amd import hip, trainer  # noqa: E402

HBM, LDS = 6.3e12, 256 * 128 * 2.4e9
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
window = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
dim, S, K, k = 128, (16, 16), (256, 256), 10
out = open(os.path.join(ROOT, "profiles", "stacked_1m128_time.jsonl"), "a") if n == 1_000_000 else None


def emit(**rec):
    line = json.dumps(dict(rec, n=n, dim=dim, subspaces=S, codes=K, device="MI355X, measured"))
    print(line, flush=True)
    if out:
        out.write(line + "\n")


rng = np.random.default_rng(0)
centres = rng.standard_normal((1000, dim)).astype(np.float32)
X = centres[rng.integers(0, 1000, n)] + 0.3 * rng.standard_normal((n, dim)).astype(np.float32)
books, _ = trainer.train_stacked(X[:: max(1, n // 32768)], S, K, iters=4)
sq = hip.StackedIndex(books, measure=hip.SQUARED_L2)


def unfused():
    R, codes = X, []
    for cb in books:
        codes.append(hip.encode(cb, R))
        R = R - trainer.decode(cb, codes[-1])
    return np.concatenate(codes, 1)


sq.set_rows(X[:4096])      # warm-up of both routes
hip.encode(books[0], X[:4096])
for rep in range(repeats):
    t0 = time.perf_counter()
    sq.set_rows(X)
    fused = time.perf_counter() - t0
    kernel_ms = sq.last_kernel_ms()[0]
    t0 = time.perf_counter()
    codes = unfused()
    per_level = time.perf_counter() - t0
    emit(what="encode", repeat=rep, fused_set_rows_s=round(fused, 4), fused_encode_kernels_ms=round(kernel_ms, 3),
         per_level_scann_hip_encode_s=round(per_level, 4), per_level_includes="host residual between levels and the codes' copy back",
         same_codes=bool(np.array_equal(sq.encode(X[:65536]), codes[:65536])))

T = sum(S)
tpad = (T + 3) // 4 * 4
for nq in (1, 64, 1024):
    Q = X[rng.integers(0, n, nq)] + 0.1 * rng.standard_normal((nq, dim)).astype(np.float32)
    sq.search_batched(Q, k)   # warm-up of this shape
    t0 = time.perf_counter()
    sq.search_batched(Q, k)
    steps = max(5, int(window / (time.perf_counter() - t0)))
    ms = []
    t0 = time.perf_counter()
    for _ in range(steps):
        sq.search_batched(Q, k)
        ms.append(sq.last_kernel_ms()[1:])
    wall = time.perf_counter() - t0
    lut, scan, merge = (float(x) for x in np.median(np.array(ms), 0))
    info = sq.info()
    code_bytes = n * tpad * info["groups"]
    lane_reads = n * tpad * ((nq + 3) // 4)
    emit(what="search", batch=nq, k=k, steps=steps, qps=round(nq * steps / wall, 1), lut_ms=round(lut, 4), scan_ms=round(scan, 4),
         merge_ms=round(merge, 4), slabs=info["slabs"], chunks=info["chunks"], query_groups=info["groups"],
         code_bytes_read=code_bytes, code_bytes_share_of_hbm_peak=round(code_bytes / (scan * 1e-3) / HBM, 4),
         ds_read_b128_lane_reads=lane_reads, lds_bytes_share_of_peak=round(lane_reads * 16 / (scan * 1e-3) / LDS, 4))

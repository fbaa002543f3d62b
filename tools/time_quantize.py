#!/usr/bin/env python3
"""Times scann_hip_index_quantize_rows against the route a user takes without it, on 1M x 128 uniform
rows resident in

  bf   the brute-force DotProduct index of the README table
  ah   the flat hasher of the README table (S = 32, K = 16, pre_reorder_k = 5000)

Per index, row format (bf16 / fp8 / int8) and, for int8, mode (signed / stddev), alternating in one process (3 warm-up
rounds, medians of `repeats` >= 20 rounds, host clock around a synchronise):
  device   Index.quantize_rows: stats, calibrate, quantize pass, norms and the rest of the create, nothing leaves the
           card.  Split: `stats` = quantization_stats alone, `quantize` = scalar_quantize_device alone (int8; the
           bf16 / fp8 pass has no entry point of its own), `rest` = device - stats - quantize.
  host     the rows the caller already holds on the host, quantized there (hip.symmetric_int8, bf16_quantize,
           fp8_quantize: the last two upload and download through their own entry points), then *_create_quantized.
           The reference-mode int8 rows have no host route at the parent commit: `host` is then the signed route.
Per kernel: bytes moved (from shapes) over the time as a share of the measured HBM copy rate.  One JSON line per
point; --write puts them into profiles/scalar_quantizer_1m128_time.jsonl.

    python tools/time_quantize.py [bf|ah|all] [n] [repeats] [--write]
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from scann_rust_amd import hip, synth, trainer  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
which = args[0] if len(args) > 0 else "all"
n = int(args[1]) if len(args) > 1 else 1_000_000
repeats = int(args[2]) if len(args) > 2 else 20
dim, k, S, K, m = 128, 10, 32, 16, 5000
HBM_COPY_TBS = 6.29   # measured float4 copy rate of the MI355X (read + write bytes per second)
if not torch.cuda.is_available():
    sys.exit("time_quantize.py needs the GPU: a timing taken elsewhere says nothing")

rows = synth.uniform_f32(n, dim, 42) - np.float32(0.5)
lines = []


def med(v):
    return round(statistics.median(v), 4)


def build(kind):
    if kind == "bf":
        return hip.bf_create(rows, n, dim, dim, hip.DOT_PRODUCT), None
    sample = np.ascontiguousarray(rows[:: max(1, n // 65536)][:65536])
    codebook = trainer.train_codebook(sample, S, K, iters=10, seed=42, sample=1 << 30)
    desc = dict(n_rows=n, dim=dim, stride=dim, centers=None, leaf_offsets=None, leaf_ids=None, codebook=codebook,
                codes=hip.encode(codebook, rows, stride=dim), use_residuals=False, partitions_to_search=1,
                pre_reorder_multiplier=float(m) / k)
    return hip.txh_create(data=rows, **desc), desc


def host_route(kind, desc, fmt):
    if fmt == hip.ROWS_BF16:
        q, inv = hip.bf16_quantize(rows), 1.0
    elif fmt == hip.ROWS_FP8_E4M3:
        q, inv = hip.fp8_quantize(rows), 1.0
    else:
        q, inv = hip.symmetric_int8(rows)
    if kind == "bf":
        return hip.bf_create_quantized(q, n, dim, dim, fmt, hip.DOT_PRODUCT, inv)
    return hip.txh_create_quantized(rows=q, fmt=fmt, inv_multiplier=inv, **desc)


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    if isinstance(out, tuple):
        out = out[0]
    if hasattr(out, "close"):
        out.close()
    return ms


def run(kind):
    src, desc = build(kind)
    d_rows = torch.from_numpy(rows).to("cuda:0")
    d_out = torch.empty(n * dim, dtype=torch.int8, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    for name, fmt, mode in (("bf16", hip.ROWS_BF16, hip.SQ_SIGNED), ("fp8", hip.ROWS_FP8_E4M3, hip.SQ_SIGNED),
                            ("int8-signed", hip.ROWS_INT8, hip.SQ_SIGNED), ("int8-stddev", hip.ROWS_INT8, hip.SQ_STDDEV)):
        t = {"device": [], "host": [], "stats": [], "quantize": []}
        params = None
        for r in range(repeats + 3):
            got = {}
            got["device"] = clocked(lambda: src.quantize_rows(fmt, mode=mode))
            got["host"] = clocked(lambda: host_route(kind, desc, fmt))
            if fmt == hip.ROWS_INT8:
                got["stats"] = clocked(lambda: hip.quantization_stats(src))
                if params is None:
                    sq = hip.ScalarQuantizer(mode=mode)
                    sq.calibrate(hip.quantization_stats(src))
                    params = sq.params
                got["quantize"] = clocked(lambda: hip.scalar_quantize_device(d_rows.data_ptr(), n, dim, dim, d_out.data_ptr(),
                                                                            dim, params, mode=mode, stream=stream))
            if r >= 3:
                for key, v in got.items():
                    t[key].append(v)
        line = {"index": kind, "n": n, "dim": dim, "format": name, "repeats": repeats,
                "device_ms": med(t["device"]), "host_route_ms": med(t["host"]),
                "speedup": round(med(t["host"]) / med(t["device"]), 2)}
        if t["stats"]:
            st, qu = med(t["stats"]), med(t["quantize"])
            line.update(stats_ms=st, quantize_ms=qu, rest_ms=round(line["device_ms"] - st - qu, 4),
                        stats_share_of_copy_rate=round(n * dim * 4 / (st * 1e-3) / (HBM_COPY_TBS * 1e12), 3),
                        quantize_share_of_copy_rate=round(n * dim * 5 / (qu * 1e-3) / (HBM_COPY_TBS * 1e12), 3),
                        note="stats_ms and quantize_ms are host-clocked calls: they include a launch, a synchronise and, "
                             "for stats, two launches and a 32-byte read-back")
        print(json.dumps(line), flush=True)
        lines.append(line)
    src.close()


for kind in (("bf", "ah") if which == "all" else (which,)):
    run(kind)
if "--write" in sys.argv:
    path = os.path.join(ROOT, "profiles", "scalar_quantizer_1m128_time.jsonl")
    with open(path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
    print("wrote", path)

#!/usr/bin/env python3
"""Times brute force over 1M x 128 U[0,1) rows stored as f32, bf16, FP8 E4M3 and int8 (k = 10, SquaredL2 and
DotProduct, batches 1, 32, 1024) through the device entry point.  Prints one JSON line per case: QPS, the main
pass kernel's HIP-event time and name, the bytes-per-row floor of one read of the rows at 6.3 TB/s and the
fraction of it the kernel reached, and the fraction of queries the first (unforced) pass verified (status Ok).

    python tools/time_bf_quantized.py [n] [steps]
"""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from scann_rust_amd import hip, synth  # noqa: E402
from tests import quantized_checker as qc  # noqa: E402

HBM = 6.3e12
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dim, k = 128, 10
x = synth.uniform_f32(n, dim, 42)
L = hip.load()
dev = torch.device("cuda", 0)
sptr = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
p = lambda t: ctypes.c_void_p(t.data_ptr())

formats = [("f32", 0, 4), ("bf16", hip.ROWS_BF16, 2), ("fp8_e4m3", hip.ROWS_FP8_E4M3, 1), ("int8", hip.ROWS_INT8, 1)]
for fname, fmt, bpe in formats:
    if fmt == hip.ROWS_BF16:
        rows, inv = qc.bf16_from_f32(x), 1.0
    elif fmt == hip.ROWS_FP8_E4M3:
        from oracle import pyoracle as orc
        rows, inv = orc.fp8_quantize(x, 64.0), 1.0
    elif fmt == hip.ROWS_INT8:
        rows, inv = hip.symmetric_int8(x)
    for mname, meas in (("sql2", hip.SQUARED_L2), ("dot", hip.DOT_PRODUCT)):
        ix = hip.bf_create(x, n, dim, dim, meas) if fmt == 0 else hip.bf_create_quantized(rows, n, dim, dim, fmt,
                                                                                           meas, inv)
        for nq in (1, 32, 1024):
            q = synth.uniform_f32(nq, dim, 123)
            qd = torch.from_numpy(q).to(dev)
            oi = torch.empty((nq, k), dtype=torch.int32, device=dev)
            od = torch.empty((nq, k), dtype=torch.float32, device=dev)
            oc = torch.empty((nq,), dtype=torch.int32, device=dev)
            hip.check(L.scann_hip_index_reserve(ix.h, nq, k, None))

            def run():
                hip.check(L.scann_hip_search_batched_device(ix.h, p(qd), nq, dim, k, None, p(oi), p(od), p(oc), sptr))
            run()
            verified = L.scann_hip_index_last_device_status(ix.h, sptr) == hip.OK
            ix.enable_timing(True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                run()
            torch.cuda.synchronize()
            el = (time.perf_counter() - t0) / steps
            kms, kname = ix.last_kernel_ms()
            ix.enable_timing(False)
            floor_ms = n * dim * bpe / HBM * 1e3
            print(json.dumps({"rows": fname, "measure": mname, "n": n, "dim": dim, "nq": nq, "k": k,
                              "qps": round(nq / el, 1), "step_ms": round(el * 1e3, 4), "kernel": kname,
                              "kernel_ms": round(kms, 4), "bytes_per_row": dim * bpe,
                              "floor_ms": round(floor_ms, 4),
                              "floor_fraction": round(floor_ms / kms, 3) if kms > 0 else None,
                              "verified": bool(verified)}), flush=True)
        ix.close()

#!/usr/bin/env python3
"""Times brute force over n bit rows (ROWS_BIN1, Hamming, k = 10) of 256, 1024 and 4096 bits at batches 1, 32, 64, 128, 256 and 1024
through the device entry point, and at 256 and 1024 bits the one-query search of an f32 SquaredL2 handle over the same
rows unpacked to 0/1 floats (the form such data had to take before).  Prints one JSON line per case: QPS from a host
clock around enough enqueued searches to fill the window, ending in a synchronise, the main pass kernel's HIP-event time (median of
20 single searches) and name, and that time against one read of the rows at 6.3 TB/s.

    python tools/time_binary_rows.py [n] [seconds per timed window] [variant tag copied into every line]

A variant library (build.build_variant("popc", ["-DSCANN_BF_BIN_MFMA_MIN_QUERIES=0x7fffffff"], only=("bf_bin.hip",)):
the popcount kernel at every batch size) is selected with SCANN_HIP_LIB; the two builds are timed in alternating
processes of one job.
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

from scann_rust_amd import hip  # noqa: E402

HBM = 6.3e12
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
window = float(sys.argv[2]) if len(sys.argv) > 2 else 0.5
variant = sys.argv[3] if len(sys.argv) > 3 else None
k = 10
L = hip.load()
dev = torch.device("cuda", 0)
sptr = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
p = lambda t: ctypes.c_void_p(t.data_ptr())


def time_handle(ix, name, dim, row_bytes, batches):
    for nq in batches:
        q = (np.random.default_rng(nq).random((nq, dim)) < 0.5).astype(np.float32)
        qd = torch.from_numpy(q).to(dev)
        oi = torch.empty((nq, k), dtype=torch.int32, device=dev)
        od = torch.empty((nq, k), dtype=torch.float32, device=dev)
        oc = torch.empty((nq,), dtype=torch.int32, device=dev)
        hip.check(L.scann_hip_index_reserve(ix.h, nq, k, None))

        def run():
            hip.check(L.scann_hip_search_batched_device(ix.h, p(qd), nq, dim, k, None, p(oi), p(od), p(oc), sptr))
        run()   # warm-up of this shape
        assert L.scann_hip_index_last_device_status(ix.h, sptr) == hip.OK
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        steps = max(20, int(window / ((time.perf_counter() - t0) / 5)))   # a timed window of about `window` seconds
        t0 = time.perf_counter()
        for _ in range(steps):
            run()
        torch.cuda.synchronize()
        el = (time.perf_counter() - t0) / steps
        ix.enable_timing(True)
        kms = []
        for _ in range(20):
            run()
            torch.cuda.synchronize()
            ms, kname = ix.last_kernel_ms()
            kms.append(ms)
        ix.enable_timing(False)
        kmed = float(np.median(kms))
        floor_ms = n * row_bytes / HBM * 1e3
        print(json.dumps({**({"variant": variant} if variant else {}), "rows": name, "steps": steps, "n": n, "dim": dim, "nq": nq, "k": k, "qps": round(nq / el, 1),
                          "step_ms": round(el * 1e3, 4), "kernel": kname, "kernel_ms": round(kmed, 4),
                          "kernel_ms_min": round(float(np.min(kms)), 4), "bytes_per_row": row_bytes,
                          "floor_ms": round(floor_ms, 4), "floor_fraction": round(floor_ms / kmed, 3) if kmed > 0 else None}),
              flush=True)


for dim in (256, 1024, 4096):
    packed = np.random.default_rng(dim).integers(0, 256, (n, dim // 8), dtype=np.uint8)
    ix = hip.bf_create_quantized(packed, n, dim, dim, hip.ROWS_BIN1, hip.HAMMING)
    time_handle(ix, "bin1", dim, dim // 8, (1, 32, 64, 128, 256, 1024))
    ix.close()
    if dim <= 1024:
        x = hip.unpack_bits(packed, dim).astype(np.float32)
        ix = hip.bf_create(x, n, dim, dim, hip.SQUARED_L2)
        del x
        time_handle(ix, "f32", dim, dim * 4, (1,))
        ix.close()

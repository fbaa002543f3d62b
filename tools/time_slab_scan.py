#!/usr/bin/env python3
"""Times the slab-walking LUT16 scan (adc_slab_scan_kernel) beside adc_scan_kernel<Codec<64, 4>> and records
what the extra subspaces buy in recall.

    python tools/time_slab_scan.py                                  # 1M x 768 flat hashers, batch 1024
    python tools/time_slab_scan.py --num-points 50000 --rounds 3    # a quick look

Flat hashers over synth.clustered_f32 rows, built on the device (hip.txh_build, num_partitions = 0) at S = 64 (forced
onto the f32 gather scan: SCANN_HIP_MFMA=0 SCANN_HIP_RESIDENT=0, the parent's code path) and S = 96 / 192 / 384 (the
slab scan).  One process, a warm-up, then interleaved rounds: every round times every handle.
(a) scan: the kernel time scann_hip_index_last_kernel_ms reports at m = 5000, and from it picoseconds per
    point x query x subspace, median with min / max, and the ratio to S = 64.
(b) recall10@10 against the exact brute force of the same rows and the QPS of whole search calls, at equal
    pre_reorder_k = 100 and 1000.
One JSON line per measurement, appended to profiles/slab_scan_768_time.jsonl.

    python tools/time_slab_scan.py --num-codes 256 --subspaces 16 32 64 96 128 192x16 \
        --json profiles/slab8_scan_768_time.jsonl

--num-codes 256: byte codes, S = 16 on adc_scan_kernel<Codec<16, 8>> as the yardstick and the others on
adc_slab8_scan_kernel.  An entry SxK builds that handle with K codes: 192x16 beside 96 is the
equal-code-bytes pair of part (b)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-points", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--subspaces", nargs="+", default=["64", "96", "192", "384"], help="S, or SxK for a handle of K codes")
    ap.add_argument("--num-codes", type=int, default=16)
    ap.add_argument("--training-iterations", type=int, default=6)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--scan-m", type=int, default=5000)
    ap.add_argument("--recall-m", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "slab_scan_768_time.jsonl"))
    a = ap.parse_args()
    os.environ["SCANN_HIP_MFMA"] = "0"        # S = 64 on adc_scan_kernel; a knob never reroutes S > 64
    os.environ["SCANN_HIP_RESIDENT"] = "0"
    from scann_rust_amd import hip, synth
    n, dim, Q, k = a.n, a.dim, a.batch, a.k
    rows, _ = synth.clustered_f32(n, dim, 42, n_clusters=1000)
    q = synth.clustered_f32(Q, dim, 43, n_clusters=1000)[0]
    bf = hip.bf_create(rows, n, dim, dim, hip.SQUARED_L2)
    ne = min(256, Q)
    truth = bf.search_batched(q[:ne], k)[0]
    handles = {}
    codes = {}   # handle key (S, or the string SxK) -> (S, K)
    for spec in a.subspaces:
        S, _, K = spec.partition("x")
        codes[spec if K else int(S)] = (int(S), int(K) if K else a.num_codes)
    for key, (S, K) in codes.items():
        t0 = time.time()
        handles[key], _ = hip.txh_build(bf, num_partitions=0, num_subspaces=S, num_codes=K,
                                        training_iterations=a.training_iterations)
        handles[key].enable_timing(True)
        print("built S=%d K=%d in %.1fs" % (S, K, time.time() - t0), file=sys.stderr, flush=True)
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    def opts(m):
        o = hip.default_opts()
        o.pre_reorder_k = m
        return o

    # ---- (a) the scan kernels ---------------------------------------------------------------------------------------
    o = opts(a.scan_m)
    for ix in handles.values():
        for _ in range(3):
            ix.search_batched(q, k, o)
    scan = {S: [] for S in handles}
    names = {}
    for _ in range(a.rounds):
        for S, ix in handles.items():
            ix.search_batched(q, k, o)
            ms, names[S] = ix.last_kernel_ms()
            scan[S].append(ms)
    ps = lambda key, ms: ms * 1e9 / (float(n) * Q * codes[key][0])
    yard = 64 if a.num_codes <= 16 else 16   # the largest S of the gather scan for these codes
    base = ps(yard, med(scan[yard])[0]) if yard in scan else None
    for key in handles:
        m_, lo, hi = med(scan[key])
        emit({"what": "scan", "kernel": names[key], "n": n, "dim": dim, "S": codes[key][0], "num_codes": codes[key][1],
              "nq": Q, "m": a.scan_m, "ms": round(m_, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
              "ps_per_point_query_subspace": round(ps(key, m_), 4),
              "ratio_to_S%d" % yard: round(ps(key, m_) / base, 3) if base else None, "rounds": a.rounds})
    # ---- (b) recall and QPS at equal pre_reorder_k ------------------------------------------------------------------
    for m in a.recall_m:
        o = opts(m)
        step = {S: [] for S in handles}
        for ix in handles.values():
            ix.search_batched(q, k, o)
        for _ in range(a.rounds):
            for S, ix in handles.items():
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    ix.search_batched(q, k, o)
                step[S].append((time.perf_counter() - t0) / a.steps * 1e3)
        for S, ix in handles.items():
            gi = ix.search_batched(q[:ne], k, o)[0]
            rec = sum(len(set(gi[i].tolist()) & set(truth[i].tolist())) for i in range(ne)) / (ne * float(k))
            m_, lo, hi = med(step[S])
            emit({"what": "search", "n": n, "dim": dim, "S": codes[S][0], "num_codes": codes[S][1], "nq": Q, "k": k, "m": m,
                  "step_ms": round(m_, 4),
                  "step_ms_min": round(lo, 4), "step_ms_max": round(hi, 4), "qps": round(Q / (m_ * 1e-3), 1),
                  "recall10at10": round(rec, 4)})
    with open(a.json, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

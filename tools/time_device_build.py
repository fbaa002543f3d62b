#!/usr/bin/env python3
"""Times scann_hip_txh_build (the one-call device build) against the chained route of tools/time_build.py (upload,
k-means++, Lloyd, host residuals, upload, per-subspace codebook, encode, host CSR, scann_hip_txh_create), and the
batched codebook training against the per-subspace loop.  The routes run ALTERNATELY in one process after a warm-up
round; medians of --reps with the spread (min .. max).  libscann_hip.so only.

    python tools/time_device_build.py                      # the three 1M x 128 shapes, profiles/device_build_1m128_time.jsonl
    python tools/time_device_build.py --num-points 100000 --reps 3 --out /tmp/t.jsonl
    rocprofv3 --kernel-trace --stats -d trace -- python tools/time_device_build.py --one-call-only --shapes tree-S32-K16
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("tree-S32-K16", dict(L=1000, S=32, K=16)), ("tree-S8-K256", dict(L=1000, S=8, K=256)),
          ("flat-S32-K16", dict(L=0, S=32, K=16)))


def chained(hip, data, rows, n, dim, stride, L, S, K, kmeans_iters, pq_iters):
    """the parent route: every step of tools/time_build.py, then the CSR on the host and scann_hip_txh_create"""
    dsub = dim // S
    bf = hip.bf_create(data, n, dim, stride, hip.SQUARED_L2)
    if L:
        init = hip.kmeans_init_pp(bf, L, seed=42)
        centers, assign, _, _, _, _ = hip.kmeans_lloyd(bf, init, max_iterations=kmeans_iters)
        resid = np.zeros((n, stride), np.float32)
        resid[:, :dim] = rows - centers[assign]
        bf.close()
        bf = hip.bf_create(resid, n, dim, stride, hip.SQUARED_L2)
    else:
        resid = data
    cb = np.zeros((S, K, dsub), np.float32)
    for s in range(S):
        c0 = hip.kmeans_init_pp(bf, K, seed=42 + s, col_offset=s * dsub, sub_dim=dsub)
        cb[s] = hip.kmeans_lloyd(bf, c0, max_iterations=pq_iters, col_offset=s * dsub)[0]
    bf.close()
    codes = hip.encode(cb, resid, stride=stride)
    if L:
        order = np.argsort(assign, kind="stable").astype(np.uint32)
        leaf_off = np.zeros(L + 1, np.uint32)
        leaf_off[1:] = np.cumsum(np.bincount(assign, minlength=L))
        ix = hip.txh_create(data=data, n_rows=n, dim=dim, stride=stride, centers=centers, leaf_offsets=leaf_off,
                            leaf_ids=order, codebook=cb, codes=codes[order])
    else:
        ix = hip.txh_create(data=data, n_rows=n, dim=dim, stride=stride, centers=None, leaf_offsets=None, leaf_ids=None,
                            codebook=cb, codes=codes)
    ix.close()


def one_call(hip, data, n, dim, stride, L, S, K, kmeans_iters, pq_iters, batched):
    """upload + scann_hip_txh_build: the same span as the chained route; returns (stage_ms, build-call seconds)"""
    bf = hip.bf_create(data, n, dim, stride, hip.SQUARED_L2)
    t = time.perf_counter()
    ix, rep = hip.txh_build(bf, num_partitions=L, num_subspaces=S, num_codes=K, kmeans_iterations=kmeans_iters,
                            training_iterations=pq_iters, batched_codebook=batched)
    call = time.perf_counter() - t
    ix.close()
    bf.close()
    return rep["stage_ms"], call


def stats(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-points", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kmeans-iters", type=int, default=100)
    ap.add_argument("--pq-iters", type=int, default=25)
    ap.add_argument("--shapes", default=",".join(name for name, _ in SHAPES))
    ap.add_argument("--one-call-only", action="store_true",
                    help="one batched build per shape and nothing else: the run a kernel trace is taken from")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_build_1m128_time.jsonl"))
    a = ap.parse_args()
    from scann_rust_amd import hip, synth
    n, dim = a.n, a.dim
    stride = hip.compute_stride(dim)
    rows, _ = synth.clustered_f32(n, dim, 7, n_clusters=1000)
    data = np.zeros((n, stride), np.float32)
    data[:, :dim] = rows
    lines = []
    for name, sh in SHAPES:
        if name not in a.shapes.split(","):
            continue
        L, S, K = sh["L"], sh["S"], sh["K"]
        if a.one_call_only:
            ms, call = one_call(hip, data, n, dim, stride, L, S, K, a.kmeans_iters, a.pq_iters, 1)
            print("%s: build call %.3f s  %s" % (name, call, "  ".join("%s %.1f" % kv for kv in ms.items())), flush=True)
            continue
        t = dict(chained=[], one_call=[], one_call_per_subspace=[], build_call=[], build_call_per_subspace=[])
        stages = {0: [], 1: []}
        for rep in range(a.reps + 1):          # round 0 is the warm-up
            t0 = time.perf_counter()
            chained(hip, data, rows, n, dim, stride, L, S, K, a.kmeans_iters, a.pq_iters)
            t1 = time.perf_counter()
            ms1, call1 = one_call(hip, data, n, dim, stride, L, S, K, a.kmeans_iters, a.pq_iters, 1)
            t2 = time.perf_counter()
            ms0, call0 = one_call(hip, data, n, dim, stride, L, S, K, a.kmeans_iters, a.pq_iters, 0)
            t3 = time.perf_counter()
            if rep == 0:
                continue
            t["chained"].append(t1 - t0); t["one_call"].append(t2 - t1); t["one_call_per_subspace"].append(t3 - t2)
            t["build_call"].append(call1); t["build_call_per_subspace"].append(call0)
            stages[1].append(ms1); stages[0].append(ms0)
        line = dict(shape=name, n=n, dim=dim, L=L, S=S, K=K, kmeans_iterations=a.kmeans_iters,
                    training_iterations=a.pq_iters, reps=a.reps, seconds={k: stats(v) for k, v in t.items()},
                    stage_ms_batched={k: stats([m[k] for m in stages[1]]) for k in hip.BUILD_STAGES},
                    stage_ms_per_subspace={k: stats([m[k] for m in stages[0]]) for k in hip.BUILD_STAGES})
        lines.append(line)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:      # rewritten after every shape: a run cut short keeps what it measured
            for done in lines:
                f.write(json.dumps(done) + "\n")
        s = line["seconds"]
        print("%s: chained %.3f s [%.3f .. %.3f]  one call %.3f s [%.3f .. %.3f]  one call, per-subspace codebook %.3f s "
              "[%.3f .. %.3f]" % (name, s["chained"]["median"], s["chained"]["min"], s["chained"]["max"],
                                  s["one_call"]["median"], s["one_call"]["min"], s["one_call"]["max"],
                                  s["one_call_per_subspace"]["median"], s["one_call_per_subspace"]["min"],
                                  s["one_call_per_subspace"]["max"]), flush=True)
        for label, key in (("batched", "stage_ms_batched"), ("per-subspace", "stage_ms_per_subspace")):
            print("  stage_ms %-12s %s" % (label, "  ".join("%s %.1f" % (k, line[key][k]["median"])
                                                           for k in hip.BUILD_STAGES)), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times scann_hip_txh_build_hierarchical (a k-means tree trained level by level, flattened to its leaves) against
scann_hip_txh_build's flat partitioner with about as many leaves, on the clustered rows bench.py's tree workload uses
(bench.clustered_points, seed 11; queries seed 12; ground truth = the library's exact brute force).  The routes run
ALTERNATELY in one process after a warm-up round; medians of --reps with the spread (min .. max).  One JSON line per
route.  libscann_hip.so only.

    python tools/time_hier_build.py                  # 1M x 128: flat L = 1024 against 32 children x depth 2
                                                     #   -> profiles/hier_build_1m128_time.jsonl
    python tools/time_hier_build.py --mode quality   # recall10@10 and QPS of the two 1M indexes at P = 10 and at the
                                                     #   smallest P of a grid with recall >= 0.95
                                                     #   -> profiles/hier_build_1m128_quality.jsonl
    python tools/time_hier_build.py --mode big       # 10M x 128: 100 x 100 against flat L = 10000 CAPPED at 3 Lloyd
                                                     #   iterations (its per-round and per-iteration cost, measured)
                                                     #   -> profiles/hier_build_10m128_time.jsonl
    rocprofv3 --kernel-trace --stats -d trace -- python tools/time_hier_build.py --mode trace   # one hierarchical build
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P_GRID = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 32, 48, 64, 96, 128)


def stats(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def rows_and_queries(n, dim, nq):
    """bench.py's tree workload: rows of seed 11, queries of seed 12 (generated on the device, as bench.py does)"""
    import torch

    import bench
    device = torch.device("cuda:0")
    rows = bench.clustered_points(torch, device, 11, n, dim).cpu().numpy().astype(np.float32)
    queries = bench.clustered_points(torch, device, 12, nq, dim).cpu().numpy().astype(np.float32)
    return rows, queries


def build_flat(hip, bf, L, S, K, iters, pq_iters):
    t = time.perf_counter()
    ix, rep = hip.txh_build(bf, num_partitions=L, num_subspaces=S, num_codes=K, kmeans_iterations=iters,
                            training_iterations=pq_iters)
    return ix, rep, None, time.perf_counter() - t


def build_hier(hip, bf, children, depth, S, K, iters, pq_iters):
    t = time.perf_counter()
    ix, rep, trep = hip.txh_build_hierarchical(bf, tree=dict(num_children=children, max_depth=depth,
                                                             kmeans_iterations=iters),
                                               num_subspaces=S, num_codes=K, training_iterations=pq_iters)
    return ix, rep, trep, time.perf_counter() - t


def line_of(route, desc, calls, reps_list, treps):
    from scann_rust_amd import hip
    out = dict(route=route, **desc, reps=len(calls), build_call_s=stats(calls),
               stage_ms={k: stats([r["stage_ms"][k] for r in reps_list]) for k in hip.BUILD_STAGES},
               partitioner_ms=stats([r["stage_ms"]["partition_seeding"] + r["stage_ms"]["partition_lloyd"]
                                     for r in reps_list]),
               partition_iterations=reps_list[-1]["partition_iterations"])
    if treps:
        last = treps[-1]
        out.update(num_leaves=last["num_leaves"], depth_reached=last["depth_reached"], level_nodes=last["level_nodes"],
                   level_iterations=last["level_iterations"], level_converged=last["level_converged"],
                   level_leaves=last["level_leaves"],
                   level_seeding_ms=[stats([t["stage_ms"][d][0] for t in treps]) for d in range(5)],
                   level_lloyd_ms=[stats([t["stage_ms"][d][1] for t in treps]) for d in range(5)])
    return out


def write(path, lines):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


def show(ln):
    b, p = ln["build_call_s"], ln["partitioner_ms"]
    print("%s: build call %.3f s [%.3f .. %.3f]  partitioner stages %.1f ms [%.1f .. %.1f]" % (
        ln["route"], b["median"], b["min"], b["max"], p["median"], p["min"], p["max"]), flush=True)
    print("  stage_ms  " + "  ".join("%s %.1f" % (k, v["median"]) for k, v in ln["stage_ms"].items()), flush=True)
    if "level_nodes" in ln:
        for d in range(5):
            if ln["level_nodes"][d] or ln["level_leaves"][d]:
                print("  level %d: %d nodes trained, %d iterations, %d converged, %d leaves; seeding %.1f ms, Lloyd %.1f ms" % (
                    d, ln["level_nodes"][d], ln["level_iterations"][d], ln["level_converged"][d], ln["level_leaves"][d],
                    ln["level_seeding_ms"][d]["median"], ln["level_lloyd_ms"][d]["median"]), flush=True)


def timing(a, hip, bf, n, dim, flat_L, children, depth, flat_iters, label, out):
    acc = dict(flat=([], [], []), hier=([], [], []))
    for rep in range(a.reps + 1):          # round 0 is the warm-up
        for route in ("flat", "hier"):
            if route == "flat":
                ix, r, t, call = build_flat(hip, bf, flat_L, a.S, a.K, flat_iters, a.pq_iters)
            else:
                ix, r, t, call = build_hier(hip, bf, children, depth, a.S, a.K, a.kmeans_iters, a.pq_iters)
            ix.close()
            if rep:
                acc[route][0].append(call); acc[route][1].append(r); acc[route][2].append(t)
    base = dict(n=n, dim=dim, S=a.S, K=a.K, training_iterations=a.pq_iters)
    lines = [line_of("flat" + label, dict(base, L=flat_L, kmeans_iterations=flat_iters), acc["flat"][0], acc["flat"][1], None),
             line_of("hierarchical", dict(base, num_children=children, max_depth=depth, kmeans_iterations=a.kmeans_iters),
                     acc["hier"][0], acc["hier"][1], acc["hier"][2])]
    write(out, lines)
    for ln in lines:
        show(ln)


def quality(a, hip, bf, rows, queries, n, dim, out):
    k, m = 10, a.pre_reorder_k
    truth, _, _ = bf.search_batched(queries, k)
    lines = []
    for route in ("flat", "hier"):
        if route == "flat":
            ix, rep, trep, _ = build_flat(hip, bf, a.flat_leaves, a.S, a.K, a.kmeans_iters, a.pq_iters)
        else:
            ix, rep, trep, _ = build_hier(hip, bf, a.children, a.depth, a.S, a.K, a.kmeans_iters, a.pq_iters)
        leaves = trep["num_leaves"] if trep else a.flat_leaves

        def run(P):
            o = hip.default_opts()
            o.partitions_to_search, o.pre_reorder_k = P, m
            idx = ix.search_batched(queries, k, o)[0]
            rec = sum(len(set(idx[i].tolist()) & set(truth[i].tolist())) for i in range(queries.shape[0])) / float(
                queries.shape[0] * k)
            ts = []
            for _ in range(a.reps + 1):
                t = time.perf_counter()
                ix.search_batched(queries, k, o)
                ts.append(time.perf_counter() - t)
            return rec, queries.shape[0] / float(np.median(ts[1:]))

        points = {}
        for P in P_GRID:
            if P > leaves:
                break
            points[P] = run(P)
            if points[P][0] >= 0.95 and P >= 10:
                break
        p95 = next((P for P in sorted(points) if points[P][0] >= 0.95), None)
        ln = dict(route=route, n=n, dim=dim, leaves=leaves, pre_reorder_k=m, queries=int(queries.shape[0]),
                  recall_at_P10=points[10][0], qps_at_P10=points[10][1], P_for_recall_095=p95,
                  recall_at_that_P=points[p95][0] if p95 else None, qps_at_that_P=points[p95][1] if p95 else None,
                  grid={str(P): dict(recall=v[0], qps=v[1]) for P, v in points.items()})
        lines.append(ln)
        write(out, lines)
        print(json.dumps({kk: vv for kk, vv in ln.items() if kk != "grid"}), flush=True)
        ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="time", choices=["time", "quality", "big", "trace"])
    ap.add_argument("--num-points", dest="n", type=int, default=None)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kmeans-iters", type=int, default=100)
    ap.add_argument("--pq-iters", type=int, default=25)
    ap.add_argument("--subspaces", dest="S", type=int, default=32)
    ap.add_argument("--codes", dest="K", type=int, default=16)
    ap.add_argument("--flat-leaves", type=int, default=None)
    ap.add_argument("--children", type=int, default=None)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--eval-queries", type=int, default=1024)
    ap.add_argument("--pre-reorder-k", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (before the library is loaded: both then share one HIP runtime, as in bench.py)
    from scann_rust_amd import hip
    big = a.mode == "big"
    n = a.n or (10_000_000 if big else 1_000_000)
    a.flat_leaves = a.flat_leaves or (10_000 if big else 1024)
    a.children = a.children or (100 if big else 32)
    dim, stride = a.dim, hip.compute_stride(a.dim)
    rows, queries = rows_and_queries(n, dim, a.eval_queries)
    if stride != dim:
        data = np.zeros((n, stride), np.float32)
        data[:, :dim] = rows
    else:
        data = rows
    bf = hip.bf_create(data, n, dim, stride, hip.SQUARED_L2)
    name = "%dm%d" % (n // 1_000_000, dim) if n % 1_000_000 == 0 else "%dx%d" % (n, dim)
    prof = os.path.join(ROOT, "profiles")
    if a.mode == "trace":
        ix, rep, trep, call = build_hier(hip, bf, a.children, a.depth, a.S, a.K, a.kmeans_iters, a.pq_iters)
        print("hierarchical build call %.3f s, %d leaves" % (call, trep["num_leaves"]), flush=True)
        ix.close()
    elif a.mode == "quality":
        quality(a, hip, bf, rows, queries, n, dim, a.out or os.path.join(prof, "hier_build_%s_quality.jsonl" % name))
    elif big:
        timing(a, hip, bf, n, dim, a.flat_leaves, a.children, a.depth, 3, "-capped-3-iterations",
               a.out or os.path.join(prof, "hier_build_%s_time.jsonl" % name))
    else:
        timing(a, hip, bf, n, dim, a.flat_leaves, a.children, a.depth, a.kmeans_iters, "",
               a.out or os.path.join(prof, "hier_build_%s_time.jsonl" % name))
    bf.close()


if __name__ == "__main__":
    main()

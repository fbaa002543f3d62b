#!/usr/bin/env python3
"""Times the sparse brute-force search (hip.SparseIndex) on a seeded learned-sparse-like workload:
dimensionality 30 522, Zipf-distributed dimensions, about 128 stored entries per row and about 32 per query, k = 10,
DotProduct, batches of 1024 queries.

Per handle size it prints one JSON line: QPS (host clock around calls that end in a synchronise), the scan and merge
kernels' device-event times (median and range over the repeats), the scan's achieved bytes/s -- nnz * 8 B, one read of
the CSR entries, over the scan time -- next to the HBM peak (bandwidth is the bound it is compared with), the bytes/s
the workgroups requested (every query tile reads the entries again, mostly from L2), and the mean hash-map probes per
element and the share of elements found in the map (hits) from one more, untimed batch with the counters on.

Where the scan's time goes is measured by subtraction, with two variant builds of the library whose answers are wrong
on purpose (made where the compiler is, next to libscann_hip.so, before the run):

    python -c "from scann_rust_amd import build as b; b.build_variant('sparse_noprobe', ['-DSCANN_SPARSE_SKIP_PROBE'], only=('sparse.hip',)); b.build_variant('sparse_nowalk', ['-DSCANN_SPARSE_SKIP_WALK'], only=('sparse.hip',))"

`noprobe` streams the CSR entries and runs the epilogue and the selection, `nowalk` also probes the map and reads the
slot but lets every hit be used once by its own lane; the full kernel adds the ordered walk.  With --variants the tool
runs itself once per variant found (a fresh process, SCANN_HIP_LIB) at the small size and prints their lines, labelled.

The baseline is the only other route to the same answer: the same rows densified into a brute-force handle at
dim = 30 522 (n = 100 000: 12.2 GB), the same queries densified.  The two routes are timed alternately in one run; the
dense route sums in another order, so the top-10 lists are compared by overlap.

--inverted times the posting-list route (SparseIndex.build_postings) against the exhaustive one instead: two handles over
the same arrays, 3 warm-ups, at least 10 batches each, alternating; one JSON line per size with both routes' QPS and
kernel times, the postings visited per query, the bytes of the two layouts and the posting build time.

    python tools/time_sparse.py [--n 1000000] [--n-small 100000] [--batch 1024] [--reps 5] [--no-dense] [--variants] [--inverted]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scann_rust_amd import hip  # noqa: E402

HBM = 8.0e12   # MI355X HBM3E peak, bytes/s: the bound the scan's bytes/s is set against
D, K = 30522, 10
PERM = np.random.default_rng(7).permutation(D).astype(np.uint32)   # rank -> dimension, one law for rows and queries: the frequent dimensions of the rows are the frequent ones of the queries, spread over the vocabulary


def zipf_lists(rng, n, draws, block=65536):
    """n ascending duplicate-free dimension lists from `draws` Zipf(1) draws each, with U[-1, 1) values, as CSR"""
    cdf = np.cumsum(1.0 / np.arange(1, D + 1))
    cdf /= cdf[-1]
    dims, lens = [], []
    for s in range(0, n, block):
        m = min(block, n - s)
        d = np.sort(PERM[np.searchsorted(cdf, rng.random((m, draws), dtype=np.float32))], axis=1)
        keep = np.ones(d.shape, bool)
        keep[:, 1:] = d[:, 1:] != d[:, :-1]
        dims.append(d[keep])
        lens.append(keep.sum(1))
    dims = np.concatenate(dims)
    off = np.concatenate([[0], np.cumsum(np.concatenate(lens))]).astype(np.uint64)
    return off, dims, rng.uniform(-1, 1, dims.size).astype(np.float32)


def densify(csr, n, width):
    off, dims, vals = csr
    x = np.zeros((n, width), np.float32)
    x[np.repeat(np.arange(n), np.diff(off.astype(np.int64))), dims] = vals
    return x


def spread(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def time_inverted(a, csr, n, queries):
    """The exhaustive and the posting-list route over the same rows in one process: two handles made from the same
    arrays (a handle with postings always takes them), 3 warm-ups, then the two alternate.  One JSON line."""
    nnz = int(csr[1].size)
    ex = hip.SparseIndex(*csr, dimensionality=D)
    inv = hip.SparseIndex(*csr, dimensionality=D)
    t0 = time.perf_counter()
    inv.build_postings()
    build_s = time.perf_counter() - t0
    for _ in range(3):
        want = ex.search_batched(queries, K)
        got = inv.search_batched(queries, K)
    same = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(want, got))
    t = {"ex": ([], [], []), "inv": ([], [], [])}
    for _ in range(max(a.reps, 10)):
        for name, ix in (("ex", ex), ("inv", inv)):
            t0 = time.perf_counter()
            ix.search_batched(queries, K)
            t[name][0].append(time.perf_counter() - t0)
            ms = ix.last_kernel_ms()
            t[name][1].append(ms[0])
            t[name][2].append(ms[1])
    inv.enable_stats(True)
    inv.search_batched(queries, K)
    info = inv.postings_info()
    out = {"route": "postings_vs_exhaustive", "build": a.label, "n": n, "nnz": nnz, "batch": a.batch, "k": K, "same_bits": same,
           "block_rows": info["block_rows"], "blocks": info["blocks"], "chunks": info["chunks"], "build_postings_s": round(build_s, 3),
           "postings_bytes": info["bytes"], "csr_bytes": ex.device_bytes(),
           "visited_per_query": round(info["visited"] / a.batch, 1), "visited_share_of_entries": round(info["visited"] / a.batch / nnz, 5)}
    for name, label in (("ex", "exhaustive"), ("inv", "postings")):
        out[label] = {"qps": round(a.batch / float(np.median(t[name][0])), 1), "call_ms": spread([w * 1e3 for w in t[name][0]]),
                      "scan_ms": spread(t[name][1]), "merge_ms": spread(t[name][2])}
    print(json.dumps(out), flush=True)
    ex.close()
    inv.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inverted", action="store_true", help="time the posting-list route against the exhaustive one, nothing else")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--n-small", type=int, default=100_000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-dense", action="store_true")
    ap.add_argument("--variants", action="store_true")
    ap.add_argument("--only-small", action="store_true")
    ap.add_argument("--label", default="full")
    a = ap.parse_args()
    rng = np.random.default_rng(42)
    rows = zipf_lists(rng, a.n, 175)
    queries = zipf_lists(rng, a.batch, 40)
    small = (rows[0][:a.n_small + 1], rows[1][:int(rows[0][a.n_small])], rows[2][:int(rows[0][a.n_small])])

    if a.inverted:
        for csr, n in ((small, a.n_small),) if a.only_small else ((small, a.n_small), (rows, a.n)):
            time_inverted(a, csr, n, queries)
        return

    dense = dense_q = None
    if not a.no_dense:
        try:
            stride = hip.compute_stride(D)
            x = densify(small, a.n_small, stride)
            dense = hip.bf_create(x, a.n_small, D, stride, hip.DOT_PRODUCT)
            del x
            dense_q = densify(queries, a.batch, stride)
            dense.search_batched(dense_q, K, q_dim=D)   # (a dimensionality ceiling shows here, not at create)
        except (hip.ScannError, MemoryError) as e:
            print(json.dumps({"route": "dense", "n": a.n_small, "refused": str(e)}), flush=True)
            dense = None

    for csr, n in ((small, a.n_small),) if a.only_small else ((small, a.n_small), (rows, a.n)):
        ix = hip.SparseIndex(*csr, dimensionality=D)
        nnz = int(csr[1].size)
        idx, _, _ = ix.search_batched(queries, K)   # warm-up: code objects, workspaces
        both = dense is not None and n == a.n_small
        if both:
            didx, _, _ = dense.search_batched(dense_q, K, q_dim=D)
        wall, scan, merge, dwall = [], [], [], []
        for _ in range(a.reps):   # the two routes alternate
            t0 = time.perf_counter()
            ix.search_batched(queries, K)
            wall.append(time.perf_counter() - t0)
            ms = ix.last_kernel_ms()
            scan.append(ms[0])
            merge.append(ms[1])
            if both:
                t0 = time.perf_counter()
                dense.search_batched(dense_q, K, q_dim=D)
                dwall.append(time.perf_counter() - t0)
        plan = ix.last_plan()
        ix.enable_stats(True)
        ix.search_batched(queries, K)
        st = ix.last_plan()
        bytes_read = nnz * 8   # one read of the CSR entries per batch: what the algorithm needs from HBM
        out = {"route": "sparse", "build": a.label, "n": n, "nnz_per_row": round(nnz / n, 1), "nnz_per_query": round(queries[1].size / a.batch, 1),
               "batch": a.batch, "k": K, "tiles": plan["tiles"], "chunks": plan["chunks"],
               "qps": round(a.batch / float(np.median(wall)), 1), "call_ms": spread([w * 1e3 for w in wall]),
               "scan_ms": spread(scan), "merge_ms": spread(merge),
               "scan_bytes_per_s": round(bytes_read / (float(np.median(scan)) * 1e-3), 1), "hbm_peak_bytes_per_s": HBM,
               "scan_fraction_of_hbm_peak": round(bytes_read / (float(np.median(scan)) * 1e-3) / HBM, 4),
               "scan_requested_bytes_per_s": round(bytes_read * plan["tiles"] / (float(np.median(scan)) * 1e-3), 1),
               "probes_per_element": round(st["probes"] / max(st["elements"], 1), 3),
               "hits_per_element": round(st["hits"] / max(st["elements"], 1), 4), "device_bytes": ix.device_bytes()}
        print(json.dumps(out), flush=True)
        if both:
            overlap = np.mean([len(set(idx[i]) & set(didx[i])) / K for i in range(a.batch)])
            print(json.dumps({"route": "dense", "n": n, "dim": D, "batch": a.batch, "k": K,
                              "qps": round(a.batch / float(np.median(dwall)), 1), "call_ms": spread([w * 1e3 for w in dwall]),
                              "device_bytes": dense.device_bytes(), "top10_overlap_with_sparse": round(float(overlap), 4),
                              "sparse_over_dense_qps": round(float(np.median(dwall)) / float(np.median(wall)), 2)}), flush=True)
        ix.close()
    if a.variants:
        for name in ("noprobe", "nowalk"):
            lib = os.path.join(ROOT, "scann_rust_amd", "libscann_hip_sparse_%s.so" % name)
            if os.path.exists(lib):
                subprocess.check_call([sys.executable, os.path.abspath(__file__), "--no-dense", "--only-small", "--label", name,
                                       "--n", str(a.n), "--n-small", str(a.n_small), "--batch", str(a.batch), "--reps", str(a.reps)],
                                      env=dict(os.environ, SCANN_HIP_LIB=lib))


if __name__ == "__main__":
    main()

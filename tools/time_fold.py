#!/usr/bin/env python3
"""Times scann_hip_fold_mutable against what it replaces: 1M x 128 uniform rows, a delta of 16 384 rows and
1 % of the base removed (row (e) of the 3.3f table), on

  tree  1000 leaves (centres = sampled rows, frozen), S = 32, K = 16, residual codes, partitions_to_search 10
  ah    the flat hasher of the README table (S = 32, K = 16, pre_reorder_k = 5000)
  bf    the brute-force DotProduct index of the README table

Per index, alternating in one process (1 warm-up round, medians of `repeats` rounds, the mutations outside the clock):
  fold     Mutable.fold(): rows, codes and ids stay on the device
  rebuild  the route of the parent commit: export_live, assign + encode of ALL live rows with the frozen model through
           the build helpers (bf_create + bf_assign_nearest, encode), the CSR on the host, txh_create / bf_create, rebase
then the search per batch of `nq` queries through the handle before and after the fold, beside the plain search of an
index built from the same rows (with that plain search's own spread over two interleaved series), and the fold's stage
times: HIP-event spans over the kernels of a stage and nothing else (every allocation and upload of the fold comes
before the first event, the offsets' read-back lies between two spans), with the bytes the row gather and the scatter
move as a share of the measured HBM copy rate.  A span still holds the launch gaps between its kernels; for single
kernels run the tool under a kernel trace.  One JSON line per point; --write puts them into
profiles/fold_1m128_time.jsonl.

    python tools/time_fold.py [tree|ah|bf|all] [n] [nq] [repeats] [delta rows] [--write] [--fold-only]

--fold-only skips the search series (for a second delta size or a kernel trace).
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
nq = int(args[2]) if len(args) > 2 else 1024
repeats = int(args[3]) if len(args) > 3 else 5
dim, k, S, K, m, L, P = 128, 10, 32, 16, 5000, 1000, 10
ND = int(args[4]) if len(args) > 4 else 16384
HBM_COPY_TBS = 6.29   # measured float4 copy rate of the MI355X (read + write bytes per second)
if not torch.cuda.is_available():
    sys.exit("time_fold.py needs the GPU: a timing taken elsewhere says nothing")

rows = synth.uniform_f32(n, dim, 42)
q = synth.uniform_f32(nq, dim, 123)
fresh = synth.uniform_f32(ND, dim, 77)
gone = np.arange(0, n, 100, dtype=np.uint32)
lines = []


def med(v):
    return round(statistics.median(v), 4)


def spread(v):
    return [round(min(v), 4), round(max(v), 4)]


def model(kind):
    """the frozen model: (centres or None, codebook or None)"""
    if kind == "bf":
        return None, None
    sample = synth.uniform_rows((synth.splitmix64(0xC0DE, 0, 65536) % np.uint64(n)).astype(np.int64), dim, 42)
    centers = np.ascontiguousarray(sample[:L]) if kind == "tree" else None
    train = sample - centers[hip.bf_assign_nearest(hip.bf_create(sample, sample.shape[0], dim, dim, hip.SQUARED_L2), centers,
                                                   want_dist=False)] if kind == "tree" else sample
    return centers, trainer.train_codebook(np.ascontiguousarray(train), S, K, iters=10, seed=42, sample=1 << 30)


def build(kind, centers, codebook, data):
    """the index over `data` with the model frozen, through the existing build helpers"""
    cnt = data.shape[0]
    if kind == "bf":
        return hip.bf_create(data, cnt, dim, dim, hip.DOT_PRODUCT)
    if kind == "ah":
        return hip.txh_create(data=data, n_rows=cnt, dim=dim, stride=dim, centers=None, leaf_offsets=None, leaf_ids=None,
                              codebook=codebook, codes=hip.encode(codebook, data, stride=dim), use_residuals=False,
                              partitions_to_search=1, pre_reorder_multiplier=float(m) / k)
    tmp = hip.bf_create(data, cnt, dim, dim, hip.SQUARED_L2)
    tok = hip.bf_assign_nearest(tmp, centers, want_dist=False)
    tmp.close()
    codes = hip.encode(codebook, data, stride=dim, centers=centers, leaf_of_row=tok)
    order = np.argsort(tok, kind="stable").astype(np.uint32)
    off = np.zeros(L + 1, np.uint32)
    off[1:] = np.cumsum(np.bincount(tok, minlength=L))
    return hip.txh_create(data=data, n_rows=cnt, dim=dim, stride=dim, centers=centers, leaf_offsets=off, leaf_ids=order,
                          codebook=codebook, codes=np.ascontiguousarray(codes[order]), use_residuals=True,
                          partitions_to_search=P, pre_reorder_multiplier=float(m) / k)


def mutated(base):
    mut = hip.Mutable(base, ND)   # (a fresh handle every round: its first fold allocates everything it uses)
    for i in range(0, ND, 1024):
        mut.add(fresh[i:i + 1024])
    mut.remove(gone)
    return mut


def series(fns, reps):
    t = {name: [] for name, _ in fns}
    for r in range(reps + 3):
        for name, fn in fns:
            t0 = time.perf_counter()
            fn()
            if r >= 3:
                t[name].append((time.perf_counter() - t0) * 1e3)
    return t


def run(kind):
    centers, codebook = model(kind)
    base = build(kind, centers, codebook, rows)
    opts = hip.default_opts()
    if kind != "bf":
        opts.pre_reorder_k = m
    fold_ms, rebuild_ms, stages = [], [], []
    for r in range(repeats + 1):
        mut = mutated(base)
        t0 = time.perf_counter()
        folded, ids = mut.fold()
        t1 = time.perf_counter()
        st = mut.fold_stage_ms()
        mut.close()
        folded.close()
        mut = mutated(base)
        t2 = time.perf_counter()
        er, ei = mut.export_live()
        rebuilt = build(kind, centers, codebook, er)
        mut.rebase(rebuilt, ei)
        t3 = time.perf_counter()
        mut.close()
        rebuilt.close()
        assert np.array_equal(ids, ei)
        if r:
            fold_ms.append((t1 - t0) * 1e3)
            rebuild_ms.append((t3 - t2) * 1e3)
            stages.append(st)
    n_live = int(ei.size)
    st = [med([s[i] for s in stages]) for i in range(5)]
    nw = S // 8
    gather_bytes = 2 * n_live * dim * 4
    scatter_bytes = 2 * n_live * (nw * 4 + (4 if kind == "tree" else 0)) if kind != "bf" else 0
    line = {"index": kind, "point": "fold against export + rebuild + rebase", "n": n, "dim": dim, "delta_rows": ND,
            "removed": int(gone.size), "live_rows": n_live, "repeats": repeats,
            "fold_ms": med(fold_ms), "fold_spread_ms": spread(fold_ms),
            "rebuild_ms": med(rebuild_ms), "rebuild_spread_ms": spread(rebuild_ms),
            "speedup": round(med(rebuild_ms) / med(fold_ms), 2),
            "stage_ms": dict(zip(["row_gather", "delta_assign_encode", "count_scans", "scatter", "finish"], st)),
            "row_gather_bytes": gather_bytes, "scatter_bytes": scatter_bytes,
            "row_gather_of_hbm_copy": round(gather_bytes / (st[0] * 1e-3) / 1e12 / HBM_COPY_TBS, 4) if st[0] > 0 else None,
            "scatter_of_hbm_copy": round(scatter_bytes / (st[3] * 1e-3) / 1e12 / HBM_COPY_TBS, 4) if st[3] > 0 else None}
    lines.append(line)
    print(json.dumps(line), flush=True)
    if "--fold-only" in sys.argv:
        base.close()
        return
    # ---- search per batch: through the handle before and after the fold, beside a plain index over the same rows
    mut = mutated(base)
    er, ei = mut.export_live()
    plain_ix = build(kind, centers, codebook, er)
    plain = lambda: plain_ix.search_batched(q, k, opts=opts)
    msearch = lambda: mut.search_batched(q, k, opts=opts)
    t_before = series([("a", plain), ("a2", plain), ("x", msearch)], 11)
    folded, ids = mut.fold()
    fsearch = lambda: folded.search_batched(q, k, opts=opts)
    t_after = series([("a", plain), ("a2", plain), ("x", msearch), ("f", fsearch)], 11)
    both = t_after["a"] + t_after["a2"]
    line = {"index": kind, "point": "search per batch before and after the fold", "nq": nq, "k": k, "repeats": 11,
            "before_fold_ms": med(t_before["x"]), "before_fold_spread_ms": spread(t_before["x"]),
            "after_fold_ms": med(t_after["x"]), "after_fold_spread_ms": spread(t_after["x"]),
            "folded_base_direct_ms": med(t_after["f"]),
            "plain_ms": med(t_after["a"]), "plain_again_ms": med(t_after["a2"]), "plain_spread_ms": spread(both),
            "after_over_plain_ms": round(med(t_after["x"]) - med(both), 4)}
    lines.append(line)
    print(json.dumps(line), flush=True)
    mut.close()
    folded.close()
    plain_ix.close()
    base.close()


for kind in (("tree", "ah", "bf") if which == "all" else (which,)):
    run(kind)
if "--write" in sys.argv:
    with open(os.path.join(ROOT, "profiles", "fold_1m128_time.jsonl"), "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")

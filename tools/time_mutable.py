#!/usr/bin/env python3
"""Times the mutable index against the plain search of its base: 1M x 128 uniform rows, batch 1024, k = 10,
host entry points (queries go up and rows come back in every call), on

  bf   the brute-force DotProduct index of the README table
  ah   the flat hasher of the README table (S = 32, K = 16, pre_reorder_k = 5000)

Points, alternating in one loop per configuration (3 warm-ups, medians of `repeats` timed batches):
  (a) plain search on the base            (a2) the same again: the spread of the plain search's own repeated runs
  (b) mutable search, no mutation         -- IS the plain search: must sit inside the spread of (a)
  (c) delta of 1024 / 16384 rows, no removal
  (d) 1 % of the base rows removed, empty delta
  (e) both
with the handle's stage events (base pass, delta scan, merge) for (c)-(e), the delta scan's rate against the f32 VALU
peak, a 1024-row add batch and one export_live.  One JSON line per point; --write puts them into
profiles/mutable_1m128_time.jsonl.

    python tools/time_mutable.py [bf|ah|both] [n] [nq] [repeats] [--write]

(a) across two commits: `--plain-only --label=NAME` times the plain search alone (it needs nothing of the mutable layer,
so the same file runs from a checkout of the parent commit) and, with --append, adds its line to the profile of the
checkout it runs in.  Run it alternately, a fresh process per run, from a built checkout of each commit, so that a
drift of the machine lands on both.
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
which = args[0] if len(args) > 0 else "both"
n = int(args[1]) if len(args) > 1 else 1_000_000
nq = int(args[2]) if len(args) > 2 else 1024
repeats = int(args[3]) if len(args) > 3 else 11
dim, k, S, K, m = 128, 10, 32, 16, 5000
VALU_PEAK_TFLOPS = 157.3   # f32 vector peak of the MI355X (FMA = 2 FLOP)
if not torch.cuda.is_available():
    sys.exit("time_mutable.py needs the GPU: a timing taken elsewhere says nothing")

rows = synth.uniform_f32(n, dim, 42)
q = synth.uniform_f32(nq, dim, 123)
fresh = synth.uniform_f32(16384, dim, 77)
lines = []


def timed(fns, reps):
    """{name: [ms]}: the functions called in turn, `reps` rounds after 3 warm-up rounds"""
    t = {name: [] for name, _ in fns}
    for r in range(reps + 3):
        for name, fn in fns:
            t0 = time.perf_counter()
            fn()
            if r >= 3:
                t[name].append((time.perf_counter() - t0) * 1e3)
    return t


def med(v):
    return round(statistics.median(v), 4)


def run(kind):
    opts = hip.default_opts()
    if kind == "bf":
        base = hip.bf_create(rows, n, dim, dim, hip.DOT_PRODUCT)
    else:
        sample = synth.uniform_rows((synth.splitmix64(0xC0DE, 0, 65536) % np.uint64(n)).astype(np.int64), dim, 42)
        codebook = trainer.train_codebook(sample, S, K, iters=25, seed=42, sample=1 << 30)
        codes = hip.encode(codebook, rows, stride=dim)
        base = hip.txh_create(data=rows, n_rows=n, dim=dim, stride=dim, centers=None, leaf_offsets=None, leaf_ids=None,
                              codebook=codebook, codes=codes, use_residuals=False, partitions_to_search=1,
                              pre_reorder_multiplier=float(m) / k)
        opts.pre_reorder_k = m
    plain = lambda: base.search_batched(q, k, opts=opts)
    if "--plain-only" in sys.argv:
        t = timed([("a", plain)], repeats)
        label = ([a.split("=", 1)[1] for a in sys.argv if a.startswith("--label=")] or [""])[0]
        line = {"index": kind, "point": "a: plain search", "build": label, "n": n, "dim": dim, "nq": nq, "k": k,
                "repeats": repeats, "plain_ms": med(t["a"]), "plain_spread_ms": [round(min(t["a"]), 4), round(max(t["a"]), 4)]}
        lines.append(line)
        print(json.dumps(line), flush=True)
        base.close()
        return
    mut = hip.Mutable(base, 16384)
    mut.enable_timing(True)
    msearch = lambda: mut.search_batched(q, k, opts=opts)

    def point(name, extra):
        t = timed([("a", plain), ("a2", plain), ("x", msearch)], repeats)
        msearch()
        stages = mut.last_stage_ms()
        line = {"index": kind, "point": name, "n": n, "dim": dim, "nq": nq, "k": k, "repeats": repeats,
                "plain_ms": med(t["a"]), "plain_again_ms": med(t["a2"]),
                "plain_spread_ms": [round(min(t["a"] + t["a2"]), 4), round(max(t["a"] + t["a2"]), 4)],
                "mutable_ms": med(t["x"]), "mutable_spread_ms": [round(min(t["x"]), 4), round(max(t["x"]), 4)],
                "over_plain_ms": round(med(t["x"]) - med(t["a"]), 4),
                "base_pass_ms": round(stages[0], 4), "delta_scan_ms": round(stages[1], 4), "merge_ms": round(stages[2], 4)}
        line.update(extra)
        if stages[1] > 0:
            nd = extra["delta_rows"]
            tf = 2.0 * nq * nd * dim / (stages[1] * 1e-3) / 1e12
            line["delta_scan_tflops"] = round(tf, 3)
            line["delta_scan_of_valu_peak"] = round(tf / VALU_PEAK_TFLOPS, 4)
        lines.append(line)
        print(json.dumps(line), flush=True)

    point("b: no mutation", {"delta_rows": 0, "removed": 0})
    # a 1024-row add batch (timed once per batch, over the first eight), then the delta points
    add_ms = []
    for i in range(16):
        t0 = time.perf_counter()
        mut.add(fresh[i * 1024:(i + 1) * 1024])
        add_ms.append((time.perf_counter() - t0) * 1e3)
        if i == 0:
            point("c: delta 1024", {"delta_rows": 1024, "removed": 0})
    point("c: delta 16384", {"delta_rows": 16384, "removed": 0})
    gone = np.arange(0, n, 100, dtype=np.uint32)
    t0 = time.perf_counter()
    mut.remove(gone)
    remove_ms = (time.perf_counter() - t0) * 1e3
    point("e: delta 16384, 1 % removed", {"delta_rows": 16384, "removed": int(gone.size)})
    t0 = time.perf_counter()
    er, ei = mut.export_live()
    export_ms = (time.perf_counter() - t0) * 1e3
    assert ei.size == mut.size()
    mut.remove(np.arange(n, n + 16384, dtype=np.uint32))
    point("d: 1 % removed, empty delta", {"delta_rows": 0, "removed": int(gone.size)})
    line = {"index": kind, "point": "mutations", "add_1024_rows_ms": med(add_ms), "remove_%d_ids_ms" % gone.size: round(remove_ms, 3),
            "export_live_ms": round(export_ms, 2), "exported_rows": int(ei.size)}
    lines.append(line)
    print(json.dumps(line), flush=True)
    mut.close()
    base.close()


for kind in (("bf", "ah") if which == "both" else (which,)):
    run(kind)
if "--append" in sys.argv:
    with open(os.path.join(ROOT, "profiles", "mutable_1m128_time.jsonl"), "a") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")
if "--write" in sys.argv:
    with open(os.path.join(ROOT, "profiles", "mutable_1m128_time.jsonl"), "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")

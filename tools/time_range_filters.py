#!/usr/bin/env python3
"""Times the attribute table's range kernel under the conditions of tools/time_token_filters.py: 1M rows, batch 1024,
inputs resident on the device, wall time of the call plus a stream synchronise, medians of `repeats` runs with the
routes alternating in one loop.

  A  block build.  Columns: ts (i64, a random permutation of the rows), price (f32, uniform [0, 1)), qty (i64, uniform
     0..999).  Every query allows about 10 % of the rows:
       one_i64     ts in a window of n / 10                                        op 0
       one_f32     price in a window of 0.1                                         op 0
       two         ts in a window of n / 5 AND price <= 0.5                         op 0
       four        ts window of n / 2 AND price <= 0.5 AND qty <= 799 AND row index in the upper half      op 0
       and_i64     the one_i64 ranges ANDed into an existing block (a random 50 % block), op AND
     Beside each: (1) a device fill of the same block in the same loop, a measured streaming store of the same bytes;
     (2) what a caller does today for the same allowed rows: scann_hip_allow_bitmaps_from_ids_device over id lists
     made on the host (for and_i64: into a second block, then scann_hip_allow_bitmaps_combine_device), with the host
     time to make the lists and their upload reported separately (taken once, not in the loop).
  B  the filtered tree search end to end, 1M x 128, 1000 leaves, P = 10, m = 1000, k = 10, under the `two` ranges:
     device-resident routes (build the block, search, one stream, one synchronise) by the table and by the id lists,
     the search alone, and the two host-pointer entries: scann_hip_search_batched_ranges, and scann_hip_search_batched
     under the block built on the host (its upload included, the host time to evaluate the ranges not).

The blocks of the two routes are compared bitwise before anything is timed.

    python tools/time_range_filters.py [n] [nq] [repeats] [--write] [--skip-search]

One JSON line per workload, appended to profiles/range_filters_1m_time.jsonl with --write."""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from scann_rust_amd import hip, synth  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 1_000_000
nq = int(args[1]) if len(args) > 1 else 1024
repeats = int(args[2]) if len(args) > 2 else 9
dim, S, k = 128, 32, 10
if not torch.cuda.is_available():
    sys.exit("time_range_filters.py needs the GPU: a timing taken elsewhere says nothing")
L = hip.load()
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream()
sptr = ctypes.c_void_p(stream.cuda_stream)
p = lambda t: ctypes.c_void_p(t.data_ptr())
u64 = lambda t: ctypes.cast(p(t), ctypes.POINTER(ctypes.c_uint64))
words = -(-n // 64)
lib = os.path.basename(hip.LIB_PATH)
ROW = hip.ATTR_ROW_INDEX


def median_ms(fns, reps):
    """medians of the functions' wall times, the functions alternating in one loop"""
    for f in fns.values():
        f()
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, f in fns.items():
            t0 = time.perf_counter()
            f()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    return {name: round(statistics.median(v), 4) for name, v in ts.items()}, ts


def spread(v):
    """half the range of the runs around their median, in ms"""
    return round((max(v) - min(v)) / 2, 4)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype.itemsize == 8 else np.int32).reshape(-1).copy()).to(dev)


rng = np.random.default_rng(11)
ts_col = rng.permutation(n).astype(np.int64)
price = rng.random(n, dtype=np.float32)
qty = rng.integers(0, 1000, n).astype(np.int64)
columns = [ts_col, price, qty]
table = hip.AttrTable(n, columns)
a_ts = rng.integers(0, n - n // 2, nq).astype(np.int64)
a_pr = (rng.random(nq) * 0.9).astype(np.float32)
inf = np.float32(np.inf)
WORKLOADS = {
    "one_i64": ([0], [a_ts], [a_ts + n // 10 - 1], 0),
    "one_f32": ([1], [a_pr], [a_pr + np.float32(0.1)], 0),
    "two": ([0, 1], [a_ts, -inf], [a_ts + n // 5 - 1, np.float32(0.5)], 0),
    "four": ([0, 1, 2, ROW], [a_ts, -inf, 0, n // 2], [a_ts + n // 2 - 1, np.float32(0.5), 799, n], 0),
    "and_i64": ([0], [a_ts], [a_ts + n // 10 - 1], hip.ALLOW_AND),
}
block_mb = nq * words * 8 / 1e6


def host_id_lists(cols, lo, hi):
    """what a caller does today: the predicate per query on the host, the allowed rows as id lists"""
    values = [np.arange(n, dtype=np.int64) if c == ROW else columns[c] for c in cols]
    lists = []
    for q in range(nq):
        m = np.ones(n, bool)
        for v, l, h in zip(values, lo, hi):
            m &= (v >= (l[q] if np.ndim(l) else l)) & (v <= (h[q] if np.ndim(h) else h))
        lists.append(np.flatnonzero(m).astype(np.uint32))
    return lists


def workload(name, cols, lo, hi, op):
    b = hip._range_bounds(table.clause_types(cols), lo, hi)
    d_b = to_dev(b)
    t0 = time.perf_counter()
    lists = host_id_lists(cols, lo, hi)
    ids = np.concatenate(lists)
    off = np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.uint64)
    host_lists_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    d_ids, d_off = to_dev(ids), to_dev(off)
    torch.cuda.synchronize()
    upload_s = time.perf_counter() - t0
    blk_ids = torch.empty((nq, words), dtype=torch.int64, device=dev)
    blk_rng = torch.full((nq, words), -1, dtype=torch.int64, device=dev)
    base = blk_tmp = None
    if op:   # the existing block both routes narrow: the same random half of the rows, restored before every run
        base = to_dev(np.random.default_rng(12).integers(0, 2 ** 63, (nq, words), dtype=np.uint64)).view(nq, words)
        if n % 64:
            base[:, -1] &= (1 << (n % 64)) - 1
        blk_tmp = torch.empty((nq, words), dtype=torch.int64, device=dev)

    def from_ids():
        if op:
            blk_ids.copy_(base)
            hip.allow_bitmaps_from_ids_device(d_ids.data_ptr(), d_off.data_ptr(), nq, n, words, blk_tmp.data_ptr(), stream.cuda_stream)
            hip.allow_bitmaps_combine_device(op, blk_ids.data_ptr(), words, blk_tmp.data_ptr(), words, nq, n, blk_ids.data_ptr(),
                                             words, stream.cuda_stream)
        else:
            hip.allow_bitmaps_from_ids_device(d_ids.data_ptr(), d_off.data_ptr(), nq, n, words, blk_ids.data_ptr(), stream.cuda_stream)
        stream.synchronize()

    def from_ranges():
        if op:
            blk_rng.copy_(base)
        table.allow_bitmaps_device(cols, d_b.data_ptr(), nq, words, blk_rng.data_ptr(), op, stream.cuda_stream)
        stream.synchronize()

    def fill():
        if op:   # (the restore both routes pay, so that it can be taken off)
            blk_tmp.copy_(base)
        else:
            blk_ids.zero_()
        stream.synchronize()

    from_ids()
    from_ranges()
    equal = bool(torch.equal(blk_ids, blk_rng))
    if not equal:
        sys.exit("%s: the two routes' blocks differ: nothing is timed" % name)
    med, ts = median_ms({"from_ids_ms": from_ids, "from_ranges_ms": from_ranges, "fill_block_ms": fill}, repeats)
    net = (lambda key: med[key] - med["fill_block_ms"]) if op else (lambda key: med[key])
    rec = dict(workload="A_" + name, lib=lib, n=n, nq=nq, repeats=repeats, tile_bits=hip.RANGE_TILE_BITS, blocks_equal=equal,
               clauses=len(cols), op=op, ids_per_query=round(ids.size / nq, 1), **med,
               fill_is="a device copy of the block (the restore both routes include)" if op else "a device fill of the block",
               from_ids_spread_ms=spread(ts["from_ids_ms"]), from_ranges_spread_ms=spread(ts["from_ranges_ms"]),
               ids_over_ranges=round(net("from_ids_ms") / net("from_ranges_ms"), 2),
               ranges_over_fill=round(net("from_ranges_ms") / med["fill_block_ms"], 2),
               bitmap_block_mb=round(block_mb, 1), id_lists_mb=round(ids.size * 4 / 1e6, 1),
               host_id_lists_s=round(host_lists_s, 2), id_lists_upload_s=round(upload_s, 3),
               runs_ms={key: [round(t, 3) for t in v] for key, v in ts.items()})
    print(json.dumps(rec), flush=True)
    return rec, (b, d_b, d_ids, d_off, blk_ids, blk_rng)


def tree_index():
    leaves, P = 1000, 10
    r2 = np.random.default_rng(5)
    rows = synth.clustered_f32(n, dim, 7, n_clusters=leaves)[0]
    centers = np.ascontiguousarray(rows[np.sort(r2.choice(n, leaves, replace=False))], np.float32)
    bf = hip.bf_create(rows, n, dim, dim, hip.SQUARED_L2)
    assign = hip.bf_assign_nearest(bf, centers, want_dist=False).astype(np.int64)
    bf.close()
    order = np.argsort(assign, kind="stable").astype(np.uint32)
    leaf_off = np.zeros(leaves + 1, np.uint32)
    leaf_off[1:] = np.cumsum(np.bincount(assign, minlength=leaves))
    cb = np.ascontiguousarray(rows[r2.choice(n, 16, replace=False)].reshape(16, S, dim // S).transpose(1, 0, 2), np.float32)
    codes = r2.integers(0, 16, (n, S), dtype=np.uint8)
    ix = hip.txh_create(data=rows, n_rows=n, dim=dim, stride=dim, centers=centers, leaf_offsets=leaf_off, leaf_ids=order,
                        codebook=cb, codes=codes, codes_packed4=False, use_residuals=True, partitions_to_search=P,
                        pre_reorder_multiplier=1.0)
    return ix, synth.clustered_f32(nq, dim, 8, n_clusters=leaves)[0], 1000, P


lines = []
keep = None
for name, (cols, lo, hi, op) in WORKLOADS.items():
    rec, kept = workload(name, cols, lo, hi, op)
    lines.append(rec)
    if name == "two":
        keep = (cols,) + kept
    del kept

if "--skip-search" not in sys.argv:
    cols, b, d_b, d_ids, d_off, blk_ids, blk_rng = keep
    ix, q, m, P = tree_index()
    qd = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    outs = [(torch.empty((nq, k), dtype=torch.int32, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev),
             torch.empty((nq,), dtype=torch.int32, device=dev)) for _ in range(2)]

    def opts(block):
        o = hip.default_opts()
        o.pre_reorder_k, o.partitions_to_search = m, P
        if block is not None:
            o.allow_bitmap, o.allow_bitmap_bits, o.allow_bitmap_stride = u64(block), n, words
        return o
    o_ids, o_rng, o_plain = opts(blk_ids), opts(blk_rng), opts(None)
    hip.check(L.scann_hip_index_reserve(ix.h, nq, k, ctypes.byref(o_plain)))

    def search(o, out):
        hip.check(L.scann_hip_search_batched_device(ix.h, p(qd), nq, dim, k, ctypes.byref(o), p(out[0]), p(out[1]), p(out[2]), sptr))

    def route_ids():
        hip.allow_bitmaps_from_ids_device(d_ids.data_ptr(), d_off.data_ptr(), nq, n, words, blk_ids.data_ptr(), stream.cuda_stream)
        search(o_ids, outs[0])
        stream.synchronize()

    def route_ranges():
        table.allow_bitmaps_device(cols, d_b.data_ptr(), nq, words, blk_rng.data_ptr(), 0, stream.cuda_stream)
        search(o_rng, outs[1])
        stream.synchronize()

    def search_only():
        search(o_rng, outs[1])
        stream.synchronize()

    host_block = blk_rng.cpu().numpy().view(np.uint64).reshape(nq, words)
    host_out = {}

    def entry_ranges():
        host_out["ranges"] = table.search_batched(ix, q, k, cols, b, o_plain)

    def entry_host_block():
        host_out["block"] = ix.search_batched(q, k, o_plain, allow=host_block, allow_bits=n)

    route_ids()
    s0 = L.scann_hip_index_last_device_status(ix.h, sptr)
    route_ranges()
    s1 = L.scann_hip_index_last_device_status(ix.h, sptr)
    same = bool(torch.equal(outs[0][2], outs[1][2]) and torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32)) and
                torch.equal(outs[0][0], outs[1][0]))
    if s0 != hip.OK or s1 != hip.OK or not same:
        sys.exit("B: statuses %d %d, rows equal: %s: nothing is timed" % (s0, s1, same))
    entry_ranges()
    entry_host_block()
    # (counts and distances bitwise; indices may differ inside ties between the two entries' pipelines)
    entries_same = np.array_equal(host_out["ranges"][2], host_out["block"][2]) and \
        np.array_equal(host_out["ranges"][1].view(np.uint32), host_out["block"][1].view(np.uint32)) and \
        np.array_equal(host_out["ranges"][2], outs[1][2].cpu().numpy().view(np.uint32))
    if not entries_same:
        sys.exit("B: the host-pointer entries' rows differ: nothing is timed")
    med, ts = median_ms({"ids_build_plus_search_ms": route_ids, "ranges_build_plus_search_ms": route_ranges,
                         "search_alone_ms": search_only, "search_batched_ranges_ms": entry_ranges,
                         "search_batched_host_block_ms": entry_host_block}, repeats)
    rec = dict(workload="B_tree_search_end_to_end", lib=lib, n=n, dim=dim, nq=nq, k=k, m=m, P=P, repeats=repeats, clauses=len(cols),
               rows_equal=same, entries_equal=entries_same, **med, ids_spread_ms=spread(ts["ids_build_plus_search_ms"]),
               ranges_spread_ms=spread(ts["ranges_build_plus_search_ms"]),
               ids_over_ranges=round(med["ids_build_plus_search_ms"] / med["ranges_build_plus_search_ms"], 2),
               filter_share_ranges=round(1 - med["search_alone_ms"] / med["ranges_build_plus_search_ms"], 3),
               host_block_over_ranges_entry=round(med["search_batched_host_block_ms"] / med["search_batched_ranges_ms"], 2),
               runs_ms={key: [round(t, 3) for t in v] for key, v in ts.items()})
    print(json.dumps(rec), flush=True)
    lines.append(rec)
    ix.close()

if "--write" in sys.argv:
    with open(os.path.join(ROOT, "profiles", "range_filters_1m_time.jsonl"), "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")

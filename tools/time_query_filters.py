#!/usr/bin/env python3
"""Times per-query allow-lists (scann_hip_search_opts.allow_bitmap_stride) on the two headline shapes, batch 1024,
k = 10, through the device entry with the bitmaps resident on the device:

    flat   1M x 128 flat hasher (S = 32, 4-bit codes), m = 5000
    tree   1M x 128, 1000 leaves, P = 10, m = 1000

  (a) the unfiltered search;
  (b) one shared 10 % bitmap (stride 0);
  (c) 1024 distinct 10 % bitmaps, by stride;
  (d) the same 1024 filtered queries as single-query device calls, each with its own bitmap: the only way before;
  (e) scann_hip_allow_bitmaps_from_ids_device for 1024 lists of 100 k ids (n / 10 each).

(c) against (b) is the cost of distinct bitmaps, (c) against (d) what the batch buys.  Medians of `repeats` runs, the
five alternating in one loop; one JSON line per shape, appended to profiles/query_filters_1m128_time.jsonl with --write.
The indexes are over explicit random codes (a codebook of 16 rows of the data set): the timing needs no training.
Rows of (c) are compared with (d)'s before anything is timed.

    python tools/time_query_filters.py [n] [nq] [repeats] [--write]
"""
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
    sys.exit("time_query_filters.py needs the GPU: a timing taken elsewhere says nothing")
L = hip.load()
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream()
sptr = ctypes.c_void_p(stream.cuda_stream)
p = lambda t: ctypes.c_void_p(t.data_ptr())
u64 = lambda t: ctypes.cast(p(t), ctypes.POINTER(ctypes.c_uint64))
words = -(-n // 64)
rng = np.random.default_rng(3)


def flat_index():
    rows = synth.uniform_f32(n, dim, 42)
    cb = np.ascontiguousarray(rows[rng.choice(n, 16, replace=False)].reshape(16, S, dim // S).transpose(1, 0, 2), np.float32)
    codes = rng.integers(0, 16, (n, S), dtype=np.uint8)
    ix = hip.txh_create(data=rows, n_rows=n, dim=dim, stride=dim, centers=None, leaf_offsets=None, leaf_ids=None,
                        codebook=cb, codes=codes, codes_packed4=False, use_residuals=False, partitions_to_search=1,
                        pre_reorder_multiplier=1.0)
    return ix, synth.uniform_f32(nq, dim, 123), 5000, 0


def tree_index():
    leaves, P = 1000, 10
    rows = synth.clustered_f32(n, dim, 7, n_clusters=leaves)[0]
    centers = np.ascontiguousarray(rows[np.sort(rng.choice(n, leaves, replace=False))], np.float32)
    bf = hip.bf_create(rows, n, dim, dim, hip.SQUARED_L2)
    assign = hip.bf_assign_nearest(bf, centers, want_dist=False).astype(np.int64)
    bf.close()
    order = np.argsort(assign, kind="stable").astype(np.uint32)
    leaf_off = np.zeros(leaves + 1, np.uint32)
    leaf_off[1:] = np.cumsum(np.bincount(assign, minlength=leaves))
    cb = np.ascontiguousarray(rows[rng.choice(n, 16, replace=False)].reshape(16, S, dim // S).transpose(1, 0, 2), np.float32)
    codes = rng.integers(0, 16, (n, S), dtype=np.uint8)
    ix = hip.txh_create(data=rows, n_rows=n, dim=dim, stride=dim, centers=centers, leaf_offsets=leaf_off, leaf_ids=order,
                        codebook=cb, codes=codes, codes_packed4=False, use_residuals=True, partitions_to_search=P,
                        pre_reorder_multiplier=1.0)
    return ix, synth.clustered_f32(nq, dim, 8, n_clusters=leaves)[0], 1000, P


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


lines = []
for shape, make in (("flat", flat_index), ("tree", tree_index)):
    ix, q, m, P = make()
    qd = torch.from_numpy(np.ascontiguousarray(q)).to(dev)
    oi = torch.empty((nq, k), dtype=torch.int32, device=dev)
    od = torch.empty((nq, k), dtype=torch.float32, device=dev)
    oc = torch.empty((nq,), dtype=torch.int32, device=dev)
    si = torch.empty((nq, k), dtype=torch.int32, device=dev)
    sd = torch.empty((nq, k), dtype=torch.float32, device=dev)
    sc = torch.empty((nq,), dtype=torch.int32, device=dev)
    # 1024 lists of n / 10 ids each, their bitmaps built on the device (e); the shared bitmap is list 0's
    per = n // 10
    ids = rng.integers(0, n, (nq, per), dtype=np.uint32)   # (drawn with replacement: 9.5 % of the rows per list)
    d_ids = torch.from_numpy(ids.view(np.int32).reshape(-1).copy()).to(dev)
    d_off = torch.from_numpy((np.arange(nq + 1, dtype=np.int64) * per)).to(dev)
    d_blk = torch.empty((nq, words), dtype=torch.int64, device=dev)

    def from_ids():
        hip.allow_bitmaps_from_ids_device(d_ids.data_ptr(), d_off.data_ptr(), nq, n, words, d_blk.data_ptr(),
                                          stream.cuda_stream)
        stream.synchronize()
    from_ids()

    def opts(stride, bitmap):
        o = hip.default_opts()
        o.pre_reorder_k = m
        if P:
            o.partitions_to_search = P
        if bitmap is not None:
            o.allow_bitmap, o.allow_bitmap_bits, o.allow_bitmap_stride = u64(bitmap), n, stride
        return o
    o_plain, o_shared, o_strided = opts(0, None), opts(0, d_blk[0]), opts(words, d_blk)
    o_single = [opts(0, d_blk[i]) for i in range(nq)]
    hip.check(L.scann_hip_index_reserve(ix.h, nq, k, ctypes.byref(o_plain)))

    def batch(o, wi=oi, wd=od, wc=oc):
        def run():
            hip.check(L.scann_hip_search_batched_device(ix.h, p(qd), nq, dim, k, ctypes.byref(o), p(wi), p(wd), p(wc), sptr))
            stream.synchronize()
        return run

    def singles():
        for i in range(nq):
            hip.check(L.scann_hip_search_batched_device(ix.h, p(qd[i]), 1, dim, k, ctypes.byref(o_single[i]), p(si[i]),
                                                        p(sd[i]), p(sc[i]), sptr))
        stream.synchronize()

    # (c) answers what (d) answers: the same counts and distances (indices may differ inside a tie)
    batch(o_strided)()
    status = L.scann_hip_index_last_device_status(ix.h, sptr)
    singles()
    same = bool(torch.equal(oc, sc) and torch.equal(od.view(torch.int32), sd.view(torch.int32)))
    if status != hip.OK or not same:
        sys.stderr.write("%s: strided batch status %d, rows equal to the single-query calls': %s\n" % (shape, status, same))
    med, ts = median_ms({"a_unfiltered_ms": batch(o_plain), "b_shared_10pct_ms": batch(o_shared),
                         "c_strided_1024x10pct_ms": batch(o_strided), "e_from_ids_1024x100k_ms": from_ids}, repeats)
    med_d, ts_d = median_ms({"d_single_query_calls_ms": singles}, max(3, repeats // 3))
    rec = dict(shape=shape, n=n, dim=dim, nq=nq, k=k, m=m, P=P or 1, repeats=repeats, strided_status=int(status),
               strided_rows_equal_singles=same, **med, **med_d,
               strided_over_shared=round(med["c_strided_1024x10pct_ms"] / med["b_shared_10pct_ms"], 3),
               singles_over_strided=round(med_d["d_single_query_calls_ms"] / med["c_strided_1024x10pct_ms"], 2),
               bitmap_block_mb=round(nq * words * 8 / 1e6, 1), id_lists_mb=round(nq * per * 4 / 1e6, 1),
               runs_ms={name: [round(t, 3) for t in v] for name, v in dict(ts, **ts_d).items()})
    print(json.dumps(rec), flush=True)
    lines.append(rec)
    ix.close()
    del d_ids, d_blk

if "--write" in sys.argv:
    with open(os.path.join(ROOT, "profiles", "query_filters_1m128_time.jsonl"), "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")

#!/usr/bin/env python3
"""Times the token map's bitmap kernel against scann_hip_allow_bitmaps_from_ids_device on the same rows, under the
conditions of DESIGN 3.3c-q's table: 1M rows, batch 1024, inputs resident on the device, wall time of the call plus a
stream synchronise, medians of `repeats` runs with the routes alternating in one loop.

  A  every query names ONE token whose posting is 100 k ids: the 1024 postings are the 1024 id lists of row (e) of
     tools/time_query_filters.py (the same generator, the same draws).  tokens: 1024 x 8 bytes; ids: 410 MB.
  B  every query names FOUR tokens of 25 k ids each, drawn from 64; the ids route gets the same rows as concatenated
     lists.
  C  the filtered tree search end to end (build the block, search, one stream, one synchronise) by both routes, on
     workload A's lists: 1M x 128, 1000 leaves, P = 10, m = 1000, k = 10.

The two routes' blocks are compared bitwise before anything is timed.  Next to each result stands the floor: the
block's bytes (128 MB) over the plain streaming-store rate of MI355X_MICROARCH.md (6.2 TB/s), and the time a device
fill of the same block takes in the same loop (a measured streaming store of the same bytes).

    python tools/time_token_filters.py [n] [nq] [repeats] [--write] [--skip-search]

One JSON line per workload, appended to profiles/token_filters_1m128_time.jsonl with --write.  SCANN_HIP_LIB selects
another build of the library (a tuning variant); its name is recorded."""
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
STORE_TBS = 6.2   # plain 16-byte streaming stores, MI355X_MICROARCH.md "Global float atomics" comparison row
if not torch.cuda.is_available():
    sys.exit("time_token_filters.py needs the GPU: a timing taken elsewhere says nothing")
L = hip.load()
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream()
sptr = ctypes.c_void_p(stream.cuda_stream)
p = lambda t: ctypes.c_void_p(t.data_ptr())
u64 = lambda t: ctypes.cast(p(t), ctypes.POINTER(ctypes.c_uint64))
words = -(-n // 64)
lib = os.path.basename(hip.LIB_PATH)
# the draws of tools/time_query_filters.py up to its row (e): the flat index's codebook rows and codes come first
rng = np.random.default_rng(3)
rng.choice(n, 16, replace=False)
rng.integers(0, 16, (n, S), dtype=np.uint8)


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
    """half the range of the runs around their median, in ms: what two medians may differ by from run to run"""
    return round((max(v) - min(v)) / 2, 4)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype.itemsize == 8 else np.int32).reshape(-1).copy()).to(dev)


def workload(name, lists_ids, token_of_posting, postings, token_lists):
    """lists_ids: [nq, per] ids of the ids route; postings: the token map's (token, ids) rows; token_lists: per query"""
    per = lists_ids.shape[1]
    d_ids = to_dev(lists_ids.astype(np.uint32))
    d_off = to_dev(np.arange(nq + 1, dtype=np.uint64) * np.uint64(per))
    idx = np.concatenate(postings).astype(np.uint32)
    tok = np.repeat(np.asarray(token_of_posting, np.uint64), [x.size for x in postings])
    t0 = time.perf_counter()
    tm = hip.TokenMap(n, idx, tok)
    create_s = time.perf_counter() - t0
    del idx, tok
    qt, qoff = hip._token_lists(token_lists)
    d_qt, d_qoff = to_dev(qt), to_dev(qoff)
    blk_ids = torch.empty((nq, words), dtype=torch.int64, device=dev)
    blk_tok = torch.full((nq, words), -1, dtype=torch.int64, device=dev)

    def from_ids():
        hip.allow_bitmaps_from_ids_device(d_ids.data_ptr(), d_off.data_ptr(), nq, n, words, blk_ids.data_ptr(), stream.cuda_stream)
        stream.synchronize()

    def from_tokens():
        tm.allow_bitmaps_device(d_qt.data_ptr(), d_qoff.data_ptr(), nq, words, blk_tok.data_ptr(), stream.cuda_stream)
        stream.synchronize()

    def fill():
        blk_ids.zero_()
        stream.synchronize()

    from_ids()
    from_tokens()
    equal = bool(torch.equal(blk_ids, blk_tok))
    if not equal:
        sys.exit("%s: the two routes' blocks differ: nothing is timed" % name)
    med, ts = median_ms({"from_ids_ms": from_ids, "from_tokens_ms": from_tokens, "fill_block_ms": fill}, repeats)
    block_mb = nq * words * 8 / 1e6
    floor_ms = block_mb / 1e6 / STORE_TBS * 1e3
    rec = dict(workload=name, lib=lib, n=n, nq=nq, repeats=repeats, tile_bits=hip.TOKEN_TILE_BITS, blocks_equal=equal,
               tokens_per_query=len(token_lists[0]), ids_per_query=per, map_tokens=tm.num_tokens(),
               map_create_s=round(create_s, 2), **med,
               from_ids_spread_ms=spread(ts["from_ids_ms"]), from_tokens_spread_ms=spread(ts["from_tokens_ms"]),
               ids_over_tokens=round(med["from_ids_ms"] / med["from_tokens_ms"], 2),
               bitmap_block_mb=round(block_mb, 1), id_lists_mb=round(nq * per * 4 / 1e6, 1),
               store_floor_ms=round(floor_ms, 4), store_floor_tb_s=STORE_TBS,
               fraction_of_store_floor=round(floor_ms / med["from_tokens_ms"], 3),
               fraction_of_measured_fill=round(med["fill_block_ms"] / med["from_tokens_ms"], 3),
               runs_ms={key: [round(t, 3) for t in v] for key, v in ts.items()})
    print(json.dumps(rec), flush=True)
    return rec, (tm, d_ids, d_off, d_qt, d_qoff, blk_ids, blk_tok)


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
# ---- A: one token of 100 k ids per query -----------------------------------------------------------------------
per = n // 10
ids_a = rng.integers(0, n, (nq, per), dtype=np.uint32)   # (row (e)'s lists: drawn with replacement, 9.5 % of the rows each)
rec_a, keep_a = workload("A_one_token_100k", ids_a, np.arange(nq) + 1, [np.unique(r) for r in ids_a],
                         [[i + 1] for i in range(nq)])
lines.append(rec_a)

# ---- B: four tokens of 25 k ids per query, drawn from 64 -------------------------------------------------------
rb = np.random.default_rng(4)
post_b = [np.unique(rb.integers(0, n, per // 4, dtype=np.uint32)) for _ in range(64)]
pad = lambda x: np.concatenate([x, np.full(per // 4 - x.size, x[0], np.uint32)])   # (a list repeats an id: same set)
pick = [rb.choice(64, 4, replace=False) for _ in range(nq)]
ids_b = np.stack([np.concatenate([pad(post_b[j]) for j in c]) for c in pick])
rec_b, keep_b = workload("B_four_tokens_25k_of_64", ids_b, np.arange(64) + 1, post_b, [[int(j) + 1 for j in c] for c in pick])
lines.append(rec_b)
del keep_b, ids_b

# ---- C: the filtered tree search end to end, workload A's lists ------------------------------------------------
if "--skip-search" not in sys.argv:
    tm, d_ids, d_off, d_qt, d_qoff, blk_ids, blk_tok = keep_a
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
    o_ids, o_tok, o_plain = opts(blk_ids), opts(blk_tok), opts(None)
    hip.check(L.scann_hip_index_reserve(ix.h, nq, k, ctypes.byref(o_plain)))

    def search(o, out):
        hip.check(L.scann_hip_search_batched_device(ix.h, p(qd), nq, dim, k, ctypes.byref(o), p(out[0]), p(out[1]), p(out[2]), sptr))

    def route_ids():
        hip.allow_bitmaps_from_ids_device(d_ids.data_ptr(), d_off.data_ptr(), nq, n, words, blk_ids.data_ptr(), stream.cuda_stream)
        search(o_ids, outs[0])
        stream.synchronize()

    def route_tokens():
        tm.allow_bitmaps_device(d_qt.data_ptr(), d_qoff.data_ptr(), nq, words, blk_tok.data_ptr(), stream.cuda_stream)
        search(o_tok, outs[1])
        stream.synchronize()

    def search_only():
        search(o_tok, outs[1])
        stream.synchronize()

    route_ids()
    s0 = L.scann_hip_index_last_device_status(ix.h, sptr)
    route_tokens()
    s1 = L.scann_hip_index_last_device_status(ix.h, sptr)
    same = bool(torch.equal(outs[0][2], outs[1][2]) and torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32)) and
                torch.equal(outs[0][0], outs[1][0]))
    if s0 != hip.OK or s1 != hip.OK or not same:
        sys.exit("C: statuses %d %d, rows equal: %s: nothing is timed" % (s0, s1, same))
    med, ts = median_ms({"ids_build_plus_search_ms": route_ids, "tokens_build_plus_search_ms": route_tokens,
                         "search_alone_ms": search_only}, repeats)
    rec = dict(workload="C_tree_search_end_to_end", lib=lib, n=n, dim=dim, nq=nq, k=k, m=m, P=P, repeats=repeats,
               rows_equal=same, **med, ids_spread_ms=spread(ts["ids_build_plus_search_ms"]),
               tokens_spread_ms=spread(ts["tokens_build_plus_search_ms"]),
               ids_over_tokens=round(med["ids_build_plus_search_ms"] / med["tokens_build_plus_search_ms"], 2),
               filter_share_tokens=round(1 - med["search_alone_ms"] / med["tokens_build_plus_search_ms"], 3),
               runs_ms={key: [round(t, 3) for t in v] for key, v in ts.items()})
    print(json.dumps(rec), flush=True)
    lines.append(rec)
    ix.close()

if "--write" in sys.argv:
    with open(os.path.join(ROOT, "profiles", "token_filters_1m128_time.jsonl"), "a") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")

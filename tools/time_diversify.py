#!/usr/bin/env python3
"""Times the MMR and the multi-attribute crowding stages: brute force over 1M x 128 f32 rows (DotProduct), batch 1024,
depth = 100, k = 10.  All device entry points on one stream, bracketed by device events, alternating in one loop
(medians):

  plain       scann_hip_search_batched_device at k = depth; its dominant kernel also by the handle's own kernel timing
  crowd       scann_hip_search_crowded_device, attributes idx mod 1000, limit 3
  crowd_md<d> scann_hip_search_crowded_md_device with d in {1, 2, 8} attribute dimensions (idx mod 1000, 997, ...)
  mmr         scann_hip_search_mmr_device, lambda 0.5

Cost of a stage = its call - plain.  One JSON line, also written to profiles/diversify_1m128_time.json with --write.
The stages' answers are compared with the CPU models for the first queries before anything is timed.

    python tools/time_diversify.py [n] [nq] [repeats] [--write]
"""
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import diversify_model as DM  # noqa: E402
from scann_rust_amd import hip, synth  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 1_000_000
nq = int(args[1]) if len(args) > 1 else 1024
repeats = int(args[2]) if len(args) > 2 else 21
dim, k, depth, lam = 128, 10, 100, 0.5
if not torch.cuda.is_available():
    sys.exit("time_diversify.py needs the GPU: a timing taken elsewhere says nothing")
L = hip.load()
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream()
st = stream.cuda_stream
p = lambda t: t.data_ptr()

x = synth.uniform_f32(n, dim, 42)
ix = hip.bf_create(x, n, dim, dim, hip.DOT_PRODUCT)
i = np.arange(n, dtype=np.uint64)
moduli = (1000, 997, 991, 983, 977, 971, 967, 953)
attrs = np.stack([i % np.uint64(m) for m in moduli])
ix.set_crowding_attributes(attrs[0])
q = synth.uniform_f32(nq, dim, 123)
qd = torch.from_numpy(q).to(dev)
oi = torch.empty((nq, k), dtype=torch.int32, device=dev)
od = torch.empty((nq, k), dtype=torch.float32, device=dev)
oc = torch.empty((nq,), dtype=torch.int32, device=dev)
pi = torch.empty((nq, depth), dtype=torch.int32, device=dev)
pd = torch.empty((nq, depth), dtype=torch.float32, device=dev)
pc = torch.empty((nq,), dtype=torch.int32, device=dev)
o = hip.default_opts()
o.bf_exact = 1     # the exact kernels everywhere: no query of a timed call is left unverified
ix.reserve_mmr(nq, k, depth, opts=o)
ix.enable_timing(True)


def plain():
    hip.check(L.scann_hip_search_batched_device(ix.h, ctypes.c_void_p(p(qd)), nq, dim, depth, ctypes.byref(o),
                                                ctypes.c_void_p(p(pi)), ctypes.c_void_p(p(pd)), ctypes.c_void_p(p(pc)),
                                                ctypes.c_void_p(st)))


def crowd():
    hip.check(L.scann_hip_search_crowded_device(ix.h, ctypes.c_void_p(p(qd)), nq, dim, k, depth, 3, ctypes.byref(o),
                                                ctypes.c_void_p(p(oi)), ctypes.c_void_p(p(od)), ctypes.c_void_p(p(oc)),
                                                ctypes.c_void_p(st)))


def crowd_md(nd):
    return lambda: ix.search_crowded_md_device(p(qd), nq, dim, k, depth, [3] * nd, p(oi), p(od), p(oc), st, opts=o)


def mmr():
    ix.search_mmr_device(p(qd), nq, dim, k, depth, lam, p(oi), p(od), p(oc), st, opts=o)


def result():
    stream.synchronize()
    assert L.scann_hip_index_last_device_status(ix.h, ctypes.c_void_p(st)) == hip.OK
    return oi.cpu().numpy().view(np.uint32), od.cpu().numpy(), oc.cpu().numpy().view(np.uint32)


# the answers agree with the models before anything is timed (the first 16 queries)
plain()
stream.synchronize()
hi, hd, hc = pi.cpu().numpy().view(np.uint32), pd.cpu().numpy(), pc.cpu().numpy()
mmr()
gi, gd, gc = result()
for j in range(16):
    wi, wd, _ = DM.mmr_apply_rows(hi[j, :hc[j]], hd[j, :hc[j]], k, lam, x, dim, dim, hip.DOT_PRODUCT)
    assert gc[j] == wi.size and np.array_equal(gi[j, :wi.size], wi) and np.array_equal(gd[j].view(np.uint32), wd.view(np.uint32))
for nd in (1, 2, 8):
    ix.set_crowding_attributes_md(attrs[:nd])
    crowd_md(nd)()
    gi, gd, gc = result()
    for j in range(16):
        wi, wd = DM.md_apply(hi[j, :hc[j]], hd[j, :hc[j]], attrs[:nd], [3] * nd, k)
        assert gc[j] == wi.size and np.array_equal(gi[j, :wi.size], wi)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


t = {}
kernel_ms = []
for nd in (1, 2, 8):     # (the attribute array is set outside the timed loop: it waits for the device)
    ix.set_crowding_attributes_md(attrs[:nd])
    routes = [("plain", plain), ("crowd", crowd), ("crowd_md%d" % nd, crowd_md(nd)), ("mmr", mmr)]
    for name, fn in routes:
        fn()
    stream.synchronize()
    for _ in range(repeats):   # alternating: a drift of the machine lands on all routes alike
        for name, fn in routes:
            t.setdefault(name, []).append(timed(fn))
            if name == "plain":
                kernel_ms.append(ix.last_kernel_ms())
med = {name: statistics.median(v) for name, v in t.items()}
line = {"n": n, "dim": dim, "nq": nq, "k": k, "depth": depth, "lambda": lam, "repeats": repeats,
        "measure": "DotProduct",
        "plain_ms": round(med["plain"], 4), "plain_kernel": kernel_ms[-1][1],
        "plain_kernel_ms": round(statistics.median(m for m, _ in kernel_ms), 4)}
for name in ("crowd", "crowd_md1", "crowd_md2", "crowd_md8", "mmr"):
    line[name + "_ms"] = round(med[name], 4)
    line[name + "_stage_ms"] = round(med[name] - med["plain"], 4)
    line[name + "_spread_ms"] = [round(min(t[name]), 4), round(max(t[name]), 4)]
line["plain_spread_ms"] = [round(min(t["plain"]), 4), round(max(t["plain"]), 4)]
print(json.dumps(line), flush=True)
if "--write" in sys.argv:
    with open(os.path.join(ROOT, "profiles", "diversify_1m128_time.json"), "w") as fh:
        fh.write(json.dumps(line) + "\n")

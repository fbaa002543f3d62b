#!/usr/bin/env python3
"""Times the crowding stage: brute force over 1M x 128 f32 rows (SquaredL2), batch 1024, k = 10, attributes
idx mod 1000, per_crowd_limit in {1, 3}, depth in {64, 512, 2048}.  Per point, alternating in one loop (medians):

  (a) the crowded device entry point (search at k = depth + crowding kernel, nothing leaves the device);
  (b) the route a caller had before: plain device search at k = depth, device-to-host copy of the [nq][depth]
      rows, the rule on one host thread (tests/crowding_model.apply_fast: the numpy form of CrowdingConstraint::apply,
      a sort per row -- the dict walk of apply() itself is ~30x slower in Python and would flatter the gain);
      the copy alone (plain search + device-to-host) is reported next to it;
  (c) the plain device search at k = depth alone.

Cost of the stage = (a) - (c); gain = (b) / (a).  One JSON line per point, also appended to
profiles/crowding_1m128_time.jsonl with --write.  The three answers are compared before anything is timed.

    python tools/time_crowding.py [n] [nq] [repeats] [--write]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import crowding_model as CM  # noqa: E402
from scann_rust_amd import hip, synth  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 1_000_000
nq = int(args[1]) if len(args) > 1 else 1024
repeats = int(args[2]) if len(args) > 2 else 15
dim, k = 128, 10
if not torch.cuda.is_available():
    sys.exit("time_crowding.py needs the GPU: a timing taken elsewhere says nothing")
L = hip.load()
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream()
sptr = ctypes.c_void_p(stream.cuda_stream)
p = lambda t: ctypes.c_void_p(t.data_ptr())

x = synth.uniform_f32(n, dim, 42)
ix = hip.bf_create(x, n, dim, dim, hip.SQUARED_L2)
attrs = (np.arange(n, dtype=np.uint64) % np.uint64(1000))
ix.set_crowding_attributes(attrs)
q = synth.uniform_f32(nq, dim, 123)
qd = torch.from_numpy(q).to(dev)
lines = []
for depth in (64, 512, 2048):
    oi = torch.empty((nq, k), dtype=torch.int32, device=dev)
    od = torch.empty((nq, k), dtype=torch.float32, device=dev)
    oc = torch.empty((nq,), dtype=torch.int32, device=dev)
    pi = torch.empty((nq, depth), dtype=torch.int32, device=dev)
    pd = torch.empty((nq, depth), dtype=torch.float32, device=dev)
    pc = torch.empty((nq,), dtype=torch.int32, device=dev)
    o = hip.default_opts()
    o.bf_exact = 1     # the exact kernels in (a), (b) and (c): no query of a timed call is left unverified
    hip.check(L.scann_hip_index_reserve_crowded(ix.h, nq, k, depth, ctypes.byref(o)))
    for limit in (1, 3):
        def crowded():
            hip.check(L.scann_hip_search_crowded_device(ix.h, p(qd), nq, dim, k, depth, limit, ctypes.byref(o), p(oi),
                                                        p(od), p(oc), sptr))
            stream.synchronize()

        def plain():
            hip.check(L.scann_hip_search_batched_device(ix.h, p(qd), nq, dim, depth, ctypes.byref(o), p(pi), p(pd),
                                                        p(pc), sptr))
            stream.synchronize()

        def host_route():
            plain()
            hi, hd, hc = pi.cpu().numpy().view(np.uint32), pd.cpu().numpy(), pc.cpu().numpy()
            return [CM.apply_fast(hi[i, :hc[i]], hd[i, :hc[i]], attrs, limit, k) for i in range(nq)]

        def copy_only():
            plain()
            return pi.cpu(), pd.cpu(), pc.cpu()

        # the three routes agree before anything is timed
        crowded()
        assert L.scann_hip_index_last_device_status(ix.h, sptr) == hip.OK
        gi, gd, gc = oi.cpu().numpy().view(np.uint32), od.cpu().numpy(), oc.cpu().numpy()
        for i, (wi, wd) in enumerate(host_route()):
            assert gc[i] == wi.size and np.array_equal(gi[i, :wi.size], wi)
            assert np.array_equal(gd[i, :wi.size].view(np.uint32), wd.view(np.uint32))
        t = {"a": [], "b": [], "c": [], "copy": []}
        for _ in range(repeats):   # alternating: a drift of the machine lands on all three alike
            for name, fn in (("a", crowded), ("b", host_route), ("c", plain), ("copy", copy_only)):
                t0 = time.perf_counter()
                fn()
                t[name].append((time.perf_counter() - t0) * 1e3)
        a, b, c = (statistics.median(t[x_]) for x_ in ("a", "b", "c"))
        line = {"n": n, "dim": dim, "nq": nq, "k": k, "depth": depth, "limit": limit, "repeats": repeats,
                "crowded_device_ms": round(a, 4), "plain_copy_hostwalk_ms": round(b, 4), "plain_ms": round(c, 4),
                "plain_copy_ms": round(statistics.median(t["copy"]), 4),
                "stage_ms": round(a - c, 4), "gain": round(b / a, 2),
                "spread_a_ms": [round(min(t["a"]), 4), round(max(t["a"]), 4)],
                "kept_mean": round(float(gc.mean()), 2)}
        lines.append(line)
        print(json.dumps(line), flush=True)
if "--write" in sys.argv:
    out = os.path.join(ROOT, "profiles", "crowding_1m128_time.jsonl")
    with open(out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")

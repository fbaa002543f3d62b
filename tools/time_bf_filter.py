#!/usr/bin/env python3
"""Times filtered brute force over n x 128 U[0,1) f32 rows (k = 10), one JSON line per case.

    python tools/time_bf_filter.py sweep [n] [steps]
        host entry, SquaredL2 and DotProduct, batches 1024 and 1, allowed fractions 0.1 % .. 100 %, each with the
        compacted id list (SCANN_HIP_BF_FILTER=1) and the bit test at the emit (=2), next to the unfiltered step
        (bf_exact = 1, the kernels a filtered call takes, and the default path).  step_ms = median wall time of a
        synchronous call, copies included.
    python tools/time_bf_filter.py unfiltered LABEL [n] [steps] [tree]
        unfiltered device-entry steps (batch 1024 exact and default path, batch 1), one line per case with the median,
        the quartiles and every step; package and library are those of `tree` (default: this tree).
    python tools/time_bf_filter.py compare OTHER_TREE [n] [steps] [rounds]
        `unfiltered` in child processes, this tree and OTHER_TREE (a built checkout of the parent commit) alternating
        `rounds` times; prints the children's lines and, per case, both medians over all rounds and the parent's own
        run-to-run spread (the range of its per-round medians).
"""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIM, K = 128, 10
FRACTIONS = (0.001, 0.01, 0.05, 0.10, 0.25, 0.50, 0.75, 1.0)


def _median_ms(fn, steps):
    fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), ts


def sweep(n, steps):
    from scann_rust_amd import hip, synth
    x = synth.uniform_f32(n, DIM, 42)
    rng = np.random.default_rng(7)
    u = rng.random(n)
    for mname, meas in (("sql2", hip.SQUARED_L2), ("dot", hip.DOT_PRODUCT)):
        ix = hip.bf_create(x, n, DIM, DIM, meas)
        ix.enable_timing(True)
        for nq in (1024, 1):
            os.environ["SCANN_HIP_SMALL"] = "0"
            q = synth.uniform_f32(nq, DIM, 123)
            o = hip.default_opts()
            o.bf_exact = 1
            base = {"measure": mname, "n": n, "dim": DIM, "nq": nq, "k": K}
            ms, _ = _median_ms(lambda: ix.search_batched(q, K, opts=o), steps)
            print(json.dumps(dict(base, filter="none", path="exact", step_ms=round(ms, 4), kernel=ix.last_kernel_ms()[1],
                                  kernel_ms=round(ix.last_kernel_ms()[0], 4))), flush=True)
            ms, _ = _median_ms(lambda: ix.search_batched(q, K), steps)
            print(json.dumps(dict(base, filter="none", path="default", step_ms=round(ms, 4),
                                  kernel=ix.last_kernel_ms()[1], kernel_ms=round(ix.last_kernel_ms()[0], 4))), flush=True)
            for f in FRACTIONS:
                ids = np.flatnonzero(u < f) if f < 1.0 else np.arange(n)
                words = hip.allow_bitmap(n, ids)
                for mech, val in (("compact", "1"), ("bittest", "2")):
                    os.environ["SCANN_HIP_BF_FILTER"] = val
                    ms, _ = _median_ms(lambda: ix.search_batched(q, K, allow=words, allow_bits=n), steps)
                    kms, kname = ix.last_kernel_ms()
                    print(json.dumps(dict(base, filter=f, allowed=int(ids.size), path=mech, step_ms=round(ms, 4),
                                          kernel=kname, kernel_ms=round(kms, 4))), flush=True)
                del os.environ["SCANN_HIP_BF_FILTER"]
            if nq == 1:   # the few-query host pipeline (SCANN_HIP_SMALL unset), where the handle takes it
                del os.environ["SCANN_HIP_SMALL"]
                for f in (None, 0.01, 0.5):
                    words = None if f is None else hip.allow_bitmap(n, np.flatnonzero(u < f))
                    ms, _ = _median_ms(lambda: ix.search_batched(q, K, allow=words, allow_bits=None if f is None else n), steps)
                    print(json.dumps(dict(base, filter=f or "none", path="small-default", step_ms=round(ms, 4))), flush=True)
        ix.close()


def unfiltered(label, n, steps, tree=None):
    if tree:
        sys.path.insert(0, tree)
    import torch
    from scann_rust_amd import hip, synth
    dev = torch.device("cuda", 0)
    L = hip.load()
    sptr = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    x = synth.uniform_f32(n, DIM, 42)
    for mname, meas in (("sql2", hip.SQUARED_L2), ("dot", hip.DOT_PRODUCT)):
        ix = hip.bf_create(x, n, DIM, DIM, meas)
        for nq, exact in ((1024, 1), (1024, 0), (1, 1)):
            qd = torch.from_numpy(synth.uniform_f32(nq, DIM, 123)).to(dev)
            oi = torch.empty((nq, K), dtype=torch.int32, device=dev)
            od = torch.empty((nq, K), dtype=torch.float32, device=dev)
            oc = torch.empty((nq,), dtype=torch.int32, device=dev)
            o = hip.default_opts()
            o.bf_exact = exact
            hip.check(L.scann_hip_index_reserve(ix.h, nq, K, ctypes.byref(o)))

            def run():
                hip.check(L.scann_hip_search_batched_device(ix.h, p(qd), nq, DIM, K, ctypes.byref(o), p(oi), p(od), p(oc), sptr))
                torch.cuda.synchronize()
            run()
            ms, ts = _median_ms(run, steps)
            print(json.dumps({"lib": label, "measure": mname, "n": n, "nq": nq, "path": "exact" if exact else "default",
                              "median_ms": round(ms, 4), "q25_ms": round(float(np.percentile(ts, 25)), 4),
                              "q75_ms": round(float(np.percentile(ts, 75)), 4), "steps_ms": [round(t, 4) for t in ts]}),
                  flush=True)
        ix.close()


def compare(other, n, steps, rounds):
    runs = {}
    for r in range(rounds):
        for label, tree in (("parent", other), ("this", ROOT)):
            env = dict(os.environ)
            env.pop("SCANN_HIP_LIB", None)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "unfiltered", label, str(n), str(steps), tree],
                                 env=env, capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise SystemExit("child %s failed (%d): %s" % (label, out.returncode, out.stderr[-2000:]))
            for line in out.stdout.splitlines():
                rec = json.loads(line)
                rec["round"] = r
                print(json.dumps(rec), flush=True)
                runs.setdefault((rec["measure"], rec["nq"], rec["path"]), {}).setdefault(label, []).append(rec)
    for (mname, nq, path), by in sorted(runs.items()):
        row = {"summary": True, "measure": mname, "nq": nq, "path": path}
        for label in ("parent", "this"):
            allsteps = [t for rec in by[label] for t in rec["steps_ms"]]
            meds = [rec["median_ms"] for rec in by[label]]
            row[label + "_median_ms"] = round(float(np.median(allsteps)), 4)
            row[label + "_batches"] = len(allsteps)
            row[label + "_round_medians_ms"] = meds
        row["parent_spread_ms"] = round(max(by["parent"][i]["median_ms"] for i in range(rounds)) -
                                        min(by["parent"][i]["median_ms"] for i in range(rounds)), 4)
        row["difference_ms"] = round(row["this_median_ms"] - row["parent_median_ms"], 4)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "sweep"
    if mode == "sweep":
        sweep(int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000, int(sys.argv[3]) if len(sys.argv) > 3 else 15)
    elif mode == "unfiltered":
        unfiltered(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000,
                   int(sys.argv[4]) if len(sys.argv) > 4 else 20, sys.argv[5] if len(sys.argv) > 5 else None)
    elif mode == "compare":
        compare(os.path.abspath(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000,
                int(sys.argv[4]) if len(sys.argv) > 4 else 20, int(sys.argv[5]) if len(sys.argv) > 5 else 3)
    else:
        raise SystemExit(__doc__)

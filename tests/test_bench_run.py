"""bench.py end to end at a small size: a plain run prints the result line with `ms_per_step` for exactly
`--steps` timed steps, measures nothing of `--full`, and `--dump-outputs` writes the rows of the last timed step,
which are the oracle's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_last_timed_step(tmp_path):
    from oracle import pyoracle as orc
    from scann_rust_amd import hip, synth

    n, dim, Q, k, steps = 20000, 64, 64, 10, 3
    out = tmp_path / "outputs"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        os.path.join(ROOT, "bench.py"), "--workload", "bf_dot", "--num-points", str(n), "--dim", str(dim),
        "--batch", str(Q), "--k", str(k), "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["value"] > 0
    assert (line["unit"], line["higher_is_better"], line["dtype"], line["full"]) == ("queries/s", True, "f32", False)
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["batch_sweep"] is None
    assert line["config"]["recall10@10"] is None and line["config"]["oracle_check"] is None

    idx, dist, cnt = (np.load(out / (name + ".npy")) for name in ("indices", "distances", "counts"))
    assert (idx.dtype, dist.dtype, cnt.dtype) == (np.float64, np.float32, np.float64)
    assert idx.shape == (Q, k) and dist.shape == (Q, k) and cnt.shape == (Q,)
    assert np.all(cnt == k)
    # the bench's inputs: the last timed step searched batch (steps - 1) % 4 of these queries
    rows = synth.uniform_f32(n, dim, 42)
    queries = synth.uniform_f32(max(Q * 4, 256), dim, 123)[((steps - 1) % 4) * Q:][:Q]
    stride = hip.compute_stride(dim)
    data = np.zeros((n, stride), np.float32)
    data[:, :dim] = rows
    for i in range(4):
        oi, od = orc.bf_search(data, n, dim, stride, orc.DOT_PRODUCT, queries[i], k)
        assert np.array_equal(dist[i].view(np.uint32), od.view(np.uint32)), (i, dist[i], od)
        assert sorted(idx[i].astype(np.int64).tolist()) == sorted(oi.tolist()), (i, idx[i], oi)

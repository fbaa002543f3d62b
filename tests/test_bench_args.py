"""bench.py's workload defaults (no GPU): N = 1 -> BASELINE configs[2] (AsymmetricHasher 1M x 128), N > 1 -> one
configs[4]-shaped Tree-X-Hybrid shard per GPU through the library's exchange, and the replica fallback the run
takes when the RCCL communicator cannot be created restores the N = 1 workload on every rank.  A plain run is the
default (`--full` adds the rest), and `--dump-outputs` writes the result rows as exact float arrays."""
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return _bench().parse()


def test_single_gpu_default_is_the_headline_config(monkeypatch):
    a = _parse(monkeypatch)
    assert (a.workload, a.sharded, a.n, a.dim, a.subspaces, a.pre_reorder_k, a.batch, a.k) == \
        ("ah", False, 1_000_000, 128, 32, 5000, 1024, 10)
    assert a.steps >= 100 and a.warmup >= 1


def test_multi_gpu_default_is_the_sharded_tree(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "8")
    assert (a.workload, a.sharded, a.n, a.dim, a.subspaces, a.leaves, a.partitions_to_search, a.pre_reorder_k) == \
        ("txh", True, 12_500_000, 96, 24, 1250, 10, 8192)
    r = _parse(monkeypatch, "--gpus", "8", "--multi-gpu", "replica")
    assert (r.workload, r.sharded, r.n, r.dim) == ("ah", False, 1_000_000, 128)


def test_replica_fallback_restores_the_single_gpu_workload(monkeypatch):
    mod = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--batch", "512"])
    a = mod.parse()
    assert a.sharded and a.workload == "txh"
    a.multi_gpu = "replica"            # what main() does when the communicator cannot be created
    mod.resolve_defaults(a)
    assert (a.workload, a.sharded, a.n, a.dim, a.subspaces, a.pre_reorder_k, a.batch) == \
        ("ah", False, 1_000_000, 128, 32, 5000, 512)
    # values given on the command line survive the fallback
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--workload", "txh", "--num-points", "2000000"])
    b = mod.parse()
    b.multi_gpu = "replica"
    mod.resolve_defaults(b)
    assert (b.workload, b.sharded, b.n) == ("txh", False, 2_000_000)


def test_plain_run_is_the_default_and_steps_are_checked(monkeypatch):
    a = _parse(monkeypatch)
    assert a.full is False and a.dump_outputs is None
    b = _parse(monkeypatch, "--full", "--dump-outputs", "out", "--steps", "7", "--warmup", "0")
    assert (b.full, b.dump_outputs, b.steps, b.warmup) == (True, "out", 7, 0)
    for argv in (("--steps", "0"), ("--warmup", "-1")):
        with pytest.raises(SystemExit):
            _parse(monkeypatch, *argv)


def test_dump_outputs_writes_exact_float_arrays(tmp_path):
    mod = _bench()
    idx = np.array([[3, 0xFFFFFFFF], [2**31 + 5, 7]], np.uint32).view(np.int32)
    dist = np.array([[0.5, np.inf], [1.25, 2.0]], np.float32)
    cnt = np.array([1, 2], np.int32)
    assert mod.dump_outputs(str(tmp_path), idx, dist, cnt) == ["counts", "distances", "indices"]
    i, d, c = (np.load(tmp_path / (name + ".npy")) for name in ("indices", "distances", "counts"))
    assert i.dtype == np.float64 and d.dtype == np.float32 and c.dtype == np.float64
    assert i.tolist() == [[3.0, 4294967295.0], [2147483653.0, 7.0]]
    assert np.array_equal(d.view(np.uint32), dist.view(np.uint32))
    assert c.tolist() == [1.0, 2.0]


def test_dump_outputs_samples_past_the_limit(tmp_path):
    mod = _bench()
    Q, k = 1000, 10
    idx = np.arange(Q * k, dtype=np.int32).reshape(Q, k)
    dist = idx.astype(np.float32)
    cnt = np.full(Q, k, np.int32)
    row_bytes = k * 8 + k * 4 + 8 + 8
    names = mod.dump_outputs(str(tmp_path / "a"), idx, dist, cnt, limit=100 * row_bytes)
    assert names == ["counts", "distances", "indices", "rows"]
    rows = np.load(tmp_path / "a" / "rows.npy")
    assert rows.dtype == np.float64 and rows.size == 100 and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "indices.npy"), idx[rows.astype(np.int64)].astype(np.float64))
    total = sum(os.path.getsize(tmp_path / "a" / (n + ".npy")) - 128 for n in names)
    assert total <= 100 * row_bytes
    mod.dump_outputs(str(tmp_path / "b"), idx, dist, cnt, limit=100 * row_bytes)    # the sample is fixed
    assert np.array_equal(np.load(tmp_path / "b" / "rows.npy"), rows)

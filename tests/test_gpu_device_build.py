"""scann_hip_txh_build: every array of the index it builds, bitwise against the rule of tests/device_build_model.py.

Each case builds with ONE call, reads the handle back with scann_hip_index_write_file and the numpy reader, and compares
centres, leaf offsets, leaf ids, codebook, packed codes and rows with the model.  The model's seeds are what
hip.kmeans_init_pp returns on the same rows and on the model's own training rows (tests/build_model.py and
tests/test_gpu_build.py pin those); everything after the seeds comes from the CPU oracle.  The report's iteration counts
and converged flags are the oracle's.  Every case runs with batched_codebook 0 and 1: one model, two builds."""
import functools
import os

import numpy as np
import pytest

from oracle import pyoracle as orc
from scann_rust_amd import hip, index_file
from tests import device_build_model as DM
from tests import helpers as H

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_f32(got, want, what):
    """bitwise equal, NaNs by position (a NaN's payload is not part of the contract)"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN positions differ" % what
    bad = np.flatnonzero((bits(got) != bits(want)).ravel() & ~nan.ravel())
    assert bad.size == 0, "%s: %d values differ, first at %d: %r vs %r" % (
        what, bad.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


@functools.lru_cache(maxsize=None)
def reference(name):
    """(rows, data, stride, cfg, model) of one case, computed once and shared by both flags; read-only"""
    rows, stride, cfg = DM.case(name)
    n, dim = rows.shape
    st = hip.compute_stride(dim) if stride is None else stride
    data = DM.strided(rows, st)
    dsub = dim // cfg["num_subspaces"]
    thr = cfg.get("simd_threshold", DM.SIMD_THRESHOLD)
    src = hip.bf_create(data, n, dim, st, hip.SQUARED_L2)

    def partition_seeds(k):
        return hip.kmeans_init_pp(src, k, seed=42, simd_threshold=thr)

    def subspace_seeds(train, s, kc):
        tix = subspace_seeds.index
        if tix is None:
            tix = subspace_seeds.index = hip.bf_create(DM.strided(train, st), n, dim, st, hip.SQUARED_L2)
        return hip.kmeans_init_pp(tix, kc, seed=42 + s, col_offset=s * dsub, sub_dim=dsub, simd_threshold=thr)

    subspace_seeds.index = None
    m = DM.model(rows, st, cfg, partition_seeds, subspace_seeds)
    if subspace_seeds.index is not None:
        subspace_seeds.index.close()
    src.close()
    for v in (rows, data) + tuple(a for a in m.values() if isinstance(a, np.ndarray)):
        v.setflags(write=False)
    return rows, data, st, cfg, m


def build_and_read(name, batched, tmp_path):
    rows, data, st, cfg, m = reference(name)
    n, dim = rows.shape
    src = hip.bf_create(data, n, dim, st, hip.SQUARED_L2)
    index, report = hip.txh_build(src, batched_codebook=batched, **cfg)
    path = os.path.join(str(tmp_path), "built.scannidx")
    hip.index_write_file(index, path)
    return src, index, report, index_file.arrays(path)


def check_against_model(name, report, f, m, cfg, data):
    S, K = cfg["num_subspaces"], cfg["num_codes"]
    assert (f["n_local"], f["dim"], f["stride"]) == (m["n"], m["dim"], m["stride"])
    assert (f["num_partitions"], f["num_subspaces"], f["num_codes"]) == (m["L"], S, K)
    assert f["codes_packed4"] == (1 if K <= 16 else 0)
    assert f["use_residuals"] == (1 if m["L"] and cfg.get("use_residuals", 1) else 0)
    if m["L"]:
        assert_same_f32(f["centers"], m["centers"], name + " centres")
        assert np.array_equal(f["leaf_offsets"], m["leaf_offsets"]), name + " leaf offsets"
        assert np.array_equal(f["leaf_ids"], m["leaf_ids"]), name + " leaf ids"
        assert report["partition_iterations"] == m["partition_iterations"], name
        assert report["partition_converged"] == m["partition_converged"], name
        gi, oi = np.float64(report["partition_inertia"]), np.float64(m["partition_inertia"])
        assert (np.isnan(gi) and np.isnan(oi)) or gi.view(np.uint64) == oi.view(np.uint64), (name, gi, oi)
    assert report["subspace_iterations"] == m["subspace_iterations"], \
        "%s: iterations %s vs %s" % (name, report["subspace_iterations"], m["subspace_iterations"])
    assert report["subspace_converged"] == m["subspace_converged"], name
    assert_same_f32(f["codebook"], m["codebook"], name + " codebook")
    bad = np.flatnonzero((np.asarray(f["codes"]) != m["codes_file"]).any(1))
    assert bad.size == 0, "%s: codes differ at %d CSR rows, first %d" % (name, bad.size, bad[0])
    if cfg.get("store_rows", 1):
        assert f["n_rows"] == m["n"] and np.array_equal(bits(f["data"]), bits(data)), name + " rows"
    else:
        assert "data" not in f


@pytest.mark.parametrize("batched", [0, 1], ids=["per-subspace", "batched"])
@pytest.mark.parametrize("name", DM.CASES)
def test_build_matches_the_model(name, batched, tmp_path):
    rows, data, st, cfg, m = reference(name)
    src, index, report, f = build_and_read(name, batched, tmp_path)
    try:
        check_against_model(name, report, f, m, cfg, data)
        assert set(report["stage_ms"]) == set(hip.BUILD_STAGES) and all(v >= 0.0 for v in report["stage_ms"].values())
        # `rows` is left untouched and still searches
        q = rows[:3] + np.float32(0.01)
        if not np.isnan(rows).any():
            idx, dist, cnt = src.search_batched(q, 5)[:3]
            for i in range(q.shape[0]):
                oi, od = orc.bf_search(data, rows.shape[0], rows.shape[1], st, hip.SQUARED_L2, q[i], 5)
                H.assert_topk_equal_up_to_ties(idx[i, :cnt[i]], dist[i, :cnt[i]], oi, od, what="source q%d" % i)
    finally:
        index.close()
        src.close()


@pytest.mark.parametrize("batched", [0, 1], ids=["per-subspace", "batched"])
def test_tree_searches_like_the_oracle_index(batched, tmp_path):
    """16 searches with stages on the built handle against orc.TxhIndex over the model's arrays, as
    test_build_chain_matches_oracle_step_by_step does for the chained route"""
    rows, data, st, cfg, m = reference("tree")
    n, dim, k = rows.shape[0], rows.shape[1], 10
    src, index, report, f = build_and_read("tree", batched, tmp_path)
    try:
        oix = orc.TxhIndex(data, st, dim, m["centers"], m["leaf_offsets"], m["leaf_ids"], m["codebook"], m["codes"],
                           partitions_to_search=3, pre_reorder_multiplier=4.0)
        q = rows[::n // 16][:16] + np.float32(0.01)
        o = hip.default_opts()
        o.partitions_to_search, o.pre_reorder_k = 3, orc.pre_reorder_k(k, 4.0)
        idx, dist, cnt, (tok, tokd, ci, cd, cc) = index.search_batched(q, k, o, stages=True)
        for i in range(q.shape[0]):
            H.check_txh_query(oix, q[i], k, idx[i, :cnt[i]], dist[i, :cnt[i]], tok[i], tokd[i], ci[i, :cc[i]],
                              cd[i, :cc[i]], what="q%d" % i)
    finally:
        index.close()
        src.close()


def test_flat_without_rows_refuses_exact_reordering(tmp_path):
    rows, data, st, cfg, m = reference("flat-no-rows")
    src, index, report, f = build_and_read("flat-no-rows", 1, tmp_path)
    try:
        q = rows[:4] + np.float32(0.01)
        o = hip.default_opts()
        o.exact_reorder = 0
        idx, dist, cnt = index.search_batched(q, 5, o)[:3]
        for i in range(4):      # the approximate search works: AsymmetricHasher::search over the model's codes
            oi, od = orc.ah_search(m["codebook"], m["codes"], q[i], 5)
            H.assert_topk_equal_up_to_ties(idx[i, :cnt[i]], dist[i, :cnt[i]], oi, od, what="ah q%d" % i)
        o = hip.default_opts()
        o.exact_reorder, o.pre_reorder_k = 1, 20
        with pytest.raises(hip.ScannError) as e:
            index.search_batched(q, 5, o)
        assert e.value.code == hip.FAILED_PRECONDITION, e.value
    finally:
        index.close()
        src.close()


def test_refusals_leave_the_rows_searchable():
    n, dim = 300, 16
    rows = np.random.default_rng(99).uniform(-1, 1, (n, dim)).astype(np.float32)
    st = hip.compute_stride(dim)
    data = DM.strided(rows, st)
    src = hip.bf_create(data, n, dim, st, hip.SQUARED_L2)
    ok = dict(num_partitions=4, num_subspaces=8, num_codes=16)

    def refused(index, code, **cfg):
        with pytest.raises(hip.ScannError) as e:
            hip.txh_build(index, **dict(ok, **cfg))
        assert e.value.code in (code if isinstance(code, tuple) else (code,)), e.value

    def still_searches():
        q = rows[:2] + np.float32(0.01)
        idx, dist, cnt = src.search_batched(q, 4)[:3]
        for i in range(2):
            oi, od = orc.bf_search(data, n, dim, st, hip.SQUARED_L2, q[i], 4)
            H.assert_topk_equal_up_to_ties(idx[i, :cnt[i]], dist[i, :cnt[i]], oi, od, what="source q%d" % i)

    for cfg, code in ((dict(num_subspaces=3), hip.INVALID_ARGUMENT),             # dim % S
                      (dict(num_subspaces=0), hip.INVALID_ARGUMENT),
                      (dict(num_subspaces=16, num_codes=300), hip.UNIMPLEMENTED),  # the shapes txh_create refuses
                      (dict(num_subspaces=16, num_codes=0), hip.UNIMPLEMENTED),
                      (dict(num_subspaces=2, num_codes=16), hip.UNIMPLEMENTED),
                      (dict(num_subspaces=2, num_codes=256), hip.UNIMPLEMENTED),
                      (dict(distance_measure=17), hip.UNIMPLEMENTED)):
        refused(src, code, **cfg)
        still_searches()
    # not an f32 brute-force handle: a tree handle, a quantized brute-force handle
    tree, _ = hip.txh_build(src, **ok)
    refused(tree, (hip.INVALID_ARGUMENT, hip.UNIMPLEMENTED))
    tree.close()
    bf16 = (bits(data) >> 16).astype(np.uint16)
    qix = hip.bf_create_quantized(bf16, n, dim, st, hip.ROWS_BF16, hip.SQUARED_L2)
    refused(qix, (hip.INVALID_ARGUMENT, hip.UNIMPLEMENTED))
    qix.close()
    still_searches()
    # n == 0
    empty = hip.bf_create(np.zeros((0, st), np.float32), 0, dim, st, hip.SQUARED_L2)
    refused(empty, hip.INVALID_ARGUMENT)
    empty.close()
    src.close()
    # dimensions past the k-means LDS limit: ResourceExhausted, as scann_hip_kmeans_lloyd returns it
    wide = np.random.default_rng(98).uniform(-1, 1, (16, 5128)).astype(np.float32)
    wst = hip.compute_stride(5128)
    wix = hip.bf_create(DM.strided(wide, wst), 16, 5128, wst, hip.SQUARED_L2)
    refused(wix, hip.RESOURCE_EXHAUSTED, num_partitions=2, num_subspaces=8)
    # (5128 dims are past the brute-force search's own LDS ceiling, so "still searches" cannot be asked of this handle;
    # it is intact: the same handle is refused the same way again, and a flat build whose subspaces fit goes through)
    assert wix.size() == 16 and wix.dimensionality() == 5128
    refused(wix, hip.RESOURCE_EXHAUSTED, num_partitions=2, num_subspaces=8)
    flat, rep = hip.txh_build(wix, num_partitions=0, num_subspaces=8, num_codes=16, training_iterations=2)
    assert flat.size() == 16 and all(1 <= i <= 2 for i in rep["subspace_iterations"])
    flat.close()
    wix.close()

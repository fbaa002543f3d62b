"""scann_hip_txh_build_hierarchical: every array of the index it builds, bitwise against the rule of
tests/hier_build_model.py.

Each case builds with ONE call, reads the handle back with scann_hip_index_write_file and the numpy reader, and compares
centres, leaf offsets, leaf ids, codebook, packed codes and rows with the model.  The model's seeds are what
hip.kmeans_init_pp returns on a brute-force handle of each node's rows (seed + depth) and on the model's own training
rows; everything after the seeds comes from the CPU oracle.  The tree report's per-level node counts, iteration sums and
converged counts are the model's."""
import functools
import os

import numpy as np
import pytest

from oracle import pyoracle as orc
from scann_rust_amd import hip, index_file
from tests import helpers as H
from tests import hier_build_model as HM

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
    """(rows, data, stride, tree, cfg, model) of one case, computed once; read-only"""
    rows, stride, tree, cfg = HM.case(name)
    n, dim = rows.shape
    st = hip.compute_stride(dim) if stride is None else stride
    data = HM.strided(rows, st)
    dsub = dim // cfg["num_subspaces"]
    thr = cfg.get("simd_threshold", HM.SIMD_THRESHOLD)

    def node_seeds(node_rows, k, depth):
        ix = hip.bf_create(HM.strided(node_rows, st), node_rows.shape[0], dim, st, hip.SQUARED_L2)
        try:
            return hip.kmeans_init_pp(ix, k, seed=tree["seed"] + depth, simd_threshold=thr)
        finally:
            ix.close()

    def subspace_seeds(train, s, kc):
        tix = subspace_seeds.index
        if tix is None:
            tix = subspace_seeds.index = hip.bf_create(HM.strided(train, st), n, dim, st, hip.SQUARED_L2)
        return hip.kmeans_init_pp(tix, kc, seed=42 + s, col_offset=s * dsub, sub_dim=dsub, simd_threshold=thr)

    subspace_seeds.index = None
    m = HM.model(rows, st, tree, cfg, node_seeds, subspace_seeds)
    if subspace_seeds.index is not None:
        subspace_seeds.index.close()
    for v in (rows, data) + tuple(a for a in m.values() if isinstance(a, np.ndarray)):
        v.setflags(write=False)
    return rows, data, st, tree, cfg, m


def build_and_read(name, tmp_path):
    rows, data, st, tree, cfg, m = reference(name)
    n, dim = rows.shape
    src = hip.bf_create(data, n, dim, st, hip.SQUARED_L2)
    # num_partitions and the kmeans_* fields of the build configuration are ignored: set them to nonsense
    index, report, trep = hip.txh_build_hierarchical(src, tree=tree, num_partitions=3, kmeans_iterations=1,
                                                     kmeans_seed=7, **cfg)
    path = os.path.join(str(tmp_path), "built.scannidx")
    hip.index_write_file(index, path)
    return src, index, report, trep, index_file.arrays(path)


def check_against_model(name, report, trep, f, m, cfg, data):
    S, K = cfg["num_subspaces"], cfg["num_codes"]
    tm = m["tree"]
    assert (f["n_local"], f["dim"], f["stride"]) == (m["n"], m["dim"], m["stride"])
    assert (f["num_partitions"], f["num_subspaces"], f["num_codes"]) == (m["L"], S, K), (name, f["num_partitions"], m["L"])
    assert f["codes_packed4"] == (1 if K <= 16 else 0)
    assert f["use_residuals"] == (1 if cfg.get("use_residuals", 1) else 0)
    assert np.array_equal(f["leaf_offsets"], m["leaf_offsets"]), name + " leaf offsets"
    assert np.array_equal(f["leaf_ids"], m["leaf_ids"]), name + " leaf ids"
    assert_same_f32(f["centers"], m["centers"], name + " centres")
    # the tree report
    assert trep["num_leaves"] == m["L"] and trep["depth_reached"] == max(tm["leaf_depth"]), (name, trep)
    for d, lv in enumerate(tm["levels"]):
        got = (trep["level_nodes"][d], trep["level_iterations"][d], trep["level_converged"][d], trep["level_leaves"][d])
        assert got == (lv["nodes"], lv["iterations"], lv["converged"], lv["leaves"]), (name, d, got, lv)
    assert all(a >= 0.0 and b >= 0.0 for a, b in trep["stage_ms"])
    if tm["trained"]:                       # the partitioner slots hold the root's k-means
        root = tm["trained"][0]
        assert report["partition_iterations"] == root["iterations"], name
        assert report["partition_converged"] == root["converged"], name
        gi, oi = np.float64(report["partition_inertia"]), np.float64(root["inertia"])
        assert (np.isnan(gi) and np.isnan(oi)) or gi.view(np.uint64) == oi.view(np.uint64), (name, gi, oi)
    else:
        assert report["partition_iterations"] == 0 and not report["partition_converged"]
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


def source_still_searches(src, rows, data, st):
    if np.isnan(rows).any():
        return
    q = rows[:3] + np.float32(0.01)
    idx, dist, cnt = src.search_batched(q, 5)[:3]
    for i in range(q.shape[0]):
        oi, od = orc.bf_search(data, rows.shape[0], rows.shape[1], st, hip.SQUARED_L2, q[i], 5)
        H.assert_topk_equal_up_to_ties(idx[i, :cnt[i]], dist[i, :cnt[i]], oi, od, what="source q%d" % i)


@pytest.mark.parametrize("name", HM.CASES)
def test_build_matches_the_model(name, tmp_path):
    rows, data, st, tree, cfg, m = reference(name)
    # with the library's own seeds the case still is what it is named for
    assert HM.condition(name, rows, tree, m["tree"]) is None
    src, index, report, trep, f = build_and_read(name, tmp_path)
    try:
        check_against_model(name, report, trep, f, m, cfg, data)
        assert set(report["stage_ms"]) == set(hip.BUILD_STAGES) and all(v >= 0.0 for v in report["stage_ms"].values())
        source_still_searches(src, rows, data, st)
    finally:
        index.close()
        src.close()


def test_depth_2_searches_like_the_oracle_index(tmp_path):
    """16 searches with stages on the built handle against orc.TxhIndex over the model's arrays"""
    rows, data, st, tree, cfg, m = reference("depth-2")
    n, dim, k = rows.shape[0], rows.shape[1], 10
    src, index, report, trep, f = build_and_read("depth-2", tmp_path)
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


def test_depth_1_against_the_flat_build(tmp_path):
    """max_depth 1 is the flat partitioner's k-means (num_partitions = num_children, the same seed) with every leaf's
    centre recomputed as the ordered mean of the FINAL assignment: the assignments and the CSR are the flat build's;
    the centres are the flat build's exactly when its loop's last update already was the mean of its final assignment,
    i.e. when the loop stopped on convergence with an unchanged assignment -- judged from the oracle, asserted either way."""
    rows, data, st, tree, cfg, m = reference("depth-1")
    n, dim = rows.shape
    src, index, report, trep, f = build_and_read("depth-1", tmp_path)
    flat, frep = hip.txh_build(src, num_partitions=tree["num_children"], kmeans_iterations=tree["kmeans_iterations"],
                               kmeans_convergence=tree["kmeans_convergence"], kmeans_seed=tree["seed"], **cfg)
    try:
        path = os.path.join(str(tmp_path), "flat.scannidx")
        hip.index_write_file(flat, path)
        g = index_file.arrays(path)
        assert np.array_equal(f["leaf_offsets"], g["leaf_offsets"]) and np.array_equal(f["leaf_ids"], g["leaf_ids"])
        assert report["partition_iterations"] == frep["partition_iterations"]
        assert report["partition_converged"] == frep["partition_converged"]
        # the oracle's loop from the same seeds: are its last centres the ordered means of its final assignment?
        c0 = m["tree"]["trained"][0]["seeds"]
        oc, oa, *_ = orc.kmeans_lloyd(data, n, st, dim, c0, max_iterations=tree["kmeans_iterations"],
                                      convergence_threshold=tree["kmeans_convergence"])
        means = np.stack([HM.ordered_mean(rows, np.flatnonzero(np.asarray(oa) == c)) for c in range(oc.shape[0])])
        same = np.array_equal(bits(oc), bits(means))
        assert np.array_equal(bits(f["centers"]), bits(g["centers"])) == same
        # which one holds for this case: EQUAL.  The loop converges on these six well separated clusters with an
        # assignment that no longer changes, so its last update already was the ordered mean of its final assignment.
        assert same
    finally:
        flat.close()
        index.close()
        src.close()


def test_refusals_leave_the_rows_searchable():
    n, dim = 300, 16
    rows = np.random.default_rng(199).uniform(-1, 1, (n, dim)).astype(np.float32)
    st = hip.compute_stride(dim)
    data = HM.strided(rows, st)
    src = hip.bf_create(data, n, dim, st, hip.SQUARED_L2)
    ok_tree = dict(num_children=4, max_depth=2, kmeans_iterations=3)
    ok = dict(num_subspaces=8, num_codes=16, training_iterations=2)

    def refused(index, code, tree=ok_tree, **cfg):
        with pytest.raises(hip.ScannError) as e:
            hip.txh_build_hierarchical(index, tree=tree, **dict(ok, **cfg))
        assert e.value.code in (code if isinstance(code, tuple) else (code,)), e.value
        return e.value

    def still_searches():
        q = rows[:2] + np.float32(0.01)
        idx, dist, cnt = src.search_batched(q, 4)[:3]
        for i in range(2):
            oi, od = orc.bf_search(data, n, dim, st, hip.SQUARED_L2, q[i], 4)
            H.assert_topk_equal_up_to_ties(idx[i, :cnt[i]], dist[i, :cnt[i]], oi, od, what="source q%d" % i)

    refused(src, hip.INVALID_ARGUMENT, tree=dict(ok_tree, num_children=0))
    still_searches()
    refused(src, hip.UNIMPLEMENTED, tree=dict(ok_tree, max_depth=5))
    still_searches()
    # what scann_hip_txh_build refuses, with its status
    for cfg, code in ((dict(num_subspaces=3), hip.INVALID_ARGUMENT), (dict(num_subspaces=16, num_codes=300), hip.UNIMPLEMENTED),
                      (dict(distance_measure=17), hip.UNIMPLEMENTED)):
        refused(src, code, **cfg)
        still_searches()
    # a quantized source
    bf16 = (bits(data) >> 16).astype(np.uint16)
    qix = hip.bf_create_quantized(bf16, n, dim, st, hip.ROWS_BF16, hip.SQUARED_L2)
    refused(qix, hip.INVALID_ARGUMENT)
    qix.close()
    still_searches()
    # a good configuration goes through on the same handle afterwards
    index, _, trep = hip.txh_build_hierarchical(src, tree=ok_tree, **ok)
    assert index.size() == n and 2 <= trep["num_leaves"] <= 16
    index.close()
    src.close()


def test_too_many_leaves_is_refused_after_the_tree_stage():
    """40 000 uniform points of the plane (in 8 columns, HM.too_many_leaves_case), 130 children, depth 2: more than 16384 leaves (tests/test_hier_build_model.py shows it
    from the model alone); no handle, the count in the message, the source still searches"""
    rows, tree = HM.too_many_leaves_case()
    n, dim = rows.shape
    st = hip.compute_stride(dim)
    data = HM.strided(rows, st)
    src = hip.bf_create(data, n, dim, st, hip.SQUARED_L2)
    try:
        with pytest.raises(hip.ScannError) as e:
            hip.txh_build_hierarchical(src, tree=tree, num_subspaces=8, num_codes=16, training_iterations=1)
        assert e.value.code == hip.UNIMPLEMENTED, e.value
        count = [int(w) for w in e.value.message.replace(",", " ").split() if w.isdigit()]
        assert count and max(count) > HM.MAX_LEAVES and "16384" in e.value.message, e.value.message
        q = rows[:2] + np.float32(0.01)
        idx, dist, cnt = src.search_batched(q, 4)[:3]
        for i in range(2):
            oi, od = orc.bf_search(data, n, dim, st, hip.SQUARED_L2, q[i], 4)
            H.assert_topk_equal_up_to_ties(idx[i, :cnt[i]], dist[i, :cnt[i]], oi, od, what="source q%d" % i)
    finally:
        src.close()

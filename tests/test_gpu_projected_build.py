"""scann_hip_txh_build_projected against its rule (include/scann_hip.h "projected device build"): the one-call handle
equals, section by section of its written index file and bit by bit in its searches, the chained route through the
public entry points -- scann_hip_project_device, scann_hip_bf_create, scann_hip_txh_build(store_rows = 0),
scann_hip_txh_create_projected.  (tests/test_gpu_device_build.py pins scann_hip_txh_build against the CPU model and
tests/test_gpu_projected_search.py pins projected handles against the oracle; this file pins the composition.)"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import pyoracle as orc
from scann_rust_amd import hip, index_file, trainer
from tests import helpers as H
from tests import pca_model as PM

pytestmark = pytest.mark.gpu

N, IN_DIM, OUT_DIM, STRIDE = 3000, 96, 32, 100
K = 10

SHAPES = {
    "tree-S8-K16": dict(num_partitions=12, num_subspaces=8, num_codes=16),
    "flat-S16-K16": dict(num_partitions=0, num_subspaces=16, num_codes=16),
    "tree-S4-K256": dict(num_partitions=12, num_subspaces=4, num_codes=256),
}
COMMON = dict(kmeans_iterations=4, training_iterations=4, partitions_to_search=3, pre_reorder_multiplier=4.0)


@functools.lru_cache(maxsize=None)
def rows():
    X = PM.rows(N, IN_DIM, 24, 11, offset=0.5)
    data = PM.strided(X, STRIDE, fill=0.0)
    q = (X[::N // 16][:16] + np.float32(0.01)).copy()
    for a in (X, data, q):
        a.setflags(write=False)
    return X, data, q


def projection(kind, src):
    if kind == "pca":
        return hip.pca_train(src, OUT_DIM)[0]
    if kind == "matrix":
        return hip.Projection(hip.PROJ_MATRIX, matrix=trainer.random_orthogonal(IN_DIM, OUT_DIM, 5))
    return hip.Projection(hip.PROJ_TRUNCATE, in_dim=IN_DIM, out_dim=OUT_DIM, start=17)


def chained(proj, data, cfg, store_rows, tmp_path):
    """the rule's four steps"""
    d_rows = torch.from_numpy(np.array(data)).to("cuda:0")
    d_out = torch.empty((N, OUT_DIM), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    proj.project_device(d_rows.data_ptr(), N, STRIDE, d_out.data_ptr(), OUT_DIM)
    torch.cuda.synchronize()
    projected = d_out.cpu().numpy()
    bfp = hip.bf_create(projected, N, OUT_DIM, OUT_DIM, hip.SQUARED_L2)
    built, report = hip.txh_build(bfp, store_rows=0, **cfg)
    bfp.close()
    path = os.path.join(str(tmp_path), "chain-built.scannidx")
    hip.index_write_file(built, path)
    built.close()
    f = index_file.arrays(path)
    tree = f["num_partitions"] != 0
    index = hip.txh_create_projected(
        projection=proj, rows=data if store_rows else None, n_rows=N, row_dim=IN_DIM, row_stride=STRIDE, dim=OUT_DIM,
        centers=f["centers"] if tree else None, leaf_offsets=f["leaf_offsets"] if tree else None,
        leaf_ids=f["leaf_ids"] if tree else None, codebook=f["codebook"], codes=f["codes"],
        codes_packed4=bool(f["codes_packed4"]), use_residuals=bool(f["use_residuals"]),
        partitions_to_search=f["partitions_to_search"], pre_reorder_multiplier=f["pre_reorder_multiplier"],
        distance_measure=f["distance_measure"])
    return index, report


def assert_same_file(path_a, path_b):
    ha, sa = index_file.read(path_a)
    hb, sb = index_file.read(path_b)
    assert ha == hb, (ha, hb)
    assert set(sa) == set(sb), (sorted(sa), sorted(sb))
    for name in sa:
        a, b = np.asarray(sa[name]), np.asarray(sb[name])
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert a.tobytes() == b.tobytes(), "section %s differs" % name
    return sa


def search(index, q, exact):
    o = hip.default_opts()
    o.exact_reorder = 1 if exact else 0
    idx, dist, cnt = index.search_batched(q, K, o)[:3]
    return idx, dist, cnt


def assert_same_search(a, b, q, exact):
    ia, da, ca = search(a, q, exact)
    ib, db, cb = search(b, q, exact)
    assert np.array_equal(ca, cb)
    for i in range(q.shape[0]):
        assert np.array_equal(ia[i, :ca[i]], ib[i, :cb[i]]), "q%d idx" % i
        assert np.array_equal(da[i, :ca[i]].view(np.uint32), db[i, :cb[i]].view(np.uint32)), "q%d dist" % i
    return ia, da, ca


CASES = [("tree-S8-K16", "pca", 1), ("tree-S8-K16", "matrix", 1), ("tree-S8-K16", "truncate", 1),
         ("tree-S8-K16", "pca", 0), ("flat-S16-K16", "pca", 1), ("flat-S16-K16", "matrix", 0),
         ("tree-S4-K256", "pca", 1), ("tree-S4-K256", "truncate", 0)]


@pytest.mark.parametrize("shape,kind,store_rows", CASES, ids=["%s-%s-rows%d" % c for c in CASES])
def test_one_call_equals_the_chained_route(shape, kind, store_rows, tmp_path):
    X, data, q = rows()
    cfg = dict(SHAPES[shape], **COMMON)
    src = hip.bf_create(data, N, IN_DIM, STRIDE, hip.SQUARED_L2)
    proj = projection(kind, src)
    one = two = loaded = None
    try:
        one, report = hip.txh_build_projected(src, proj, store_rows=store_rows, **cfg)
        two, report2 = chained(proj, data, cfg, store_rows, tmp_path)
        assert one.size() == N and one.dimensionality() == IN_DIM
        assert one.projection_info() == proj.info() == two.projection_info()
        assert set(report["stage_ms"]) == set(hip.BUILD_STAGES) and all(v >= 0.0 for v in report["stage_ms"].values())
        for key in ("partition_iterations", "partition_converged", "subspace_iterations", "subspace_converged"):
            assert report[key] == report2[key], key
        pa, pb = os.path.join(str(tmp_path), "one.scannidx"), os.path.join(str(tmp_path), "two.scannidx")
        hip.index_write_file(one, pa)
        hip.index_write_file(two, pb)
        sections = assert_same_file(pa, pb)
        assert "proj_meta" in sections and ("data" in sections) == bool(store_rows)
        assert ("proj_matrix" in sections) == (kind != "truncate") and ("proj_mean" in sections) == (kind == "pca")
        if store_rows:
            assert np.asarray(sections["data"]).tobytes() == data.tobytes()
        ia, da, ca = assert_same_search(one, two, q, exact=bool(store_rows))
        assert np.all(ca == K)
        # the written file reloads and searches the same
        loaded = hip.load_file(pa)
        assert_same_search(one, loaded, q, exact=bool(store_rows))
        if not store_rows:      # no rows: exact re-ordering is a FailedPrecondition, as on every handle without rows
            with pytest.raises(hip.ScannError) as e:
                search(one, q, exact=True)
            assert e.value.code == hip.FAILED_PRECONDITION, e.value
        # `rows` is left untouched and still searches
        idx, dist, cnt = src.search_batched(q[:2], 4)[:3]
        for i in range(2):
            oi, od = orc.bf_search(data, N, IN_DIM, STRIDE, hip.SQUARED_L2, q[i], 4)
            H.assert_topk_equal_up_to_ties(idx[i, :cnt[i]], dist[i, :cnt[i]], oi, od, what="source q%d" % i)
    finally:
        for h in (one, two, loaded, proj, src):
            if h is not None:
                h.close()


def test_refusals():
    X, data, q = rows()
    src = hip.bf_create(data, N, IN_DIM, STRIDE, hip.SQUARED_L2)
    proj = projection("matrix", src)
    ok = dict(num_partitions=4, num_subspaces=8, num_codes=16, kmeans_iterations=2, training_iterations=2)

    def refused(index, p, code, **cfg):
        with pytest.raises(hip.ScannError) as e:
            hip.txh_build_projected(index, p, **dict(ok, **cfg))
        assert e.value.code in (code if isinstance(code, tuple) else (code,)), e.value

    # everything scann_hip_txh_build refuses, judged on out_dim = 32
    for cfg, code in ((dict(num_subspaces=3), hip.INVALID_ARGUMENT),              # 32 % 3 (96 % 3 == 0: judged on out_dim)
                      (dict(num_subspaces=0), hip.INVALID_ARGUMENT),
                      (dict(num_subspaces=48), hip.INVALID_ARGUMENT),             # 96 % 48 == 0, 32 % 48 != 0
                      (dict(num_subspaces=16, num_codes=300), hip.UNIMPLEMENTED),
                      (dict(num_subspaces=16, num_codes=0), hip.UNIMPLEMENTED),
                      (dict(num_subspaces=2, num_codes=16), hip.UNIMPLEMENTED),
                      (dict(num_subspaces=2, num_codes=256), hip.UNIMPLEMENTED),
                      (dict(distance_measure=17), hip.UNIMPLEMENTED)):
        refused(src, proj, code, **cfg)
    # what scann_hip_txh_create_projected refuses: no projection, rows of another width
    refused(src, None, hip.INVALID_ARGUMENT)
    other = hip.Projection(hip.PROJ_MATRIX, matrix=trainer.random_orthogonal(64, 32, 5))
    refused(src, other, hip.INVALID_ARGUMENT)
    other.close()
    # not an f32 brute-force handle; no rows
    tree, _ = hip.txh_build(src, num_partitions=4, num_subspaces=8, num_codes=16, kmeans_iterations=2, training_iterations=2)
    refused(tree, proj, (hip.INVALID_ARGUMENT, hip.UNIMPLEMENTED))
    tree.close()
    bf16 = (np.ascontiguousarray(data).view(np.uint32) >> 16).astype(np.uint16)
    qix = hip.bf_create_quantized(bf16, N, IN_DIM, STRIDE, hip.ROWS_BF16, hip.SQUARED_L2)
    refused(qix, proj, (hip.INVALID_ARGUMENT, hip.UNIMPLEMENTED))
    qix.close()
    empty = hip.bf_create(np.zeros((0, STRIDE), np.float32), 0, IN_DIM, STRIDE, hip.SQUARED_L2)
    refused(empty, proj, hip.INVALID_ARGUMENT)
    empty.close()
    # the source still searches, and still builds
    idx, dist, cnt = src.search_batched(q[:2], 4)[:3]
    for i in range(2):
        oi, od = orc.bf_search(data, N, IN_DIM, STRIDE, hip.SQUARED_L2, q[i], 4)
        H.assert_topk_equal_up_to_ties(idx[i, :cnt[i]], dist[i, :cnt[i]], oi, od, what="source q%d" % i)
    index, _ = hip.txh_build_projected(src, proj, **ok)
    assert index.size() == N
    index.close()
    proj.close()
    src.close()

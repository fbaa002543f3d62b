"""One integer-MFMA prefilter search per creation route.

hip.txh_build, txh_build_projected, txh_create_projected, txh_create_quantized and write_file -> load_file all end in
txh_finish, which builds the operand planes (codes_sp) -- and their own tests search at sizes where the planes are never
read.  Here each route's handle answers one 65-query search under a forced prefilter, at the shapes of
tests/test_gpu_sp_bitmap.py and no more (the build rules themselves are pinned by the routes' own test files):
  flat  4133 rows, sp-lanes + SP_PAIRS=64: the bitmap form (adc_smfmac_bits_kernel64 + adc_refine_bits_kernel)
  tree  20000 rows, sp-words
m = 250, k = 10.  The reference is the one the route's own test file uses: the oracle over the arrays the handle holds
(read back through scann_hip_index_write_file; those arrays are NOT the planes the prefilter reads) for the builds and
the file round trip, tests/quantized_rerank_model.py for quantized rows, the oracle in the projected space with the
re-rank in the rows' own space for projected handles.  Every search asserts its kernel, and the flat ones the survivor
bitmaps in the workspace."""
import os

import numpy as np
import pytest

import helpers as H
import projection_model as pm
import quantized_rerank_cases as QC
from oracle import pyoracle as orc
from scann_rust_amd import hip, index_file, synth, trainer
from test_gpu_quantized_rerank import _assert_candidates, _assert_rows, _create
from test_gpu_sp_bitmap import _bitmap_bytes, _knob

pytestmark = pytest.mark.gpu

K, M, NQ = 10, 250, 65
NAME = "adc_smfmac_kernel"
FLAT_N, TREE_N, TREE_L, TREE_P = 4133, 20000, 16, 6
FORMS = {"flat": dict(value=None), "tree": dict(value=None, pairs=None, scan="sp-words")}


def _opts(kind):
    o = hip.default_opts()
    o.pre_reorder_k = M
    if kind == "tree":
        o.partitions_to_search = TREE_P
    return o


def _scan_ran(index, kind, n):
    assert index.last_kernel_ms()[1] == NAME, index.last_kernel_ms()[1]
    assert index.debug_survivor_bitmap_bytes() == (_bitmap_bytes(n, NQ) if kind == "flat" else 0)


def _file_arrays(index, tmp_path, name):
    path = os.path.join(str(tmp_path), name)
    hip.index_write_file(index, path)
    return index_file.arrays(path), path


def _codes(f):
    codes = np.ascontiguousarray(f["codes"])
    return orc.unpack4(codes, f["num_subspaces"]) if f["codes_packed4"] else codes


def check_from_arrays(index, kind, f, q, what, oix=None, q_scan=None, rerank=None):
    """a staged search of `index` under the forced prefilter, every query against the oracle over the arrays `f` of the
    handle's own file (a tree: through `oix`, the oracle index over them).  q_scan: the queries as the scan sees them
    (projected handles), rerank(i, candidates) -> the expected final rows in the rows' own space (projected handles: the
    stages are then checked here)"""
    index.enable_timing(True)
    idx, dist, cnt, (tok, tokd, ci, cd, cc) = index.search_batched(q, K, _opts(kind), stages=True)
    _scan_ran(index, kind, f["n_rows"])
    cb, codes = f["codebook"], _codes(f)
    for i in range(q.shape[0]):
        w = "%s q%d" % (what, i)
        got = (idx[i, :cnt[i]], dist[i, :cnt[i]])
        gci, gcd = ci[i, :cc[i]], cd[i, :cc[i]]
        if rerank is not None:     # (flat only) tests/test_gpu_projected_search.py Case.check_query
            oci, ocd = orc.ah_search(cb, codes, q_scan[i], M)
            assert gci.size == oci.size, w
            assert np.array_equal(gcd.view(np.uint32), ocd.view(np.uint32)), w + " approximate distances"
            H.assert_topk_equal_up_to_ties(gci, gcd, oci, ocd, what=w + " cand")
            oi, od = rerank(i, oci if sorted(gci.tolist()) == sorted(oci.tolist()) else gci)
            assert got[0].size == oi.size, w
            H.assert_topk_equal_up_to_ties(got[0], got[1], oi, od, what=w + " final")
        elif kind == "flat":
            H.check_ah_query(cb, codes, np.ascontiguousarray(f["data"]).ravel(), f["stride"], f["dim"], q[i], K, M,
                             got[0], got[1], gci, gcd, what=w)
        else:
            H.check_txh_query(oix, q[i], K, got[0], got[1], tok[i], tokd[i], gci, gcd, what=w)
    fast = index.search_batched(q, K, _opts(kind))
    _scan_ran(index, kind, f["n_rows"])
    assert np.array_equal(fast[2], cnt) and np.array_equal(fast[1].view(np.uint32), dist.view(np.uint32)), what + " fast"


def _tree_oracle(f):
    return orc.TxhIndex(np.ascontiguousarray(f["data"]).ravel(), f["stride"], f["dim"], f["centers"], f["leaf_offsets"],
                        f["leaf_ids"], f["codebook"], _codes(f), use_residuals=bool(f["use_residuals"]),
                        partitions_to_search=TREE_P, pre_reorder_multiplier=float(M) / K)


def _source(kind, dim=32):
    """(rows, queries) of the f32 brute-force handle a build starts from"""
    if kind == "flat":
        rows = synth.uniform_f32(FLAT_N, dim, 3100)
        q = synth.uniform_f32(NQ, dim, 3101)
    else:
        rows = synth.clustered_f32(TREE_N, dim, 3102, n_clusters=TREE_L)[0]
        q = synth.clustered_f32(NQ, dim, 3103, n_clusters=TREE_L)[0]
    return rows, q


# ---- hip.txh_build, and the written file loaded again -----------------------------------------------------------------
@pytest.mark.parametrize("kind", ["flat", "tree"])
def test_txh_build_and_file_round_trip(kind, tmp_path, monkeypatch):
    _knob(monkeypatch, **FORMS[kind])
    rows, q = _source(kind)
    n, dim = rows.shape
    data, stride = orc.to_strided(rows)
    src = hip.bf_create(data, n, dim, stride, hip.SQUARED_L2)
    cfg = dict(num_partitions=0 if kind == "flat" else TREE_L, num_subspaces=16, num_codes=16, kmeans_iterations=3,
               training_iterations=3, partitions_to_search=TREE_P if kind == "tree" else 1,
               pre_reorder_multiplier=float(M) / K)
    index, _ = hip.txh_build(src, **cfg)
    f, path = _file_arrays(index, tmp_path, "built.scannidx")
    assert f["n_rows"] == n and f["num_partitions"] == (0 if kind == "flat" else TREE_L)
    oix = _tree_oracle(f) if kind == "tree" else None
    check_from_arrays(index, kind, f, q, "txh_build " + kind, oix=oix)
    loaded = hip.load_file(path)
    check_from_arrays(loaded, kind, f, q, "load_file " + kind, oix=oix)
    for h in (loaded, index, src):
        h.close()


# ---- projected handles: flat, 96 -> 32 ------------------------------------------------------------------------------------
def _projected_inputs():
    rows = synth.uniform_f32(FLAT_N, 96, 3110)
    q = synth.uniform_f32(NQ, 96, 3111)
    mat = trainer.random_orthogonal(96, 32, 5)
    return rows, q, mat


def _check_projected(index, f, rows, q, mat, what):
    assert index.projection_info()[:3] == (pm.MATRIX, 96, 32)
    q_p = pm.project(pm.MATRIX, q, mat, None, out_dim=32)
    data, stride = orc.to_strided(rows)
    rerank = lambda i, cand: orc.reorder_measure(data, stride, 96, hip.SQUARED_L2, q[i], cand, K)
    check_from_arrays(index, "flat", f, q, what, q_scan=q_p, rerank=rerank)


def test_txh_build_projected(tmp_path, monkeypatch):
    _knob(monkeypatch, **FORMS["flat"])
    rows, q, mat = _projected_inputs()
    data, stride = orc.to_strided(rows)
    src = hip.bf_create(data, FLAT_N, 96, stride, hip.SQUARED_L2)
    proj = hip.Projection(hip.PROJ_MATRIX, matrix=mat)
    index, _ = hip.txh_build_projected(src, proj, num_partitions=0, num_subspaces=16, num_codes=16, training_iterations=3,
                                       pre_reorder_multiplier=float(M) / K)
    f, _ = _file_arrays(index, tmp_path, "built-projected.scannidx")
    assert f["projection"]["out_dim"] == 32 and f["num_subspaces"] == 16 and f["n_rows"] == FLAT_N
    _check_projected(index, f, rows, q, mat, "txh_build_projected")
    for h in (index, proj, src):
        h.close()


def test_txh_create_projected(tmp_path, monkeypatch):
    _knob(monkeypatch, **FORMS["flat"])
    rows, q, mat = _projected_inputs()
    rows_p = pm.project(pm.MATRIX, rows, mat, None, out_dim=32)
    ix = trainer.build_ah_index(rows_p, 16, K=16, pq_iters=3)
    data, stride = orc.to_strided(rows)
    proj = hip.Projection(hip.PROJ_MATRIX, matrix=mat)
    index = hip.txh_create_projected(projection=proj, rows=data, n_rows=FLAT_N, row_dim=96, row_stride=stride, dim=32,
                                     centers=None, leaf_offsets=None, leaf_ids=None, codebook=ix["codebook"],
                                     codes=ix["codes"], use_residuals=False, partitions_to_search=1,
                                     pre_reorder_multiplier=float(M) / K, distance_measure=hip.SQUARED_L2)
    proj.close()
    f = dict(n_rows=FLAT_N, codebook=ix["codebook"], codes=ix["codes"], codes_packed4=0, num_subspaces=16)
    _check_projected(index, f, rows, q, mat, "txh_create_projected")
    index.close()


# ---- quantized re-rank rows ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def quantized_bases():
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = QC.Base(64, n=FLAT_N if kind == "flat" else TREE_N, nq=NQ, leaves=TREE_L, p=TREE_P)
        return cache[kind]

    yield get
    cache.clear()


@pytest.mark.parametrize("fmt", list(QC.FMTS))
@pytest.mark.parametrize("kind", ["flat", "tree"])
def test_txh_create_quantized(kind, fmt, quantized_bases, monkeypatch):
    """bf16, FP8 and int8 rows: the result rows bitwise the model's over the oracle's merged candidates, the device's
    candidates the oracle's up to ties (tests/test_gpu_quantized_rerank.py _run, under the forced prefilter)"""
    _knob(monkeypatch, **FORMS[kind])
    base = quantized_bases(kind)
    bkind = "ah" if kind == "flat" else "txh"
    f = QC.FMTS[fmt]
    elems, inv = QC.quantize(base.rows, f)
    index = _create(base, bkind, elems, f, hip.SQUARED_L2, inv)
    index.enable_timing(True)
    what = "quantized %s %s" % (kind, fmt)
    want = base.model_rows(bkind, elems, f, hip.SQUARED_L2, inv, K, M, NQ)
    got = index.search_batched(base.q[:NQ], K, base.opts(bkind, M))
    _scan_ran(index, kind, base.n)
    _assert_rows(got, want, K, what)
    gi, gd, gc, st = index.search_batched(base.q[:NQ], K, base.opts(bkind, M), stages=True)
    _scan_ran(index, kind, base.n)
    _assert_candidates(base, bkind, M, NQ, st, what)
    _assert_rows((gi, gd, gc), want, K, what + " staged")
    index.close()

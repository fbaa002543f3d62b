"""Pins tests/quantized_rerank_model.py, the checker of tests/test_gpu_quantized_rerank.py.  CPU only.

* The model equals a brute-force search by tests/quantized_checker.py restricted to the candidate set, ties by merged
  position: random rows and duplicated rows, every format and measure.
* int8: quantized_checker.distances IS orc.one_to_many over f32(i8) * inv (asserted bit for bit at every dimension
  the GPU tests use, SquaredL2 and DotProduct), so the whole search is pinned a second way there: the oracle's own
  tree / hasher search over an index whose `data` is the dequantized rows.
* the index-file sections rows_q / rows_q_meta through the Python writer and reader, and the C writer's header view;
* the ABI symbol check with the new declarations."""
import ctypes

import numpy as np
import pytest

from oracle import pyoracle as orc
from scann_rust_amd import hip, index_file
from tests import quantized_checker as qc
from tests import quantized_rerank_cases as QC
from tests import quantized_rerank_model as QM

K, M, NQ = 10, 33, 6


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def base():
    return QC.Base(36, n=1500, nq=NQ)


def _restricted_brute_force(q, ci, rows_q, dim, fmt, measure, inv, k):
    """every row scored by the checker, the candidates picked out, (ordered distance, merged position) sorted"""
    d = qc.distances(q[None], rows_q, dim, fmt, measure, inv)[0]
    key = QM.f32_to_ordered(d)
    order = sorted(range(len(ci)), key=lambda p: (int(key[ci[p]]), p))[:k]
    return np.array([ci[p] for p in order], np.uint32), np.array([d[ci[p]] for p in order], np.float32)


@pytest.mark.parametrize("rows_kind", ["random", "duplicated"])
@pytest.mark.parametrize("fmt", list(QC.FMTS))
def test_model_is_brute_force_over_the_candidates(base, fmt, rows_kind):
    f = QC.FMTS[fmt]
    rows = base.rows if rows_kind == "random" else base.rows[np.arange(base.n) % 7]
    elems, inv = QC.quantize(rows, f)
    rows_q = QC.with_stride(elems, base.dim + 5, seed=1)
    ties = 0
    for kind in ("txh", "ah"):
        for measure in QC.MEASURES.values():
            for i in range(NQ):
                ci, _ = base.candidates(kind, i, M)
                gi, gd = QM.rerank(base.q[i], ci, rows_q, base.dim, f, measure, inv, K)
                wi, wd = _restricted_brute_force(base.q[i], ci, rows_q, base.dim, f, measure, inv, K)
                assert np.array_equal(gi, wi) and np.array_equal(_bits(gd), _bits(wd)), (kind, measure, i)
                ties += int(np.unique(_bits(gd)).size < gd.size)
    assert (ties > 0) == (rows_kind == "duplicated")   # the duplicated rows do exercise the tie rule


@pytest.mark.parametrize("dim", [8, 12, 36, 96, 128, 264])
def test_int8_checker_is_the_oracle_on_dequantized_rows_and_pins_the_search(dim):
    b = QC.Base(dim, n=1200, nq=4, leaves=8, p=3)
    elems, inv = QC.quantize(b.rows, qc.ROWS_INT8)
    deq = np.ascontiguousarray(elems.astype(np.float32) * np.float32(inv))   # f32(i8) * inv, one rounded product
    data, stride = orc.to_strided(deq)
    for measure in (qc.SQUARED_L2, qc.DOT_PRODUCT):
        got = qc.distances(b.q, elems, dim, qc.ROWS_INT8, measure, inv)
        for i in range(b.q.shape[0]):
            want = orc.one_to_many(b.q[i], data, stride, b.n, measure)
            assert np.array_equal(_bits(got[i]), _bits(want)), (dim, measure, i)   # holds at every dimension here
    # ... so the oracle's own searches over the dequantized rows are a second statement of the model
    o = b.oix
    oix = orc.TxhIndex(data, stride, dim, o.centers, o.leaf_off, o.leaf_ids, o.codebook, o.codes, use_residuals=False,
                       partitions_to_search=b.p, pre_reorder_multiplier=(M + 0.5) / K)
    assert orc.pre_reorder_k(K, oix.pre_reorder_multiplier) == M
    for i in range(b.q.shape[0]):
        oi, od, _, _, oci, _ = orc.txh_search(oix, b.q[i], K, stages=True)
        ci, _ = b.candidates("txh", i, M)
        assert np.array_equal(ci, oci)   # the candidates do not depend on the rows
        mi, md = QM.rerank(b.q[i], ci, elems, dim, qc.ROWS_INT8, qc.SQUARED_L2, inv, K)
        assert np.array_equal(mi, oi) and np.array_equal(_bits(md), _bits(od)), ("txh", dim, i)
        ai, ad = orc.ah_search_with_reordering(b.cb, b.codes, data, stride, b.q[i], K, M)
        ci, _ = b.candidates("ah", i, M)
        mi, md = QM.rerank(b.q[i], ci, elems, dim, qc.ROWS_INT8, qc.SQUARED_L2, inv, K)
        assert np.array_equal(mi, ai) and np.array_equal(_bits(md), _bits(ad)), ("ah", dim, i)
        ri, rd = orc.reorder_measure(data, stride, dim, qc.DOT_PRODUCT, b.q[i], ci, K)
        mi, md = QM.rerank(b.q[i], ci, elems, dim, qc.ROWS_INT8, qc.DOT_PRODUCT, inv, K)
        assert np.array_equal(mi, ri) and np.array_equal(_bits(md), _bits(rd)), ("dot", dim, i)


def test_ordered_key_orders_nan_and_infinities():
    d = np.array([np.inf, 1.0, -np.inf, -0.0, 0.0, -1.0], np.float32)
    nan = np.array([0x7FC00000, 0xFFC00000], np.uint32).view(np.float32)
    key = QM.f32_to_ordered(np.concatenate([d, nan]))
    assert list(np.argsort(key, kind="stable")) == [7, 2, 5, 3, 4, 1, 0, 6]


@pytest.mark.parametrize("fmt", list(QC.FMTS))
def test_index_file_round_trip_of_quantized_rows(tmp_path, base, fmt):
    f = QC.FMTS[fmt]
    elems, inv = QC.quantize(base.rows, f)
    inv = 0.0123 if f == qc.ROWS_INT8 else inv
    stride = base.dim + 5
    rows_q = QC.with_stride(elems, stride, seed=2)
    kw = base.desc("txh", stride, hip.DOT_PRODUCT)
    S, Kc, dsub = kw["codebook"].shape
    path = str(tmp_path / "q.scannidx")
    index_file.write(path, kind=1, n_rows=base.n, n_local=base.n, dim=base.dim, stride=stride,
                     num_partitions=kw["centers"].shape[0], num_subspaces=S, num_codes=Kc, dims_per_subspace=dsub,
                     distance_measure=hip.DOT_PRODUCT, use_residuals=0, partitions_to_search=QC.P,
                     pre_reorder_multiplier=3.0,
                     sections=index_file.rows_q_sections(rows_q, f, inv) +
                     [("centers", kw["centers"]), ("leaf_offsets", kw["leaf_offsets"]), ("leaf_ids", kw["leaf_ids"]),
                      ("codebook", kw["codebook"]), ("codes", kw["codes"])])
    header, secs = index_file.read(path)
    assert "data" not in secs and secs["rows_q"].dtype == np.uint8
    assert secs["rows_q"].nbytes == rows_q.nbytes and np.array_equal(secs["rows_q"], rows_q.reshape(-1).view(np.uint8))
    assert secs["rows_q_meta"].dtype == np.uint32 and secs["rows_q_meta"].size == 2
    assert int(secs["rows_q_meta"][0]) == f
    assert int(secs["rows_q_meta"][1]) == int(np.array([inv], np.float32).view(np.uint32)[0])
    a = index_file.arrays(path)
    assert a["fmt"] == f and np.float32(a["inv_multiplier"]) == np.float32(inv) and "data" not in a
    assert a["rows_q"].dtype == QC.DTYPES[f] and np.array_equal(a["rows_q"], rows_q)
    assert np.array_equal(a["codes"], kw["codes"]) and np.array_equal(a["leaf_ids"], kw["leaf_ids"])
    info = hip.index_file_info(path)   # the C reader's header view: no f32 rows in this file
    assert info["has_data"] == 0 and info["n_rows"] == base.n and info["stride"] == stride


def test_abi_symbols_with_the_new_declarations():
    from tests import test_abi_and_host as T
    T.test_header_symbols_are_exported()
    declared = T._declared_symbols()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in ("scann_hip_txh_create_quantized", "scann_hip_index_device_bytes"):
        assert name in declared and name in hip.EXPORTS and hasattr(lib, name)
    assert callable(hip.txh_create_quantized) and callable(hip.Index.device_bytes)

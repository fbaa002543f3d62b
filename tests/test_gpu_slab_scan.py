"""LUT16 indexes with 96 .. 512 subspaces: the slab-walking scan (txh_slab.hip) against the CPU oracle.

Approximate distances bitwise, candidates up to exact ties, final rows as helpers.check_txh_query / check_ah_query rule;
search_batched raises unless the status is Ok.  Leaves that are no multiple of the 512-point tile, one empty leaf, 33
queries (a partial quad, several quad groups), 130 over one long leaf (sample stride 2), odd and even slab counts."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as orc
from scann_rust_amd import hip, index_file, synth
from tests import helpers as H

pytestmark = pytest.mark.gpu

K, P, L, N, NQ = 10, 3, 7, 4133, 33
TREE_DIM = {96: 96, 128: 256, 384: 768, 512: 512}
SLAB = "adc_slab_scan_kernel"


@functools.lru_cache(maxsize=None)
def tree_case(S):
    """(txh_create kwargs, queries) of a residual tree whose leaf 2 is emptied: its rows stay in `data`, off the index"""
    dim = TREE_DIM[S]
    _, _, _, ix, _, kw = H.make_txh_case(N, dim, L, S, seed=S, P=P, mult=4.0, kmeans_iters=2, pq_iters=1)
    lo, hi = int(ix["leaf_off"][2]), int(ix["leaf_off"][3])
    keep = np.r_[0:lo, hi:N]
    off = ix["leaf_off"].copy()
    off[3:] -= hi - lo
    kw = dict(kw, leaf_offsets=off, leaf_ids=ix["leaf_ids"][keep].copy(), codes=ix["codes"][keep].copy())
    return kw, synth.uniform_f32(NQ, dim, 1000 + S)


def oracle_of(kw, m, allow=None):
    oix = orc.TxhIndex(kw["data"], kw["stride"], kw["dim"], kw["centers"], kw["leaf_offsets"], kw["leaf_ids"],
                       kw["codebook"], kw["codes"], use_residuals=kw["use_residuals"], partitions_to_search=P,
                       pre_reorder_multiplier=m / K)
    oix.allow = allow
    return oix


def timed(kw):
    index = hip.txh_create(**kw)
    index.enable_timing(True)
    return index


def tree_opts(m):
    o = hip.default_opts()
    o.partitions_to_search, o.pre_reorder_k = P, m
    return o


def check_tree(staged, kw, q, m, what, allow=None):
    idx, dist, cnt, (tok, tokd, ci, cd, cc) = staged
    for i in range(q.shape[0]):
        a = allow if allow is None or allow.ndim == 1 else allow[i]
        H.check_txh_query(oracle_of(kw, m, a), q[i], K, idx[i, :cnt[i]], dist[i, :cnt[i]], tok[i], tokd[i],
                          ci[i, :cc[i]], cd[i, :cc[i]], what="%s q%d" % (what, i))


@pytest.mark.parametrize("m", [40, 1000])
@pytest.mark.parametrize("S", sorted(TREE_DIM))
def test_tree_stage_by_stage(S, m):
    kw, q = tree_case(S)
    index = timed(kw)
    staged = index.search_batched(q, K, tree_opts(m), stages=True)
    assert index.last_kernel_ms()[1] == SLAB
    check_tree(staged, kw, q, m, "S%d m%d" % (S, m))


@functools.lru_cache(maxsize=None)
def flat_case(S):
    _, data, stride, ix, kw = H.make_ah_case(6145, 768, S, seed=S + 1, pq_iters=1)
    return kw, ix, synth.uniform_f32(130, 768, 2000 + S)


@pytest.mark.parametrize("reorder", [1, 0])
@pytest.mark.parametrize("nq", [33, 130])
@pytest.mark.parametrize("S", [96, 384])
def test_flat_hasher(S, nq, reorder):
    kw, ix, q = flat_case(S)
    q, m = q[:nq], 200
    index = timed(kw)
    o = hip.default_opts()
    o.pre_reorder_k, o.exact_reorder = m, reorder
    idx, dist, cnt, (_, _, ci, cd, cc) = index.search_batched(q, K, o, stages=True)
    assert index.last_kernel_ms()[1] == SLAB
    for i in range(0, nq, 4):
        if reorder:
            H.check_ah_query(ix["codebook"], ix["codes"], kw["data"], kw["stride"], 768, q[i], K, m, idx[i, :cnt[i]],
                             dist[i, :cnt[i]], ci[i, :cc[i]], cd[i, :cc[i]], what="q%d" % i)
        else:
            oi, od = orc.ah_search(ix["codebook"], ix["codes"], q[i], K)
            assert cnt[i] == K and np.array_equal(dist[i].view(np.uint32), od.view(np.uint32)), i
            H.assert_topk_equal_up_to_ties(idx[i], dist[i], oi, od, what="q%d" % i)


@pytest.mark.parametrize("per_query", [False, True])
def test_allow_lists(per_query):
    """one bitmap for the batch, and one per query: query 0 allows nothing, query 1 only the rows of leaf 4"""
    kw, q = tree_case(96)
    rng = np.random.default_rng(5)
    allow = H.words_of(np.flatnonzero(rng.random(N) < 0.6), N)[0]
    if per_query:
        allow = np.stack([H.words_of(np.flatnonzero(rng.random(N) < 0.3 + 0.02 * i), N)[0] for i in range(NQ)])
        allow[0] = 0
        off = kw["leaf_offsets"]
        allow[1] = H.words_of(np.sort(kw["leaf_ids"][off[4]:off[5]]), N)[0]
    index = timed(kw)
    for m in (40, 1000):
        staged = index.search_batched(q, K, tree_opts(m), stages=True, allow=allow, allow_bits=N)
        assert index.last_kernel_ms()[1] == SLAB
        check_tree(staged, kw, q, m, "allow m%d" % m, allow)
        if per_query:
            assert staged[2][0] == 0


@pytest.mark.parametrize("wide", ["0", "2"])
@pytest.mark.parametrize("nq", [1, 8])
def test_few_queries_equal_the_batched_run(nq, wide, monkeypatch):
    """the Small pipeline, and the Wide one under SCANN_HIP_WIDE=2 (up to 4 queries a call), at S = 384"""
    kw, _, q = flat_case(384)
    index = timed(kw)
    o = hip.default_opts()
    o.pre_reorder_k = 200
    monkeypatch.setenv("SCANN_HIP_SMALL", "0")
    ref = index.search_batched(q[:nq], K, o)
    assert index.last_kernel_ms()[1] == SLAB
    monkeypatch.delenv("SCANN_HIP_SMALL")
    monkeypatch.setenv("SCANN_HIP_WIDE", wide)
    step = 4 if wide == "2" else nq
    for lo in range(0, nq, step):
        got = index.search_batched(q[lo:min(nq, lo + step)], K, o)
        assert index.last_kernel_ms()[1] == ("wide_scan_kernel" if wide == "2" else "small_scan_kernel")
        hi = lo + got[0].shape[0]
        assert all(np.array_equal(g.view(np.uint32), r[lo:hi].view(np.uint32)) for g, r in zip(got, ref))


@pytest.mark.parametrize("family", ["all-15", "all-0", "tied", "nan-query"])
def test_degenerate_tables(family):
    kw, q = tree_case(96)
    kw = dict(kw)
    if family in ("all-15", "all-0"):
        kw["codes"] = np.full_like(kw["codes"], 15 if family == "all-15" else 0)
    elif family == "tied":   # every centre of a subspace is the same value: every point sums to one distance
        kw["codebook"] = np.ascontiguousarray(np.broadcast_to(kw["codebook"][:, :1, :], (96, 16, 1)), np.float32)
    q = q.copy()
    if family == "nan-query":
        q[5, 17] = np.nan
    index = timed(kw)
    idx, dist, cnt, (tok, tokd, ci, cd, cc) = index.search_batched(q, K, tree_opts(40), stages=True)
    if family == "nan-query":
        otok = orc.txh_search(oracle_of(kw, 40), q[5], K, stages=True)[2]
        assert np.array_equal(tok[5], otok)
        keep = np.arange(NQ) != 5
        q = q[keep]
        idx, dist, cnt, tok, tokd, ci, cd, cc = (a[keep] for a in (idx, dist, cnt, tok, tokd, ci, cd, cc))
    check_tree((idx, dist, cnt, (tok, tokd, ci, cd, cc)), kw, q, 40, family)


def test_device_build_and_file_round_trip(tmp_path):
    """hip.txh_build at S = 96 against the oracle over the arrays it wrote; a re-loaded index returns identical rows"""
    n, dim = 2000, 96
    rows = synth.uniform_f32(n, dim, 77)
    data, stride = orc.to_strided(rows)
    src = hip.bf_create(data, n, dim, stride, hip.SQUARED_L2)
    index, _ = hip.txh_build(src, num_partitions=5, num_subspaces=96, num_codes=16, kmeans_iterations=2,
                             training_iterations=2, partitions_to_search=P)
    path = str(tmp_path / "built.scannidx")
    hip.index_write_file(index, path)
    f = index_file.arrays(path)
    codes = orc.unpack4(f["codes"], 96) if f["codes_packed4"] else f["codes"]
    kw = dict(data=data, stride=stride, dim=dim, centers=f["centers"], leaf_offsets=f["leaf_offsets"],
              leaf_ids=f["leaf_ids"], codebook=f["codebook"], codes=codes, use_residuals=bool(f["use_residuals"]))
    q = synth.uniform_f32(NQ, dim, 78)
    check_tree(index.search_batched(q, K, tree_opts(40), stages=True), kw, q, 40, "built")
    src.close()

    kw, q = tree_case(128)
    first = hip.txh_create(**kw)
    path = str(tmp_path / "tree.scannidx")
    hip.index_write_file(first, path)
    again = hip.load_file(path)
    a, b = first.search_batched(q, K, tree_opts(40)), again.search_batched(q, K, tree_opts(40))
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


@pytest.mark.parametrize("S,ok", [(72, False), (544, False), (96, True)])
def test_subspace_counts_refused_and_accepted(S, ok):
    kw = H.ah_kwargs_from_codes(synth.uniform_f32(64, S, 9), synth.uniform_f32(S * 16, 1, 10).reshape(S, 16, 1),
                                np.zeros((64, S), np.uint8))
    if ok:
        assert hip.txh_create(**kw).size() == 64
    else:
        with pytest.raises(hip.ScannError) as e:
            hip.txh_create(**kw)
        assert e.value.code == hip.UNIMPLEMENTED

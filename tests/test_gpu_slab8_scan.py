"""Byte-code indexes (16 < num_codes <= 256) with 24 .. 128 subspaces: txh_slab8.hip against the CPU oracle, by the rule
of test_gpu_slab_scan.py.  A leaf longer than the 2048-point item and no multiple of it, one empty leaf, 33 queries (a
partial quad, an odd number of two-quad groups), 130 over three chunks and a point, a 100-code table in 256 slots."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as orc
from scann_rust_amd import hip, index_file, synth
from tests import helpers as H

pytestmark = pytest.mark.gpu

K, P, L, N, NQ = 10, 3, 3, 6150, 33
TREE = {24: (48, 256), 32: (128, 256), 72: (144, 100), 128: (256, 256)}   # S: (dim, num_codes)
SLAB8 = "adc_slab8_scan_kernel"


def sampled_pq(rows, S, codes, seed):
    """a codebook of `codes` sampled rows (tests/test_gpu_txh_subspaces.py) and every row's nearest code per subspace"""
    n, dim = rows.shape
    pick = np.random.default_rng(seed).choice(n, codes, replace=False)
    x = rows.reshape(n, S, dim // S).transpose(1, 0, 2).astype(np.float64)   # [S, n, dsub]
    cb = x[:, pick]
    near = [((cb[s] ** 2).sum(1)[None] - 2.0 * x[s] @ cb[s].T).argmin(1) for s in range(S)]
    return np.ascontiguousarray(cb, np.float32), np.ascontiguousarray(np.stack(near, 1), np.uint8)


@functools.lru_cache(maxsize=None)
def tree_case(S):
    """(txh_create kwargs, queries) of a residual tree whose shortest leaf is emptied: its rows stay in `data` only"""
    dim, codes = TREE[S]
    rows = synth.uniform_f32(N, dim, S)
    _, kw = H.txh_from_codes(rows, *sampled_pq(rows, S, codes, S), L, P, 4.0, seed=S)
    off = kw["leaf_offsets"].astype(np.int64)
    e = int(np.argmin(np.diff(off)))
    keep = np.r_[0:off[e], off[e + 1]:N]
    off[e + 1:] -= off[e + 1] - off[e]
    kw = dict(kw, leaf_offsets=off.astype(np.uint32), leaf_ids=kw["leaf_ids"][keep].copy(), codes=kw["codes"][keep].copy())
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


def opts(m, partitions=P, reorder=1):
    o = hip.default_opts()
    o.partitions_to_search, o.pre_reorder_k, o.exact_reorder = partitions, m, reorder
    return o


def check_tree(staged, kw, q, m, what, allow=None):
    idx, dist, cnt, (tok, tokd, ci, cd, cc) = staged
    for i in range(q.shape[0]):
        a = allow if allow is None or allow.ndim == 1 else allow[i]
        H.check_txh_query(oracle_of(kw, m, a), q[i], K, idx[i, :cnt[i]], dist[i, :cnt[i]], tok[i], tokd[i],
                          ci[i, :cc[i]], cd[i, :cc[i]], what="%s q%d" % (what, i))


@pytest.mark.parametrize("m", [40, 1000])
@pytest.mark.parametrize("S", sorted(TREE))
def test_tree_stage_by_stage(S, m):
    kw, q = tree_case(S)
    assert np.diff(kw["leaf_offsets"].astype(np.int64)).max() > 2048
    index = timed(kw)
    staged = index.search_batched(q, K, opts(m), stages=True)
    assert index.last_kernel_ms()[1] == SLAB8
    check_tree(staged, kw, q, m, "S%d m%d" % (S, m))


@functools.lru_cache(maxsize=None)
def flat_case(S):
    rows = synth.uniform_f32(6145, 256, S + 1)
    cb, codes = sampled_pq(rows, S, 256, S + 1)
    return H.ah_kwargs_from_codes(rows, cb, codes), dict(codebook=cb, codes=codes), synth.uniform_f32(130, 256, 2000 + S)


@pytest.mark.parametrize("reorder", [1, 0])
@pytest.mark.parametrize("nq", [33, 130])
@pytest.mark.parametrize("S", [32, 128])
def test_flat_hasher(S, nq, reorder):
    kw, ix, q = flat_case(S)
    q, m = q[:nq], 200
    index = timed(kw)
    idx, dist, cnt, (_, _, ci, cd, cc) = index.search_batched(q, K, opts(m, 1, reorder), stages=True)
    assert index.last_kernel_ms()[1] == SLAB8
    for i in range(nq):
        if reorder:
            H.check_ah_query(ix["codebook"], ix["codes"], kw["data"], kw["stride"], 256, q[i], K, m, idx[i, :cnt[i]],
                             dist[i, :cnt[i]], ci[i, :cc[i]], cd[i, :cc[i]], what="q%d" % i)
        else:
            oi, od = orc.ah_search(ix["codebook"], ix["codes"], q[i], K)
            assert cnt[i] == K and np.array_equal(dist[i].view(np.uint32), od.view(np.uint32)), i
            H.assert_topk_equal_up_to_ties(idx[i], dist[i], oi, od, what="q%d" % i)


@pytest.mark.parametrize("per_query", [False, True])
def test_allow_lists(per_query):
    """one bitmap for the batch; one per query: query 0 allows nothing, query 1 only the rows of leaf 0"""
    kw, q = tree_case(24)
    rng = np.random.default_rng(5)
    allow = H.words_of(np.flatnonzero(rng.random(N) < 0.6), N)[0]
    if per_query:
        allow = np.stack([H.words_of(np.flatnonzero(rng.random(N) < 0.3 + 0.02 * i), N)[0] for i in range(NQ)])
        allow[0] = 0
        allow[1] = H.words_of(np.sort(kw["leaf_ids"][:kw["leaf_offsets"][1]]), N)[0]
    index = timed(kw)
    for m in (40, 1000):
        staged = index.search_batched(q, K, opts(m), stages=True, allow=allow, allow_bits=N)
        assert index.last_kernel_ms()[1] == SLAB8
        check_tree(staged, kw, q, m, "allow m%d" % m, allow)
        if per_query:
            assert staged[2][0] == 0


@pytest.mark.parametrize("wide", ["0", "2"])
@pytest.mark.parametrize("nq", [1, 8])
def test_few_queries_equal_the_batched_run(nq, wide, monkeypatch):
    """the Small pipeline, and the Wide one under SCANN_HIP_WIDE=2 (up to 4 queries a call), at S = 128: 132 KB of LDS"""
    kw, _, q = flat_case(128)
    index, o = timed(kw), opts(200, 1)
    monkeypatch.setenv("SCANN_HIP_SMALL", "0")
    ref = index.search_batched(q[:nq], K, o)
    assert index.last_kernel_ms()[1] == SLAB8
    monkeypatch.delenv("SCANN_HIP_SMALL")
    monkeypatch.setenv("SCANN_HIP_WIDE", wide)
    step = 4 if wide == "2" else nq
    for lo in range(0, nq, step):
        got = index.search_batched(q[lo:min(nq, lo + step)], K, o)
        assert index.last_kernel_ms()[1] == ("wide_scan_kernel" if wide == "2" else "small_scan_kernel")
        hi = lo + got[0].shape[0]
        assert all(np.array_equal(g.view(np.uint32), r[lo:hi].view(np.uint32)) for g, r in zip(got, ref))


@pytest.mark.parametrize("family", ["all-255", "all-0", "tied", "nan-query"])
def test_degenerate_tables(family):
    kw, q = tree_case(24)
    kw, q = dict(kw), q.copy()
    if family in ("all-255", "all-0"):
        kw["codes"] = np.full_like(kw["codes"], 255 if family == "all-255" else 0)
    elif family == "tied":   # every centre of a subspace is the same value: every point sums to one distance
        kw["codebook"] = np.repeat(kw["codebook"][:, :1, :], 256, axis=1)
    elif family == "nan-query":
        q[5, 17] = np.nan
    idx, dist, cnt, (tok, tokd, ci, cd, cc) = timed(kw).search_batched(q, K, opts(40), stages=True)
    if family == "nan-query":
        otok = orc.txh_search(oracle_of(kw, 40), q[5], K, stages=True)[2]
        assert np.array_equal(tok[5], otok)
        keep = np.arange(NQ) != 5
        q = q[keep]
        idx, dist, cnt, tok, tokd, ci, cd, cc = (a[keep] for a in (idx, dist, cnt, tok, tokd, ci, cd, cc))
    check_tree((idx, dist, cnt, (tok, tokd, ci, cd, cc)), kw, q, 40, family)


def test_device_build_and_file_round_trip(tmp_path):
    """hip.txh_build at S = 24, K = 256 against the oracle over the arrays it wrote; re-loaded, it returns identical rows"""
    n, dim = 2000, 96
    rows = synth.uniform_f32(n, dim, 77)
    data, stride = orc.to_strided(rows)
    src = hip.bf_create(data, n, dim, stride, hip.SQUARED_L2)
    index, _ = hip.txh_build(src, num_partitions=5, num_subspaces=24, num_codes=256, kmeans_iterations=2,
                             training_iterations=2, partitions_to_search=P)
    index.enable_timing(True)
    path = str(tmp_path / "built.scannidx")
    hip.index_write_file(index, path)
    f = index_file.arrays(path)
    assert not f["codes_packed4"]
    kw = dict(data=data, stride=stride, dim=dim, centers=f["centers"], leaf_offsets=f["leaf_offsets"],
              leaf_ids=f["leaf_ids"], codebook=f["codebook"], codes=f["codes"], use_residuals=bool(f["use_residuals"]))
    q = synth.uniform_f32(NQ, dim, 78)
    staged = index.search_batched(q, K, opts(40), stages=True)
    assert index.last_kernel_ms()[1] == SLAB8
    check_tree(staged, kw, q, 40, "built")
    again = hip.load_file(path).search_batched(q, K, opts(40))
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(staged[:3], again))
    src.close()


@pytest.mark.parametrize("S,codes,ok", [(24, 256, True), (128, 256, True), (32, 32, True), (32, 31, False),
                                        (20, 256, False), (136, 256, False), (2, 256, False)])
def test_shapes_refused_and_accepted(S, codes, ok):
    kw = H.ah_kwargs_from_codes(synth.uniform_f32(64, S, 9), synth.uniform_f32(S * codes, 1, 10).reshape(S, codes, 1),
                                np.zeros((64, S), np.uint8))
    if ok:
        assert hip.txh_create(**kw).size() == 64
    else:
        with pytest.raises(hip.ScannError) as e:
            hip.txh_create(**kw)
        assert e.value.code == hip.UNIMPLEMENTED

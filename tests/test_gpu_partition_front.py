"""The front end of every tree search -- centroid scores, leaf selection with its key bases, work lists -- at thousands
of leaves and probes, against the oracle: the shapes of tests/partition_cases.py, which cross every switch of
launch_partition_stage, select_leaves_body, sel_cfg, kDecodeStage and the pipelines' leaf limit
(tests/test_partition_cases.py holds the table to that).  Indexes are synthetic: centroids and an explicit assignment,
no k-means.

  a. hip.txh_partition == orc.partition bit for bit: counts, tokens element by element (the reference's order is total:
     ties to the lower leaf id, NaN last) and distances -- duplicated and identical centroids, a query on a centroid,
     +inf and NaN distances.
  b. whole searches stage by stage (tokens, token distances, candidates, final rows), through the staged kernels, the
     small-batch kernels with their inline scoring and the wide ones.
  c. two leaf shards: the merge keys' low words are the key bases summed from the global leaf sizes."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as orc
from scann_rust_amd import hip, trainer
from tests import helpers as H
from tests import partition_cases as PC

pytestmark = pytest.mark.gpu

K = PC.K
MODES = {"txh": (8, 16), "bytes": (4, 32)}      # (S, K) of the codebook
STAGED_KERNELS = ("adc_scan_kernel", "adc_scan_res_kernel", "adc_mfma_kernel", "adc_mfma16_kernel", "adc_smfmac_kernel")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _csr(assign, L):
    leaf_ids = np.argsort(assign, kind="stable").astype(np.uint32)
    leaf_off = np.zeros(L + 1, np.uint32)
    leaf_off[1:] = np.cumsum(np.bincount(assign, minlength=L))
    return leaf_off, leaf_ids


# ---- a. partition, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PC.CASES, ids=[c.name for c in PC.CASES])
def test_partition_bit_exact_at_scale(case):
    """Counts, tokens and distances of every query equal the oracle's.  The two cases marked `fix` were refused with
    RESOURCE_EXHAUSTED ("kernel needs more than 160 KB of LDS") before launch_partition_stage sized the select path
    against the CU's LDS: 164 480 and 189 056 bytes asked for."""
    L, P, dim = case.L, case.P, case.dim
    centers = PC.centroids(case.name, L, dim, case.centroids)
    rows, assign = PC.rows_and_assign(case.name, centers, PC.leaf_sizes(case.name, L, case.leaves, case.avg))
    leaf_off, leaf_ids = _csr(assign, L)
    data, stride = orc.to_strided(rows)
    index = hip.txh_create(data=data, n_rows=rows.shape[0], dim=dim, stride=stride, centers=centers,
                           leaf_offsets=leaf_off, leaf_ids=leaf_ids, codebook=None, codes=None,
                           partitions_to_search=P, distance_measure=hip.SQUARED_L2)
    q = PC.queries(case.name, PC.NQ, dim, case.queries, centers)
    tok, dist, cnt = hip.txh_partition(index, q, P)
    n = min(P, L)
    edges = case.queries == "edges"
    for i in range(PC.NQ):
        ot, od = orc.partition(centers, q[i], P)
        assert cnt[i] == ot.size == n, "%s q%d: count %d" % (case.name, i, cnt[i])
        bad = np.flatnonzero(tok[i, :n] != ot)
        assert bad.size == 0, "%s q%d: %d tokens differ, first at rank %d: %d, oracle %d" % (
            case.name, i, bad.size, bad[0], tok[i, bad[0]], ot[bad[0]])
        if edges and i == PC.NAN_QUERY:      # NaN payloads differ between host and device: NaN-ness only
            assert np.isnan(od).all() and np.isnan(dist[i, :n]).all()
        else:
            assert np.array_equal(bits(dist[i, :n]), bits(od)), "%s q%d: distances" % (case.name, i)
    # what the families are there for, stated without the oracle
    if case.centroids == "identical":
        assert np.array_equal(tok[:, :n], np.tile(np.arange(n, dtype=np.uint32), (PC.NQ, 1)))
    if edges:
        assert np.array_equal(tok[PC.INF_QUERY, :n], np.arange(n)) and np.array_equal(tok[PC.NAN_QUERY, :n], np.arange(n))
        assert np.all(bits(dist[PC.INF_QUERY, :n]) == 0x7F800000)
        twins = np.flatnonzero((centers == centers[L // 2]).all(1))        # the centroid the query sits on, and its copies
        assert bits(dist[PC.HIT_QUERY, :1])[0] == 0 and np.array_equal(tok[PC.HIT_QUERY, :min(n, twins.size)], twins[:n])


# ---- b. whole searches ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _built(name):
    """(case, kwargs of hip.txh_create, queries, oracle view or None, arrays) of a search case: built once"""
    s = next(c for c in PC.SEARCHES + PC.SHARDED if c.name == name)
    centers = PC.centroids(name, s.L, s.dim, "uniform")
    sizes = PC.leaf_sizes(name, s.L, s.leaves, s.avg)
    rows, assign = PC.rows_and_assign(name, centers, sizes, near=False)     # rows of every rank's leaf reach the results
    data, stride = orc.to_strided(rows)
    q = PC.queries(name, s.nq, s.dim, "uniform", centers)
    q[1] = centers[s.L // 2]                                               # a query on a centroid
    kw = dict(data=data, n_rows=rows.shape[0], dim=s.dim, stride=stride, centers=centers, partitions_to_search=s.P)
    if s.mode == "partitioned":
        leaf_off, leaf_ids = _csr(assign, s.L)
        kw.update(leaf_offsets=leaf_off, leaf_ids=leaf_ids, codebook=None, codes=None, distance_measure=hip.SQUARED_L2)
        return s, kw, q, None, dict(centers=centers, leaf_off=leaf_off, leaf_ids=leaf_ids, data=data, stride=stride, assign=assign)
    S, Kc = MODES[s.mode]
    ix = trainer.build_txh_index(rows, s.L, S, K=Kc, centers=centers, assign=assign, pq_iters=1)
    kw.update(leaf_offsets=ix["leaf_off"], leaf_ids=ix["leaf_ids"], codebook=ix["codebook"], codes=ix["codes"],
              codes_packed4=False, use_residuals=True, pre_reorder_multiplier=3.0)
    return s, kw, q, ix, dict(data=data, stride=stride, sizes=sizes, assign=assign)


def _oracle_view(s, ix, arr, m):
    return orc.TxhIndex(arr["data"], arr["stride"], s.dim, ix["centers"], ix["leaf_off"], ix["leaf_ids"], ix["codebook"],
                        ix["codes"], partitions_to_search=s.P, pre_reorder_multiplier=m / K)


def _opts(P, m):
    o = hip.default_opts()
    o.partitions_to_search, o.pre_reorder_k = P, m
    return o


def _search_with_tokens(index, q, o, P):
    """search_batched with the token outputs alone: a small batch keeps its own pipeline (candidate outputs would send
    it through the staged kernels), so these are the tokens of the inline scoring"""
    tok, tokd = np.zeros((q.shape[0], P), np.uint32), np.zeros((q.shape[0], P), np.float32)
    o.tokens, o.token_dists = hip.ptr(tok, hip.u32p), hip.ptr(tokd, hip.f32p)
    try:
        idx, dist, cnt = index.search_batched(q, K, o)
    finally:
        o.tokens = o.token_dists = None
    return idx, dist, cnt, tok, tokd


def _deepest_rank(L, tokens, leaves):
    """the largest rank, in the query's token order, among the leaves given"""
    rank = np.full(L, -1, np.int64)
    rank[tokens] = np.arange(tokens.size)
    assert (rank[leaves] >= 0).all()
    return int(rank[leaves].max()) if leaves.size else -1


def _same_rows(what, got, want):
    (gi, gd, gc), (wi, wd, wc) = got, want
    assert np.array_equal(gc, wc), what
    assert np.array_equal(bits(gd), bits(wd)), "%s: distances" % what
    for i in range(gi.shape[0]):
        H.assert_topk_equal_up_to_ties(gi[i, :gc[i]], gd[i, :gc[i]], wi[i, :wc[i]], wd[i, :wc[i]], what="%s q%d" % (what, i))


SEARCH_RUNS = [(s.name, m, mfma) for s in PC.SEARCHES if s.mode != "partitioned" for m in s.ms
               for mfma in ((None, "3") if s.name == "staged-5000x600" and m == s.ms[0] else (None,))]


@pytest.mark.parametrize("name,m,mfma", SEARCH_RUNS, ids=["%s-m%d%s" % (n, m, "-mfma16" if f else "") for n, m, f in SEARCH_RUNS])
def test_search_stages_against_oracle(name, m, mfma, monkeypatch):
    """search_batched(stages=True) of every third query against the oracle, stage by stage; then the same batch with
    the token outputs alone and with no stage output at all: the same distances bit for bit, the same ids up to ties.
    For a small batch the first call runs the staged kernels (sorted candidates are theirs) and the other two the
    small-batch or wide kernels, whose tokens come from the inline scoring.  mfma: SCANN_HIP_MFMA=3, the 16-pair
    prefilter, whose refine decodes through the key bases as the final selects do."""
    s, kw, q, ix, arr = _built(name)
    ms = PC.max_stream(arr["sizes"], s.P)
    cl = PC.classify(s.L, s.P, s.dim, s.nq, m=m, ms=ms, wide=s.wide)
    monkeypatch.setenv("SCANN_HIP_WIDE", "2" if s.wide else "0")
    if mfma:
        monkeypatch.setenv("SCANN_HIP_MFMA", mfma)
    else:
        monkeypatch.delenv("SCANN_HIP_MFMA", raising=False)
    index = hip.txh_create(**kw)
    index.enable_timing(True)
    oix = _oracle_view(s, ix, arr, m)
    o = _opts(s.P, m)
    idx, dist, cnt, (tok, tokd, ci, cd, cc) = index.search_batched(q, K, o, stages=True)
    assert index.last_kernel_ms()[1] == ("adc_mfma16_kernel" if mfma else "adc_scan_kernel")
    oracle = {}
    for i in range(0, s.nq, 3):
        oracle[i] = orc.txh_search(oix, q[i], K, stages=True)
        H.check_txh_query(oix, q[i], K, idx[i, :cnt[i]], dist[i, :cnt[i]], tok[i], tokd[i], ci[i, :cc[i]], cd[i, :cc[i]],
                          what="%s q%d" % (name, i), oracle=oracle[i])
    assert np.array_equal(tok[1, :1], [s.L // 2]) and bits(tokd[1, :1])[0] == 0
    # the test's own reach: candidates and final rows come from leaves far down the token order, so a key base that is
    # wrong anywhere -- past the first wave of the prefix sums, past kDecodeStage -- decodes to a row the oracle lacks
    deep_c = max(_deepest_rank(s.L, o_[2], arr["assign"][o_[4]]) for o_ in oracle.values())
    deep_f = max(_deepest_rank(s.L, o_[2], arr["assign"][o_[0]]) for o_ in oracle.values())
    assert deep_c >= s.P * 3 // 4 and deep_f >= min(s.P // 2, 256), (deep_c, deep_f)
    # the token outputs alone
    idx2, dist2, cnt2, tok2, tokd2 = _search_with_tokens(index, q, o, s.P)
    assert np.array_equal(tok2, tok) and np.array_equal(bits(tokd2), bits(tokd)), "%s: tokens of the %s pipeline" % (name, cl["pipeline"])
    for i, (_, _, otok, otokd, _, _) in oracle.items():
        assert np.array_equal(tok2[i], otok) and np.array_equal(bits(tokd2[i]), bits(otokd))
    _same_rows(name + " tokens-only", (idx2, dist2, cnt2), (idx, dist, cnt))
    # no stage output: the unsorted select of the staged pipeline, or the pinned small-batch / wide call
    idx3, dist3, cnt3 = index.search_batched(q, K, o)
    kernel = index.last_kernel_ms()[1]
    if cl["pipeline"] == "Staged":
        assert kernel in STAGED_KERNELS and PC.final_select(ms, s.P, m, False) in ("select_rerank_kernel", "select_regs_kernel")
    else:
        assert kernel == {"Small": "small_scan_kernel", "Wide": "wide_scan_kernel"}[cl["pipeline"]]
    _same_rows(name + " plain", (idx3, dist3, cnt3), (idx, dist, cnt))


PARTITIONED_RUNS = [s.name for s in PC.SEARCHES if s.mode == "partitioned"]


@pytest.mark.parametrize("name", PARTITIONED_RUNS)
def test_partitioned_search_against_oracle(name):
    """A dim no code layout admits (65: one past a 64-dim chunk of the inline scoring), in Partitioned mode: the
    small-batch pipeline's tokens and rows against the oracle's, in its one-launch form."""
    s, kw, q, _, arr = _built(name)
    ms = PC.max_stream(np.diff(arr["leaf_off"].astype(np.int64)), s.P)
    cl = PC.classify(s.L, s.P, s.dim, s.nq, m=K, ms=ms, exact_scan=True)
    assert cl["pipeline"] == "Small" and cl["fused"] and cl["inline-chunks"] == "tail"
    index = hip.txh_create(**kw)
    index.enable_timing(True)
    o = hip.default_opts()
    o.partitions_to_search = s.P
    idx, dist, cnt, tok, tokd = _search_with_tokens(index, q, o, s.P)
    deep = -1
    for i in range(s.nq):
        ot, od = orc.partition(arr["centers"], q[i], s.P)
        assert np.array_equal(tok[i], ot) and np.array_equal(bits(tokd[i]), bits(od)), "%s q%d tokens" % (name, i)
        oi, od = orc.scann_search_partitioned(arr["centers"], arr["leaf_off"], arr["leaf_ids"], arr["data"], arr["stride"],
                                              hip.SQUARED_L2, q[i], s.P, K)
        assert cnt[i] == oi.size
        H.assert_topk_equal_up_to_ties(idx[i, :cnt[i]], dist[i, :cnt[i]], oi, od, what="%s q%d" % (name, i))
        deep = max(deep, _deepest_rank(s.L, ot, arr["assign"][oi]))
    assert deep >= s.P // 2, deep                      # final rows from leaves past the first wave's 64 ranks
    got = index.search_batched(q, K, o)
    assert index.last_kernel_ms()[1] == "small_scan_kernel"
    _same_rows(name + " plain", got, (idx, dist, cnt))
    # the same index through the staged kernels (a batch past the small pipeline's 16 queries)
    q33 = np.concatenate([q, PC.queries(name + "+", 25, s.dim, "uniform", arr["centers"])])
    idx33, dist33, cnt33 = index.search_batched(q33, K, o)
    assert index.last_kernel_ms()[1] == "leaf_exact_scan_kernel"
    _same_rows(name + " staged", (idx33[:s.nq], dist33[:s.nq], cnt33[:s.nq]), (idx, dist, cnt))


# ---- c. sharded key bases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [s.name for s in PC.SHARDED])
def test_sharded_key_bases_at_scale(name):
    """Two leaf shards -> local stage on each -> merge == the single index, which equals the oracle.  The low word of
    every merge key a shard emits must be the candidate's position in the query's GLOBAL stream: the sizes of the
    leaves ranked before its leaf, all shards' rows counted, plus its place inside its leaf."""
    import ctypes as C
    import torch
    from scann_rust_amd import sharding
    s, kw, q, ix, arr = _built(name)
    world, m, nq, P = 2, s.ms[0], s.nq, s.P
    o = _opts(P, m)
    full = hip.txh_create(**kw)
    want_idx, want_dist, want_cnt = full.search_batched(q, K, o)
    oix = _oracle_view(s, ix, arr, m)
    for i in range(0, nq, 8):
        oi, od = orc.txh_search(oix, q[i], K)
        assert want_cnt[i] == oi.size
        H.assert_topk_equal_up_to_ties(want_idx[i, :oi.size], want_dist[i, :oi.size], oi, od, what="%s full q%d" % (name, i))

    Lh = hip.load()
    dev = torch.device("cuda", 0)
    sptr = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    qd = torch.from_numpy(q).to(dev)
    g_keys = torch.zeros((world, nq, m), dtype=torch.int64, device=dev)
    g_idx = torch.zeros((world, nq, m), dtype=torch.int32, device=dev)
    g_ex = torch.zeros((world, nq, m), dtype=torch.float32, device=dev)
    g_cnt = torch.zeros((world, nq), dtype=torch.int32, device=dev)
    shards = []
    for r in range(world):
        skw = sharding.shard_txh_index(ix, arr["data"], arr["stride"], r, world)
        assert not np.array_equal(np.diff(skw["leaf_offsets"].astype(np.int64)), skw["leaf_sizes_global"])
        sh = hip.txh_create(partitions_to_search=P, pre_reorder_multiplier=m / K, **skw)
        shards.append(sh)
        hip.check(Lh.scann_hip_txh_search_local_device(
            sh.h, C.c_void_p(qd.data_ptr()), nq, s.dim, K, C.byref(o),
            C.c_void_p(g_keys[r].data_ptr()), C.c_void_p(g_idx[r].data_ptr()),
            C.c_void_p(g_ex[r].data_ptr()), C.c_void_p(g_cnt[r].data_ptr()), sptr))
        hip.check(Lh.scann_hip_index_last_device_status(sh.h, sptr))
    out_idx = torch.zeros((nq, K), dtype=torch.int32, device=dev)
    out_dist = torch.zeros((nq, K), dtype=torch.float32, device=dev)
    out_cnt = torch.zeros((nq,), dtype=torch.int32, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    hip.check(Lh.scann_hip_txh_merge_device(hip.context(0), world, nq, m, m, K, 0,
                                            C.c_void_p(g_keys.data_ptr()), C.c_void_p(g_idx.data_ptr()),
                                            C.c_void_p(g_ex.data_ptr()), C.c_void_p(g_cnt.data_ptr()),
                                            C.c_void_p(out_idx.data_ptr()), C.c_void_p(out_dist.data_ptr()),
                                            C.c_void_p(out_cnt.data_ptr()), C.c_void_p(status.data_ptr()), sptr))
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    # the key bases, from a model that knows only the global index
    keys = g_keys.cpu().numpy().view(np.uint64)
    kidx = g_idx.cpu().numpy().view(np.uint32)
    kcnt = g_cnt.cpu().numpy()
    leaf_off = ix["leaf_off"].astype(np.int64)
    sizes = np.diff(leaf_off)
    leaf_of_row = np.repeat(np.arange(s.L), sizes)                       # CSR row -> leaf
    csr_of = np.empty(leaf_of_row.size, np.int64)
    csr_of[ix["leaf_ids"]] = np.arange(leaf_of_row.size)                 # datapoint -> CSR row
    checked, deep = 0, -1
    for i in range(nq):
        tokens, _ = orc.partition(ix["centers"], q[i], P)
        base = np.zeros(s.L, np.int64)
        base[tokens] = np.cumsum(sizes[tokens]) - sizes[tokens]          # exclusive, in token order
        for r in range(world):
            ids = kidx[r, i, :kcnt[r, i]].astype(np.int64)
            rows_csr = csr_of[ids]
            leaf = leaf_of_row[rows_csr]
            assert np.isin(leaf, tokens).all()
            want = base[leaf] + (rows_csr - leaf_off[leaf])
            got = (keys[r, i, :kcnt[r, i]] & np.uint64(0xFFFFFFFF)).astype(np.int64)
            assert np.array_equal(got, want), "%s q%d shard %d: key bases" % (name, i, r)
            checked += ids.size
            deep = max(deep, _deepest_rank(s.L, tokens, leaf))
    assert checked >= nq * min(m, 20) and deep >= P * 3 // 4, (checked, deep)
    gi = out_idx.cpu().numpy().view(np.uint32)
    gd = out_dist.cpu().numpy()
    gc = out_cnt.cpu().numpy()
    assert np.array_equal(gc.astype(np.uint32), want_cnt)
    assert np.array_equal(gd.view(np.uint32), want_dist.view(np.uint32))
    assert np.array_equal(gi, want_idx)

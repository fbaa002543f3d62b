"""The exact re-rank behind the 8-bit row filter (txh.hip K8b) on the adversarial row families of
tests/helpers.py rerank_rows, each compared with the full re-rank, the staged path and the ORACLE.

A. single-GPU final stage: every family x every row store (int8 with a scale per row, int8 with one scale, FP8 E4M3) x
   both index kinds (flat hasher, tree) x (k, m) from (1, 8) to (10, 8192), batches of 24 queries.  The filtered rows
   must equal an unfiltered index's (SCANN_HIP_RERANK_I8=0) bit for bit, and the staged rows (final_sort_kernel) and
   the oracle's up to exact ties.  tests/rerank_filter_model.py predicts which queries rerank_short_kernel finishes
   itself and which fall back to final_topk_kernel.  Rows holding a NaN are compared with the full re-rank only (the
   reference's sort is not an order there).
B. sharded local stage with prefix-dominance pruning (ShortArgs::local_head), 2 and 3 ranks.
C. the small-batch and wide pipelines (exact re-rank without the filter) on the same rows."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

from oracle import pyoracle as orc
from scann_rust_amd import hip, sharding
from tests import helpers as H
from tests import rerank_filter_model as RM

pytestmark = pytest.mark.gpu

N, DIM, NQ, LEAVES, P = 9000, 64, 24, 12, 10
KNOBS = ("SCANN_HIP_RERANK_I8", "SCANN_HIP_RERANK_I8_MIN", "SCANN_HIP_RERANK_STORE", "SCANN_HIP_RERANK_UNIFORM",
         "SCANN_HIP_SMALL", "SCANN_HIP_WIDE", "SCANN_HIP_LOCAL_PRUNE")
STORES = {"i8-row": {"SCANN_HIP_RERANK_UNIFORM": "0"}, "i8-one": {"SCANN_HIP_RERANK_UNIFORM": "2"},
          "fp8": {"SCANN_HIP_RERANK_STORE": "fp8"}}
KM = ((1, 8), (10, 41), (10, 512), (10, 1024), (10, 1025), (64, 2048), (10, 2049), (10, 8192))
KM_TREE = ((1, 8), (10, 512), (10, 1025), (64, 2048), (10, 8192))
NAN_FAMILIES = ("nonfinite",)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@contextlib.contextmanager
def _knobs(**kv):
    """exactly these SCANN_HIP_* knobs set (the store knobs are read when an index is created)"""
    old = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Case:
    def __init__(self, family, kind, n=N, dim=DIM, nq=NQ):
        self.family, self.kind = family, kind
        d = H.rerank_rows(family, n, dim, nq, seed=5)
        self.rows, self.q, self.cb, self.codes = d["rows"], d["queries"], d["codebook"], d["codes"]
        self.data, self.stride = orc.to_strided(self.rows)
        self.dim = dim
        if kind == "ah":
            self.kw = H.ah_kwargs_from_codes(self.rows, self.cb, self.codes)
            self.oix = None
        else:
            self.oix, self.kw = H.txh_from_codes(self.rows, self.cb, self.codes, LEAVES, P, 3.0, seed=7,
                                                 use_residuals=False, tree_rows=d["base"])
        self.idx = {}

    def index(self, store):
        """'plain' (no row store: the full re-rank) or one of STORES, created once"""
        if store not in self.idx:
            env = {"SCANN_HIP_RERANK_I8": "0"} if store == "plain" else dict(STORES[store], SCANN_HIP_RERANK_I8="2")
            with _knobs(**env):
                self.idx[store] = hip.txh_create(**self.kw)
        return self.idx[store]

    def opts(self, m):
        o = hip.default_opts()
        o.pre_reorder_k = m
        if self.kind == "txh":
            o.partitions_to_search = P
        return o

    def oracle_check(self, q, k, m, got_idx, got_dist, ci, cd, what):
        if self.kind == "ah":
            H.check_ah_query(self.cb, self.codes, self.data, self.stride, self.dim, q, k, m, got_idx, got_dist, ci, cd,
                             what=what)
        else:
            oix = orc.TxhIndex(self.data, self.stride, self.dim, self.kw["centers"], self.kw["leaf_offsets"],
                               self.kw["leaf_ids"], self.cb, self.kw["codes"], use_residuals=False,
                               partitions_to_search=P, pre_reorder_multiplier=(m + 0.5) / k)
            assert orc.pre_reorder_k(k, oix.pre_reorder_multiplier) == m
            oi, od, otok, otokd, oci, ocd = orc.txh_search(oix, q, k, stages=True)
            assert ci.size == oci.size and np.array_equal(_bits(cd), _bits(ocd)), what + ": candidates"
            if sorted(ci.tolist()) == sorted(oci.tolist()):
                H.assert_topk_equal_up_to_ties(got_idx, got_dist, oi, od, what=what)
            else:
                ri, rd = orc.reorder(self.data, self.stride, self.dim, q, ci, k)
                H.assert_topk_equal_up_to_ties(got_idx, got_dist, ri, rd, what=what)


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(family, kind):
        if (family, kind) not in cache:
            cache[family, kind] = Case(family, kind)
        return cache[family, kind]

    yield get
    cache.clear()


def _equal_rows(a, b, what):
    assert np.array_equal(a[2], b[2]), what + ": counts"
    assert np.array_equal(_bits(a[1]), _bits(b[1])), what + ": distances"
    assert np.array_equal(a[0], b[0]), what + ": indices"


def _device_search(index, q, k, o):
    """scann_hip_search_batched_device on torch's current stream: (status, idx, dist, count)"""
    import torch
    dev = torch.device("cuda:0")
    L = hip.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    nq, dim = q.shape
    qd = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(dev)
    oi = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
    od = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    oc = torch.full((nq,), 7, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    hip.check(L.scann_hip_search_batched_device(index.h, p(qd), nq, dim, k, ctypes.byref(o), p(oi), p(od), p(oc), st))
    status = L.scann_hip_index_last_device_status(index.h, st)
    torch.cuda.synchronize()
    return status, oi.cpu().numpy().view(np.uint32), od.cpu().numpy(), oc.cpu().numpy().view(np.uint32)


# ---- A. single-GPU final stage ------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", list(STORES))
@pytest.mark.parametrize("kind", ["ah", "txh"])
@pytest.mark.parametrize("family", H.RERANK_FAMILIES)
def test_final_stage_equals_full_rerank(cases, family, kind, store, monkeypatch):
    c = cases(family, kind)
    plain, filt = c.index("plain"), c.index(store)
    monkeypatch.setenv("SCANN_HIP_RERANK_I8_MIN", "1")
    nan = family in NAN_FAMILIES
    paths = set()
    for k, m in (KM if kind == "ah" else KM_TREE):
        if family == "overflow-most" and k < 10:
            continue   # (fewer than k finite distances needs k above the 9 finite rows)
        what = "%s/%s/%s k=%d m=%d" % (family, kind, store, k, m)
        o = c.opts(m)
        got = filt.search_batched(c.q, k, o)
        want = plain.search_batched(c.q, k, o)
        _equal_rows(got, want, what)
        if store != "i8-row":
            continue
        # the staged path (final_sort_kernel over the whole list) and the oracle: once per (family, kind, k, m)
        sidx, sdist, scnt, (tok, tokd, ci, cd, cc) = plain.search_batched(c.q, k, c.opts(m), stages=True)
        st = RM.make_store(store, c.rows)
        for i in range(NQ):
            cnt = int(want[2][i])
            assert cnt == int(scnt[i]), what
            cand = ci[i, :cc[i]]
            acc = RM.approx_distances(st, c.q[i], cand)
            Lb, Ub = RM.bracket(acc, st.E[cand], c.dim)
            keep = RM.shortlist(Lb, Ub, k)
            paths.add((m, RM.final_path(int(keep.sum()), cand.size, k)))
            if family == "offset":
                assert keep.all(), what   # the model's shortlist is every candidate
            if nan:
                continue
            H.assert_topk_equal_up_to_ties(want[0][i, :cnt], want[1][i, :cnt], sidx[i, :cnt], sdist[i, :cnt],
                                           what="%s staged q%d" % (what, i))
            if family == "overflow-all":   # every exact distance +inf: the first k candidates, in key order
                assert np.isinf(want[1][i, :cnt]).all() and np.array_equal(want[0][i, :cnt], cand[:cnt]), what
            if i < 4:
                c.oracle_check(c.q[i], k, m, want[0][i, :cnt], want[1][i, :cnt], cand, cd[i, :cc[i]],
                               what="%s oracle q%d" % (what, i))
    if store == "i8-row" and family == "offset" and kind == "ah":
        assert (1024, "fast") in paths and (1025, "fallback") in paths and (8192, "fallback") in paths, paths
    if store == "i8-row" and family == "duplicates":
        assert (8192, "fast") in paths, paths
    if store == "i8-row":
        # once per family through the device entry: status Ok and the host's rows
        # (not the NaN query: its tables pass every point, which overflows the device's candidate lists -- the device
        # entry has no host retry, tests/test_gpu_txh_subspaces.py)
        o = c.opts(1025)
        qd = c.q[1:] if family == "nonfinite" else c.q
        status, di, dd, dc = _device_search(filt, qd, 10, o)
        assert status == 0, (family, kind, status)
        _equal_rows((di, dd, dc), plain.search_batched(qd, 10, o), "%s/%s device" % (family, kind))


@pytest.mark.parametrize("family,uniform", [("permuted", True), ("magnitudes", False)])
def test_default_knobs_large_index(family, uniform, monkeypatch):
    """65 536 rows, no knobs: the row store is built and the filter runs at m >= 512; equal magnitudes take the
    one-scale store, two magnitudes keep per-row scales (the model's rule); the rows equal the full re-rank's"""
    n = 65536
    c = Case(family, "ah", n=n)
    assert (RM.uniform_choice(RM.i8_store(c.rows)) is not None) == uniform
    with _knobs():
        filt = hip.txh_create(**c.kw)
    plain = c.index("plain")
    with _knobs():
        for k, m in ((10, 512), (10, 2049)):
            o = c.opts(m)
            _equal_rows(filt.search_batched(c.q, k, o), plain.search_batched(c.q, k, o), "%s m=%d" % (family, m))


@pytest.mark.parametrize("dim,family", [(16, "duplicates"), (48, "duplicates"), (144, "duplicates"),
                                        (1024, "permuted"), (40, "duplicates")])
def test_dims(dim, family, monkeypatch):
    """16 dims per lane pass: one partial pass (16, 48), a partial second 128-dim pass (144), eight passes (1024); a dim
    that is not a multiple of 16 builds no row store and takes the full re-rank"""
    c = Case(family, "ah", dim=dim)
    assert RM.filter_applies(dim) == (dim % 16 == 0)
    plain = c.index("plain")
    monkeypatch.setenv("SCANN_HIP_RERANK_I8_MIN", "1")
    for store in ("i8-row", "fp8"):
        filt = c.index(store)
        for k, m in ((10, 512), (10, 1025)):
            o = c.opts(m)
            _equal_rows(filt.search_batched(c.q, k, o), plain.search_batched(c.q, k, o), "dim %d %s m=%d" % (dim, store, m))
    o = c.opts(512)
    sidx, sdist, scnt, (tok, tokd, ci, cd, cc) = plain.search_batched(c.q[:4], 10, o, stages=True)
    for i in range(4):
        c.oracle_check(c.q[i], 10, 512, sidx[i, :scnt[i]], sdist[i, :scnt[i]], ci[i, :cc[i]], cd[i, :cc[i]],
                       what="dim %d q%d" % (dim, i))


# ---- B. sharded local stage ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("family", ["offset", "overflow-most", "duplicates", "permuted", "nonfinite"])
def test_sharded_local_stage_prunes(cases, family, world, monkeypatch):
    """merged rows = the single index's; the filled-in exact distances = the unpruned run's bit for bit; the first 256
    entries of every list are never pruned; every pruned entry is dominated by k of them in (exact, key) order"""
    import torch
    c = cases(family, "txh")
    k = 10
    ix = dict(centers=c.kw["centers"], leaf_off=c.kw["leaf_offsets"], leaf_ids=c.kw["leaf_ids"], codebook=c.cb,
              codes=c.kw["codes"], use_residuals=False)
    with _knobs(SCANN_HIP_RERANK_I8="2"):
        shards = [hip.txh_create(partitions_to_search=P, pre_reorder_multiplier=3.0,
                                 **sharding.shard_txh_index(ix, c.data, c.stride, r, world)) for r in range(world)]
    plain = c.index("plain")
    Lh = hip.load()
    dev = torch.device("cuda", 0)
    sptr = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    qs = c.q[1:] if family == "nonfinite" else c.q   # (the NaN query: see test_final_stage_equals_full_rerank)
    qd = torch.from_numpy(np.ascontiguousarray(qs)).to(dev)
    nq = qs.shape[0]
    for m in (513, 1500, 8192):
        o = c.opts(m)
        want_idx, want_dist, want_cnt = plain.search_batched(qs, k, o)
        runs = {}
        for prune in ("1", "0"):
            monkeypatch.setenv("SCANN_HIP_LOCAL_PRUNE", prune)
            g_keys = torch.zeros((world, nq, m), dtype=torch.int64, device=dev)
            g_idx = torch.zeros((world, nq, m), dtype=torch.int32, device=dev)
            g_ex = torch.zeros((world, nq, m), dtype=torch.float32, device=dev)
            g_cnt = torch.zeros((world, nq), dtype=torch.int32, device=dev)
            for r in range(world):
                hip.check(Lh.scann_hip_txh_search_local_device(
                    shards[r].h, ctypes.c_void_p(qd.data_ptr()), nq, c.dim, k, ctypes.byref(o),
                    ctypes.c_void_p(g_keys[r].data_ptr()), ctypes.c_void_p(g_idx[r].data_ptr()),
                    ctypes.c_void_p(g_ex[r].data_ptr()), ctypes.c_void_p(g_cnt[r].data_ptr()), sptr))
                hip.check(Lh.scann_hip_index_last_device_status(shards[r].h, sptr))
            out_idx = torch.zeros((nq, k), dtype=torch.int32, device=dev)
            out_dist = torch.zeros((nq, k), dtype=torch.float32, device=dev)
            out_cnt = torch.zeros((nq,), dtype=torch.int32, device=dev)
            status = torch.zeros((1,), dtype=torch.int32, device=dev)
            hip.check(Lh.scann_hip_txh_merge_device(
                hip.context(0), world, nq, m, m, k, 0, ctypes.c_void_p(g_keys.data_ptr()),
                ctypes.c_void_p(g_idx.data_ptr()), ctypes.c_void_p(g_ex.data_ptr()), ctypes.c_void_p(g_cnt.data_ptr()),
                ctypes.c_void_p(out_idx.data_ptr()), ctypes.c_void_p(out_dist.data_ptr()),
                ctypes.c_void_p(out_cnt.data_ptr()), ctypes.c_void_p(status.data_ptr()), sptr))
            torch.cuda.synchronize()
            what = "%s world %d m=%d prune=%s" % (family, world, m, prune)
            assert int(status.item()) == 0, what
            _equal_rows((out_idx.cpu().numpy().view(np.uint32), out_dist.cpu().numpy(),
                         out_cnt.cpu().numpy().astype(np.uint32)), (want_idx, want_dist, want_cnt), what)
            runs[prune] = (g_keys.cpu().numpy(), g_idx.cpu().numpy(), g_ex.cpu().numpy(), g_cnt.cpu().numpy())
        pk, pi, pe, pc = runs["1"]
        fk, fi, fe, fc = runs["0"]
        assert np.array_equal(pk, fk) and np.array_equal(pi, fi) and np.array_equal(pc, fc)
        valid = np.arange(m)[None, None, :] < pc[:, :, None]
        pruned = (_bits(pe) != _bits(fe)) & valid
        assert np.isinf(pe[pruned]).all()                      # a pruned entry travels as +inf
        assert np.array_equal(_bits(pe[valid & ~pruned]), _bits(fe[valid & ~pruned]))
        assert not pruned[:, :, :RM.LOCAL_HEAD].any()
        for r in range(world):
            for i in range(nq):
                n_ = int(pc[r, i])
                bad = RM.pruned_dominated(fe[r, i, :n_], fk[r, i, :n_].view(np.uint64), pruned[r, i, :n_], k)
                assert bad == [], "%s rank %d q%d: pruned entries %s are not dominated" % (family, r, i, bad[:5])


# ---- C. small-batch and wide pipelines ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ah", "txh"])
@pytest.mark.parametrize("family", H.RERANK_FAMILIES)
def test_small_and_wide_pipelines(cases, family, kind, monkeypatch):
    """1, 4 and 16 queries, SCANN_HIP_WIDE 0 and 2: the rows of the batched pipeline ((exact, key) order on +inf ties
    and duplicates)"""
    c = cases(family, kind)
    idx = c.index("i8-row")
    # (not the NaN query: the batched pipeline returns no rows for it, the small one -- and the oracle -- k rows of NaN)
    qs = c.q[1:] if family == "nonfinite" else c.q
    for k, m in ((10, 41), (10, 512)):
        o = c.opts(m)
        monkeypatch.setenv("SCANN_HIP_SMALL", "0")
        want = idx.search_batched(qs, k, o)
        monkeypatch.delenv("SCANN_HIP_SMALL")
        for nq in (1, 4, 16):
            for wide in ("0", "2"):
                monkeypatch.setenv("SCANN_HIP_WIDE", wide)
                got = idx.search_batched(qs[:nq], k, o)
                _equal_rows(got, tuple(a[:nq] for a in want), "%s/%s nq=%d wide=%s m=%d" % (family, kind, nq, wide, m))

"""Allow-list filters (search_with_filter(Some(allowlist)): opts.allow_bitmap / allow_bitmap_bits) on every tree scan,
every pipeline and every entry point, each compared with the ORACLE under the same filter.

The allow-set families of tests/helpers.py allow_family are computed from the index's leaves, the queries' probed
leaves, the threshold sample's positions, the wide pipeline's groups and the oracle's rankings; they include the word
and capacity edges (capacity 0, 1, 63, 64, 65, n - 1, n and > n with stray bits set past the capacity, a bitmap over a
prefix of the index).  References: the tree oracle with the bitmap masked to its capacity, and the flat hasher's oracle
on the allowed subset (skipped rows are never pushed).  Both index kinds are built from explicit random 4-bit codes;
the tree's leaf_ids are a real permutation, so that a CSR position tested in place of the datapoint index fails."""
import ctypes

import numpy as np
import pytest

from oracle import pyoracle as orc
from scann_rust_amd import hip, sharding, synth
from tests import helpers as H

pytestmark = pytest.mark.gpu

ABORTED = 10   # scann_hip.h SCANN_HIP_ABORTED
N, NQ, L, P, M, K = 80000, 64, 16, 6, 250, 10
FILTER_SCANS = ("gather", "resident", "dense32", "mfma16", "sp-lanes", "sp-words", "default")
HOST_FAMILIES = ("f3", "not-topm", "sampled", "cap65", "m+1", "one-leaf")
# Families correlated with the threshold sample (positions j * st of each leaf): "sampled" lets the sampled bound keep
# fewer than m points (Aborted); "unsampled" and one row per wide group (g | st) leave the sample without an allowed
# point, so there is no bound and a long stream's allowed points overflow the list sized for one (ResourceExhausted).
# The batched pipeline's device entry fails those queries (count 0, never a wrong row); the host entry repeats them.


def _batched_device_statuses(kind, fam):
    """the statuses the batched pipeline's device entry may report under `fam`: exactly Aborted for "sampled" (J allowed
    points pass the sampled bound, J < m: this pins the sample-plan mirror of tests/helpers.py to txh.h) and exactly
    ResourceExhausted for "unsampled" and for one row per wide group on the flat hasher (g = 8 divides st = 16: no
    allowed sample, no bound, 3/4 of the stream overflows the list); on the tree the wide groups follow query 0's
    stream, not the leaves' sample positions, so any of the three"""
    if fam == "sampled":
        return (ABORTED,)
    if fam == "unsampled" or (fam == "wide-one-per-group" and kind == "ah"):
        return (hip.RESOURCE_EXHAUSTED,)
    if fam == "wide-one-per-group":
        return (hip.OK, ABORTED, hip.RESOURCE_EXHAUSTED)
    return (hip.OK,)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Case:
    """one index kind at S subspaces: rows, explicit codes, the oracle view and the queries' oracle rankings"""

    def __init__(self, kind, S, n=N, nq=NQ, seed=0):
        self.kind, self.S, self.n = kind, S, n
        dim = 2 * S
        self.dim = dim
        rng = np.random.default_rng([seed, S, kind == "txh"])
        if kind == "ah":
            rows = synth.uniform_f32(n, dim, 700 + S)
            self.q = synth.uniform_f32(nq, dim, 800 + S)
        else:
            rows = synth.clustered_f32(n, dim, 900 + S, n_clusters=L)[0]
            self.q = synth.clustered_f32(nq, dim, 1000 + S, n_clusters=L)[0]
        cb = np.ascontiguousarray(rows[rng.choice(n, 16, replace=False)].reshape(16, S, 2).transpose(1, 0, 2),
                                  np.float32)
        codes = rng.integers(0, 16, (n, S), dtype=np.uint8)
        self.cb = cb
        if kind == "ah":
            self.kw = H.ah_kwargs_from_codes(rows, cb, codes)
            self.oix = None
            self.leaf_off, self.leaf_ids = np.array([0, n], np.int64), None
            self.tokens = np.zeros((nq, 1), np.int64)
            self.codes = self.kw["codes"]
        else:
            self.oix, self.kw = H.txh_from_codes(rows, cb, codes, L, P, M / K, seed=S)
            self.leaf_off, self.leaf_ids = self.kw["leaf_offsets"], self.kw["leaf_ids"]
            assert not np.array_equal(self.leaf_ids, np.arange(n)), "leaf_ids must be a real permutation"
            self.tokens = np.stack([orc.txh_search(self.oix, qi, K, stages=True)[2] for qi in self.q])
        self.data, self.stride = self.kw["data"], self.kw["stride"]
        P_ = 1 if kind == "ah" else P
        self.st = H.sample_plan(H.max_stream(self.leaf_off, P_), P_)[0]
        self.topk, self.topm = [], []
        for qi in self.q[:16]:
            if kind == "ah":
                self.topk.append(orc.ah_search_with_reordering(cb, self.codes, self.data, self.stride, qi, K, M)[0])
                self.topm.append(orc.ah_search(cb, self.codes, qi, M)[0])
            else:
                oi, _, _, _, oci, _ = orc.txh_search(self.oix, qi, K, stages=True)
                self.topk.append(oi)
                self.topm.append(oci)

    def family(self, name, seed=1):
        return H.allow_family(name, self.leaf_off, self.leaf_ids, self.tokens, K, M, self.st, seed, topk=self.topk,
                              topm=self.topm)

    def opts(self, m=M):
        o = hip.default_opts()
        o.pre_reorder_k = m
        if self.kind == "txh":
            o.partitions_to_search = P
        return o

    def check(self, q, words, cap, staged, qs, what, m=M, k=K):
        """every returned index allowed and below the capacity, unused slots empty, and the staged outputs of queries
        qs equal to the oracle's under the same filter, stage by stage"""
        idx, dist, cnt, (tok, tokd, ci, cd, cc) = staged
        allowed = H.allowed_ids(words, cap, self.n)
        ok = np.zeros(self.n + 1, bool)
        ok[allowed] = True
        for i in range(q.shape[0]):
            c = int(cnt[i])
            assert c <= k and np.all(idx[i, :c] < min(cap, self.n)), "%s q%d: index past the capacity" % (what, i)
            assert ok[idx[i, :c]].all(), "%s q%d: a disallowed index" % (what, i)
            assert np.all(idx[i, c:] == 0xFFFFFFFF) and np.all(np.isposinf(dist[i, c:])), "%s q%d: unused" % (what, i)
        for i in qs:
            w = "%s q%d" % (what, i)
            if self.kind == "txh":
                self.oix.allow = H.masked_words(words, cap, self.n)
                try:
                    H.check_txh_query(self.oix, q[i], k, idx[i, :cnt[i]], dist[i, :cnt[i]], tok[i], tokd[i],
                                      ci[i, :cc[i]], cd[i, :cc[i]], what=w)
                finally:
                    self.oix.allow = None
            elif allowed.size == 0:
                assert cnt[i] == 0 and cc[i] == 0, w
            else:
                sub_codes = np.ascontiguousarray(self.codes[allowed])
                sub_data = np.ascontiguousarray(self.data.reshape(self.n, self.stride)[allowed])
                pos = lambda x: np.searchsorted(allowed, np.asarray(x, np.int64)).astype(np.uint32)
                H.check_ah_query(self.cb, sub_codes, sub_data, self.stride, self.dim, q[i], k, m,
                                 pos(idx[i, :cnt[i]]), dist[i, :cnt[i]], pos(ci[i, :cc[i]]), cd[i, :cc[i]], what=w)


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(kind, S):
        if (kind, S) not in cache:
            cache[kind, S] = Case(kind, S)
        return cache[kind, S]

    yield get
    cache.clear()


def _same_rows(got, ref, what):
    """counts and distances bitwise, indices up to ties"""
    idx, dist, cnt = got
    assert np.array_equal(cnt, ref[2]), what + ": counts"
    assert np.array_equal(_bits(dist), _bits(ref[1])), what + ": distances"
    for i in range(idx.shape[0]):
        H.assert_topk_equal_up_to_ties(idx[i, :cnt[i]], dist[i, :cnt[i]], ref[0][i, :cnt[i]], ref[1][i, :cnt[i]],
                                       what="%s q%d" % (what, i))


# ---- 1. every scan x filter ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scan", FILTER_SCANS)
@pytest.mark.parametrize("S", [8, 16, 32, 48])
@pytest.mark.parametrize("kind", ["ah", "txh"])
def test_every_scan_under_filters(cases, kind, S, scan, monkeypatch):
    """64 queries (the batched pipeline, a sampled bound in force) under each forced scan and a set of filter families:
    the forced kernel ran on the first attempt (no retry), the staged outputs match the filtered oracle, the fast
    path's rows equal them, and the device entry returns Ok with the same rows -- also at a 1 % filter, where the
    integer prefilters' survivors would overflow their list if the filter did not bound them."""
    c = cases(kind, S)
    H.scan_env(monkeypatch, scan)
    index = hip.txh_create(**c.kw)
    index.enable_timing(True)
    o, q = c.opts(), c.q
    want = H.scan_kernel_name(scan, S)
    for fam in HOST_FAMILIES + ("f1",):
        words, cap = c.family(fam)
        what = "%s S%d %s %s" % (kind, S, scan, fam)
        # (the sample-aliased family makes the sampled bound keep fewer than m points: Aborted, and the host entry's
        # second attempt scans without a bound -- no prefilter: the resident kernel where forced, else the gather one)
        ran = (H.scan_kernel_name("resident" if scan == "resident" else "gather", S),) if fam == "sampled" else (want,)
        staged = index.search_batched(q, K, o, stages=True, allow=words, allow_bits=cap)
        assert index.last_kernel_ms()[1] in ran, what + ": " + index.last_kernel_ms()[1]
        c.check(q, words, cap, staged, range(0, NQ, 16) if fam != "f1" else (0,), what)
        fast = index.search_batched(q, K, o, allow=words, allow_bits=cap)
        assert index.last_kernel_ms()[1] in ran, what + " fast"
        _same_rows(fast, staged[:3], what + " fast")
        if fam in ("f1", "f3", "cap65"):
            status, di, dd, dc = H.device_search(index, q, K, o, allow=words, allow_bits=cap)
            assert status == hip.OK, "%s device: status %d" % (what, status)
            _same_rows((di, dd, dc), staged[:3], what + " device")


@pytest.mark.parametrize("fam", ["f3", "not-topm"])
def test_byte_codes_under_filters(fam, monkeypatch):
    """8-bit codes (K = 256) on the gather scan under a filter: the filtered oracle's rows"""
    n, dim, S = 20000, 32, 8
    H.scan_env(monkeypatch, "gather")
    rows = synth.uniform_f32(n, dim, 1100)
    rng = np.random.default_rng(11)
    cb = np.ascontiguousarray(rows[rng.choice(n, 256, replace=False)].reshape(256, S, dim // S).transpose(1, 0, 2),
                              np.float32)
    codes = rng.integers(0, 256, (n, S), dtype=np.uint8)
    kw = H.ah_kwargs_from_codes(rows, cb, codes)
    index = hip.txh_create(**kw)
    index.enable_timing(True)
    q = synth.uniform_f32(32, dim, 1101)
    topm = [orc.ah_search(cb, codes, qi, 200)[0] for qi in q]
    words, cap = H.allow_family(fam, [0, n], None, np.zeros((32, 1)), K, 200, H.sample_stride(n), 3, topm=topm)
    o = hip.default_opts()
    o.pre_reorder_k = 200
    idx, dist, cnt = index.search_batched(q, K, o, allow=words, allow_bits=cap)
    assert index.last_kernel_ms()[1] == "adc_scan_kernel"
    allowed = H.allowed_ids(words, cap, n)
    for i in range(0, 32, 4):
        oi, od = orc.ah_search_with_reordering(cb, np.ascontiguousarray(codes[allowed]),
                                               np.ascontiguousarray(kw["data"].reshape(n, kw["stride"])[allowed]),
                                               kw["stride"], q[i], K, 200)
        assert cnt[i] == oi.size
        H.assert_topk_equal_up_to_ties(idx[i, :cnt[i]], dist[i, :cnt[i]], allowed[oi].astype(np.uint32), od,
                                       what="%s q%d" % (fam, i))


# ---- 2. every pipeline x filter, both entries -------------------------------------------------------------------------
# name: (knobs, batch sizes it takes).  A filtered call is named by its batched scan, so the pipeline that ran is not
# observable; the knobs force it where plan_txh_search's limits hold, and these shapes hold them (<= 16 queries, m <= 1024,
# streams <= 262 144 points, <= 4096 leaves; the wide pipeline <= 4 queries).  The one-launch form needs P = 1 (the flat
# hasher) and nq x ceil(n / 1024) <= 512 workgroups: 1 and 3 queries at 80 000 rows; the tree takes only the others.
PIPELINES = {
    "staged": ({"SCANN_HIP_SMALL": "0"}, (1, 3, 16, 17)),
    "small": ({"SCANN_HIP_WIDE": "0", "SCANN_HIP_FUSED": "0"}, (1, 3, 16)),
    "fused": ({"SCANN_HIP_WIDE": "0", "SCANN_HIP_FUSED": "1"}, (1, 3)),
    "wide": ({"SCANN_HIP_WIDE": "2"}, (1, 3)),
}
assert max(PIPELINES["fused"][1]) * -(-N // 1024) <= 512


@pytest.mark.parametrize("fam", H.FILTER_FAMILIES)
@pytest.mark.parametrize("kind", ["ah", "txh"])
def test_every_pipeline_under_filters(cases, kind, fam, monkeypatch):
    """Each filter family through the staged (64 queries: checked against the oracle), small three-launch, small
    one-launch and wide pipelines at 1, 3, 16 and 17 queries, on the host and the device entry: the rows of the 64-query
    batch for the same queries.  The device entry returns Ok -- except on the staged pipeline for the families aliased
    with the threshold sample, where Aborted / ResourceExhausted with count 0 for the failed queries is allowed."""
    c = cases(kind, 16)
    H.scan_env(monkeypatch, "default")
    index = hip.txh_create(**c.kw)
    o, q = c.opts(), c.q
    words, cap = c.family(fam)
    monkeypatch.setenv("SCANN_HIP_SMALL", "0")
    staged = index.search_batched(q, K, o, stages=True, allow=words, allow_bits=cap)
    c.check(q, words, cap, staged, (0, 1, 2, 17, 40, 63), "%s %s staged" % (kind, fam))
    ref = staged[:3]
    status, di, dd, dc = H.device_search(index, q, K, o, allow=words, allow_bits=cap)
    _device_rows(status, (di, dd, dc), ref, _batched_device_statuses(kind, fam), "%s %s staged device nq64" % (kind, fam))
    for name, (knobs, sizes) in PIPELINES.items():
        if name == "fused" and kind == "txh":
            continue   # (P = 6: the tree never takes the one-launch form)
        H.scan_env(monkeypatch, "default")
        for kn, v in knobs.items():
            monkeypatch.setenv(kn, v)
        for nq in sizes:
            lo = 40 if nq == 1 else 0
            sub = tuple(x[lo:lo + nq] for x in ref)
            what = "%s %s %s nq%d" % (kind, fam, name, nq)
            _same_rows(index.search_batched(q[lo:lo + nq], K, o, allow=words, allow_bits=cap), sub, what + " host")
            status, di, dd, dc = H.device_search(index, q[lo:lo + nq], K, o, allow=words, allow_bits=cap)
            _device_rows(status, (di, dd, dc), sub,
                         _batched_device_statuses(kind, fam) if name == "staged" or nq > 16 else (hip.OK,), what + " device")


def _device_rows(status, got, ref, statuses, what):
    """the device entry's status is one of `statuses`; on a failure the failed queries have count 0 and the others
    the host's rows"""
    di, dd, dc = got
    assert status in statuses, "%s: status %d, expected one of %s" % (what, status, statuses)
    if status != hip.OK:
        failed = dc == 0
        assert failed.any(), what + ": a failure status without a failed query"
        ok = ~failed
        _same_rows((di[ok], dd[ok], dc[ok]), tuple(x[ok] for x in ref), what)
        return
    _same_rows(got, ref, what)


# ---- 3. thresholds --------------------------------------------------------------------------------------------------
# threshold_tail_kernel takes a bound of rank J <= 384 over a sample of more than 4096 points: the flat hasher's
# (scap 5004); the tree's 6 of 16 leaves sample fewer, so THR_TAIL=1 would repeat THR_TAIL=0 there
THR_KNOBS = [("ah", ("SCANN_HIP_THR_TAIL", "0")), ("ah", ("SCANN_HIP_THR_TAIL", "1")), ("ah", ("SCANN_HIP_THR_TIES", "0")),
             ("txh", ("SCANN_HIP_THR_TAIL", "0")), ("txh", ("SCANN_HIP_THR_TIES", "0"))]


@pytest.mark.parametrize("fam", ["f10", "f1", "sampled", "unsampled", "not-topm"])
@pytest.mark.parametrize("kind,knob", THR_KNOBS)
def test_thresholds_under_filters(cases, kind, fam, knob, monkeypatch):
    """J < m (a statistical bound) on the batched pipeline under each bound-selection knob: the host entry returns the
    filtered oracle's rows; the device entry Ok with them, or (sample-aliased families) a failure with count 0."""
    c = cases(kind, 16)
    st = c.st
    assert H.sample_rank(M, st) < M
    if kind == "ah":
        assert H.sample_rank(M, st) <= 384 and H.sample_plan(N, 1)[1] > 4096   # (the tail select bites)
    H.scan_env(monkeypatch, "default")
    monkeypatch.setenv(*knob)
    index = hip.txh_create(**c.kw)
    o, q = c.opts(), c.q
    words, cap = c.family(fam)
    staged = index.search_batched(q, K, o, stages=True, allow=words, allow_bits=cap)
    c.check(q, words, cap, staged, range(0, NQ, 9), "%s %s %s=%s" % (kind, fam, *knob))
    status, di, dd, dc = H.device_search(index, q, K, o, allow=words, allow_bits=cap)
    _device_rows(status, (di, dd, dc), staged[:3], _batched_device_statuses(kind, fam),
                 "%s %s %s=%s device" % (kind, fam, *knob))


# ---- 4. re-rank stores and the sharded local stage ------------------------------------------------------------------
@pytest.mark.parametrize("knobs", [{"SCANN_HIP_RERANK_I8": "2"}, {"SCANN_HIP_RERANK_I8": "2", "SCANN_HIP_RERANK_STORE": "fp8"}])
@pytest.mark.parametrize("kind", ["ah", "txh"])
def test_rerank_stores_under_filters(cases, kind, knobs, monkeypatch):
    """The int8 / FP8 re-rank row filter under allow-bitmaps: the rows of the f32 re-rank under the same filter"""
    c = cases(kind, 16)
    H.scan_env(monkeypatch, "default")
    plain = hip.txh_create(**c.kw)
    for kn, v in knobs.items():
        monkeypatch.setenv(kn, v)
    store = hip.txh_create(**c.kw)
    for fam in ("f10", "not-topk", "m+1", "cap-n-1"):
        words, cap = c.family(fam)
        for m in (M, 1000):
            o = c.opts(m)
            want = plain.search_batched(c.q, K, o, allow=words, allow_bits=cap)
            _same_rows(store.search_batched(c.q, K, o, allow=words, allow_bits=cap), want, "%s %s m%d" % (kind, fam, m))


@pytest.mark.parametrize("fam", ["f10", "f1", "not-topk", "one-leaf", "cap-over"])
def test_sharded_local_stage_under_filters(cases, fam, monkeypatch):
    """Two leaf shards' local stages (the device bitmap indexed by datapoint) merged by txh_merge_device: the single
    filtered index's rows, with and without prefix-dominance pruning; pruning changes no key, index or count, and a
    pruned entry travels as +inf"""
    import torch
    c = cases("txh", 16)
    H.scan_env(monkeypatch, "default")
    world = 2
    ix = dict(centers=c.kw["centers"], leaf_off=c.kw["leaf_offsets"], leaf_ids=c.kw["leaf_ids"], codebook=c.cb,
              codes=c.kw["codes"], use_residuals=True)
    shards = [hip.txh_create(partitions_to_search=P, pre_reorder_multiplier=M / K,
                             **sharding.shard_txh_index(ix, c.data, c.stride, r, world)) for r in range(world)]
    plain = hip.txh_create(**c.kw)
    words, cap = c.family(fam)
    o = c.opts()
    want = plain.search_batched(c.q, K, o, allow=words, allow_bits=cap)
    Lh = hip.load()
    dev = torch.device("cuda", 0)
    sptr = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    qd = torch.from_numpy(np.ascontiguousarray(c.q)).to(dev)
    da = torch.from_numpy(np.ascontiguousarray(words, np.uint64).view(np.int64).copy()).to(dev)
    o.allow_bitmap = ctypes.cast(ctypes.c_void_p(da.data_ptr()), ctypes.POINTER(ctypes.c_uint64))
    o.allow_bitmap_bits = cap
    nq = c.q.shape[0]
    runs = {}
    for prune in ("1", "0"):
        monkeypatch.setenv("SCANN_HIP_LOCAL_PRUNE", prune)
        g_keys = torch.zeros((world, nq, M), dtype=torch.int64, device=dev)
        g_idx = torch.zeros((world, nq, M), dtype=torch.int32, device=dev)
        g_ex = torch.zeros((world, nq, M), dtype=torch.float32, device=dev)
        g_cnt = torch.zeros((world, nq), dtype=torch.int32, device=dev)
        for r in range(world):
            hip.check(Lh.scann_hip_txh_search_local_device(
                shards[r].h, ctypes.c_void_p(qd.data_ptr()), nq, c.dim, K, ctypes.byref(o),
                ctypes.c_void_p(g_keys[r].data_ptr()), ctypes.c_void_p(g_idx[r].data_ptr()),
                ctypes.c_void_p(g_ex[r].data_ptr()), ctypes.c_void_p(g_cnt[r].data_ptr()), sptr))
            assert Lh.scann_hip_index_last_device_status(shards[r].h, sptr) == hip.OK
        out_idx = torch.zeros((nq, K), dtype=torch.int32, device=dev)
        out_dist = torch.zeros((nq, K), dtype=torch.float32, device=dev)
        out_cnt = torch.zeros((nq,), dtype=torch.int32, device=dev)
        status = torch.zeros((1,), dtype=torch.int32, device=dev)
        hip.check(Lh.scann_hip_txh_merge_device(
            hip.context(0), world, nq, M, M, K, 0, ctypes.c_void_p(g_keys.data_ptr()),
            ctypes.c_void_p(g_idx.data_ptr()), ctypes.c_void_p(g_ex.data_ptr()), ctypes.c_void_p(g_cnt.data_ptr()),
            ctypes.c_void_p(out_idx.data_ptr()), ctypes.c_void_p(out_dist.data_ptr()),
            ctypes.c_void_p(out_cnt.data_ptr()), ctypes.c_void_p(status.data_ptr()), sptr))
        torch.cuda.synchronize()
        what = "%s prune=%s" % (fam, prune)
        assert int(status.item()) == 0, what
        _same_rows((out_idx.cpu().numpy().view(np.uint32), out_dist.cpu().numpy(),
                    out_cnt.cpu().numpy().astype(np.uint32)), want, what)
        runs[prune] = (g_keys.cpu().numpy(), g_idx.cpu().numpy(), g_ex.cpu().numpy(), g_cnt.cpu().numpy())
    pk, pi, pe, pc = runs["1"]
    fk, fi, fe, fc = runs["0"]
    assert np.array_equal(pk, fk) and np.array_equal(pi, fi) and np.array_equal(pc, fc)
    valid = np.arange(M)[None, None, :] < pc[:, :, None]
    pruned = (_bits(pe) != _bits(fe)) & valid
    assert np.isinf(pe[pruned]).all()
    ok = H.allowed_ids(words, cap, c.n)
    assert np.isin(pi[valid].astype(np.int64), ok).all(), "a disallowed local candidate"


# ---- 5. semantics ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ah", "txh"])
def test_capacity_zero_allows_nothing(cases, kind, monkeypatch):
    """capacity 0 (a word of stray bits): empty rows on a fresh handle, right after a filtered call, on the device
    entry and through every pipeline"""
    c = cases(kind, 16)
    H.scan_env(monkeypatch, "default")
    o = c.opts()
    ones = np.full(1, np.uint64(0xFFFFFFFFFFFFFFFF))

    def empty(r, what):
        idx, dist, cnt = r
        assert np.all(cnt == 0), what
        assert np.all(idx == 0xFFFFFFFF) and np.all(np.isposinf(dist)), what

    for nq in (64, 3, 1):
        empty(hip.txh_create(**c.kw).search_batched(c.q[:nq], K, o, allow=ones, allow_bits=0), "fresh nq%d" % nq)
    index = hip.txh_create(**c.kw)
    words, cap = c.family("f10")
    for nq in (64, 3, 1):
        index.search_batched(c.q[:nq], K, o, allow=words, allow_bits=cap)
        empty(index.search_batched(c.q[:nq], K, o, allow=ones, allow_bits=0), "after a filter nq%d" % nq)
        status, di, dd, dc = H.device_search(index, c.q[:nq], K, o, allow=ones, allow_bits=0)
        assert status == hip.OK
        empty((di, dd, dc), "device nq%d" % nq)


@pytest.mark.parametrize("kind", ["ah", "txh"])
def test_filter_does_not_stick(cases, kind, monkeypatch):
    """after filtered calls (host and device), an unfiltered call equals a fresh handle's; mixed k with a filter
    equals the per-k calls"""
    c = cases(kind, 16)
    H.scan_env(monkeypatch, "default")
    o = c.opts()
    fresh = hip.txh_create(**c.kw)
    index = hip.txh_create(**c.kw)
    words, cap = c.family("f3")
    for nq in (64, 3):
        want = fresh.search_batched(c.q[:nq], K, o)
        index.search_batched(c.q[:nq], K, o, allow=words, allow_bits=cap)
        _same_rows(index.search_batched(c.q[:nq], K, o), want, "host nq%d" % nq)
        H.device_search(index, c.q[:nq], K, o, allow=words, allow_bits=cap)
        status, di, dd, dc = H.device_search(index, c.q[:nq], K, o)
        assert status == hip.OK
        _same_rows((di, dd, dc), want, "device nq%d" % nq)
    ks = np.array([1, 10, 5, 10, 1, 7] * 4, np.uint32)
    q = c.q[:ks.size]
    o.pre_reorder_k = 0   # (m from the multiplier: per k)
    idx, dist, cnt = index.search_batched_with_params(q, ks, o, allow=words, allow_bits=cap)
    for k in np.unique(ks):
        sel = np.flatnonzero(ks == k)
        wi, wd, wc = index.search_batched(q[sel], int(k), o, allow=words, allow_bits=cap)
        _same_rows((idx[sel, :k], dist[sel, :k], cnt[sel]), (wi, wd, wc), "params k%d" % k)
        assert np.all(idx[sel, k:] == 0xFFFFFFFF)


def test_exact_leaf_scan_rejects_filters(cases):
    """SearchMode::Partitioned (no codebook): a filter is Unimplemented on both entries"""
    c = cases("txh", 16)
    kw = {k_: v for k_, v in c.kw.items() if k_ not in ("use_residuals", "codes_packed4")}
    kw.update(codebook=None, codes=None)
    index = hip.txh_create(**kw)
    o = hip.default_opts()
    words, cap = c.family("f10")
    with pytest.raises(hip.ScannError) as e:
        index.search_batched(c.q[:8], K, o, allow=words, allow_bits=cap)
    assert e.value.code == hip.UNIMPLEMENTED
    with pytest.raises(hip.ScannError) as e:
        H.device_search(index, c.q[:8], K, o, allow=words, allow_bits=cap)
    assert e.value.code == hip.UNIMPLEMENTED


# ---- 6. headline size -----------------------------------------------------------------------------------------------
def test_headline_flat_hasher_under_a_filter(monkeypatch):
    """1M x 128 flat hasher (S = 32), 1024 queries, m = 5000, a uniform 5 % filter on the default path: the host entry
    takes the sparse prefilter without a retry, the device entry returns Ok with the host's rows, and sampled queries
    equal the oracle on the allowed subset"""
    n, dim, S, nq, m = 1 << 20, 128, 32, 1024, 5000
    H.scan_env(monkeypatch, "default")
    rng = np.random.default_rng(5)
    rows = synth.uniform_f32(n, dim, 1200)
    cb = np.ascontiguousarray(rows[rng.choice(n, 16, replace=False)].reshape(16, S, dim // S).transpose(1, 0, 2),
                              np.float32)
    codes = rng.integers(0, 16, (n, S), dtype=np.uint8)
    kw = H.ah_kwargs_from_codes(rows, cb, codes)
    del rows
    index = hip.txh_create(**kw)
    index.enable_timing(True)
    q = synth.uniform_f32(nq, dim, 1201)
    words, cap = H.words_of(np.flatnonzero(rng.random(n) < 0.05), n)
    o = hip.default_opts()
    o.pre_reorder_k = m
    idx, dist, cnt = index.search_batched(q, K, o, allow=words, allow_bits=cap)
    assert index.last_kernel_ms()[1] == "adc_smfmac_kernel"
    status, di, dd, dc = H.device_search(index, q, K, o, allow=words, allow_bits=cap)
    assert status == hip.OK, status
    _same_rows((di, dd, dc), (idx, dist, cnt), "device")
    allowed = H.allowed_ids(words, cap, n)
    sub_codes = np.ascontiguousarray(codes[allowed])
    sub_data = np.ascontiguousarray(kw["data"].reshape(n, kw["stride"])[allowed])
    for i in (0, 511, 1023):
        oi, od = orc.ah_search_with_reordering(cb, sub_codes, sub_data, kw["stride"], q[i], K, m)
        assert cnt[i] == oi.size
        H.assert_topk_equal_up_to_ties(idx[i, :cnt[i]], dist[i, :cnt[i]], allowed[oi].astype(np.uint32), od,
                                       what="q%d" % i)

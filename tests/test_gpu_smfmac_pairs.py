"""The sparse prefilter's two item shapes on flat hashers: 32 (query, leaf) pairs x 2048 points and 64 pairs x 1024 points
(adc_smfmac_body, CT = 1 / 2; SCANN_HIP_SP_PAIRS = 32 / 64 forces one where the 64-pair form is compiled: S <= 32,
lane-walk flush).  Both must produce the same survivor lists, so every output is compared with the ORACLE under each
form, and the two forms' candidate sets with each other.

Shapes are the smallest that reach every edge of an item, whether its range is 1024 or 2048 points:
  n = 4133   full ranges plus a 37-point range whose last tile has 5 live rows
  n = 6145   full ranges plus a 1-point range (a single odd tile)
  nq = 33    the second column tile has 1 pair        nq = 64   exactly one full item
  nq = 65    the second item has 1 pair               nq = 96   the last item's second column tile is all padding
  nq = 130   three items
pre_reorder_k = 250, so that a sampled bound is in force (4133 rows: sample stride 2, rank 214)."""
import numpy as np
import pytest

from oracle import pyoracle as orc
from scann_rust_amd import hip, synth
from tests import helpers as H
from tests.test_gpu_filters import Case

pytestmark = pytest.mark.gpu

ABORTED = 10   # scann_hip.h SCANN_HIP_ABORTED
NAME = "adc_smfmac_kernel"
K, M = 10, 250
AH_DIM = {8: 40, 16: 16, 24: 72, 32: 32}
POINTS, QUERIES = (4133, 6145), (33, 64, 65, 96, 130)
EDGES = [(n, nq, S) for n in POINTS for nq in QUERIES for S in (8, 32)] + [(4133, 65, 16), (4133, 65, 24)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _env(monkeypatch, pairs):
    """the sparse prefilter with the lane-walk flush, and the item shape (None: the planner's rule)"""
    H.scan_env(monkeypatch, "sp-lanes")
    monkeypatch.delenv("SCANN_HIP_SP_PAIRS", raising=False)
    if pairs is not None:
        monkeypatch.setenv("SCANN_HIP_SP_PAIRS", str(pairs))


def _opts():
    o = hip.default_opts()
    o.pre_reorder_k = M
    return o


def _same_rows(got, ref, what):
    idx, dist, cnt = got
    assert np.array_equal(cnt, ref[2]), what + ": counts"
    assert np.array_equal(_bits(dist), _bits(ref[1])), what + ": distances"
    for i in range(idx.shape[0]):
        H.assert_topk_equal_up_to_ties(idx[i, :cnt[i]], dist[i, :cnt[i]], ref[0][i, :cnt[i]], ref[1][i, :cnt[i]],
                                       what="%s q%d" % (what, i))


@pytest.fixture(scope="module")
def hashers():
    """trained flat hashers, built once per (n, S) and module; 130 queries each (a test takes the first nq)"""
    cache = {}

    def get(n, S):
        if (n, S) not in cache:
            dim = AH_DIM[S]
            rows, data, stride, ix, kw = H.make_ah_case(n, dim, S, seed=100 + S, pq_iters=3)
            cache[n, S] = dict(kw=kw, ix=ix, data=data, stride=stride, q=synth.uniform_f32(max(QUERIES), dim, 200 + S))
        return cache[n, S]

    yield get
    cache.clear()


def _check_oracle(c, q, staged, qs, what):
    idx, dist, cnt, (tok, tokd, ci, cd, cc) = staged
    for i in qs:
        H.check_ah_query(c["ix"]["codebook"], c["ix"]["codes"], c["data"], c["stride"], q.shape[1], q[i], K, M,
                         idx[i, :cnt[i]], dist[i, :cnt[i]], ci[i, :cc[i]], cd[i, :cc[i]], what="%s q%d" % (what, i))


# ---- item edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nq,S", EDGES)
def test_item_edges_under_both_forms(hashers, n, nq, S, monkeypatch):
    """Each form forced in turn: the sparse prefilter ran, the staged outputs (candidate lists and final rows) of every
    query match the oracle -- distances bitwise, indices up to ties -- and the fast path's rows equal the staged rows;
    the two forms' candidate sets are equal per query."""
    c = hashers(n, S)
    q, o = c["q"][:nq], _opts()
    cands = {}
    for pairs in (64, 32):
        what = "n%d nq%d S%d pairs%d" % (n, nq, S, pairs)
        _env(monkeypatch, pairs)
        index = hip.txh_create(**c["kw"])
        index.enable_timing(True)
        staged = index.search_batched(q, K, o, stages=True)
        assert index.last_kernel_ms()[1] == NAME, what
        _check_oracle(c, q, staged, range(nq), what)
        fast = index.search_batched(q, K, o)
        assert index.last_kernel_ms()[1] == NAME, what + " fast"
        _same_rows(fast, staged[:3], what + " fast")
        ci, cc = staged[3][2], staged[3][4]
        cands[pairs] = [np.sort(ci[i, :cc[i]]) for i in range(nq)]
    for i in range(nq):
        assert np.array_equal(cands[64][i], cands[32][i]), "n%d nq%d S%d q%d: candidate sets differ" % (n, nq, S, i)


# ---- allow-lists --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def filtered():
    c = Case("ah", 32, n=4133, nq=65)
    yield c


def test_shared_allow_list(filtered, monkeypatch):
    """One bitmap for the batch that allows about half of the points, 64-pair items: every returned index is allowed, and
    every query's staged outputs equal the oracle's over the allowed rows."""
    c = filtered
    words, cap = c.family("f50")
    _env(monkeypatch, 64)
    index = hip.txh_create(**c.kw)
    index.enable_timing(True)
    o = c.opts()
    staged = index.search_batched(c.q, K, o, stages=True, allow=words, allow_bits=cap)
    assert index.last_kernel_ms()[1] == NAME
    c.check(c.q, words, cap, staged, range(c.q.shape[0]), "shared f50")
    fast = index.search_batched(c.q, K, o, allow=words, allow_bits=cap)
    assert index.last_kernel_ms()[1] == NAME
    _same_rows(fast, staged[:3], "shared f50 fast")


def test_one_allow_list_per_query(filtered, monkeypatch):
    """One bitmap per query (allow_bitmap_stride), each a different random half of the points: a lane that filtered its
    words with another pair's bitmap -- the other column tile's, query 0's -- would return a disallowed row."""
    c = filtered
    nq = c.q.shape[0]
    block = np.stack([c.family("f50", seed=100 + i)[0] for i in range(nq)])
    assert len({b.tobytes() for b in block}) == nq
    _env(monkeypatch, 64)
    index = hip.txh_create(**c.kw)
    index.enable_timing(True)
    o = c.opts()
    staged = index.search_batched(c.q, K, o, stages=True, allow=block, allow_bits=c.n)
    assert index.last_kernel_ms()[1] == NAME
    idx, dist, cnt, (tok, tokd, ci, cd, cc) = staged
    for i in range(nq):
        s = slice(i, i + 1)
        c.check(c.q[s], block[i], c.n, (idx[s], dist[s], cnt[s], (tok[s], tokd[s], ci[s], cd[s], cc[s])), (0,),
                "per-query f50 q%d" % i)
    fast = index.search_batched(c.q, K, o, allow=block, allow_bits=c.n)
    assert index.last_kernel_ms()[1] == NAME
    _same_rows(fast, staged[:3], "per-query f50 fast")


# ---- list overflow ------------------------------------------------------------------------------------------------
def test_one_code_overflows_the_lists_of_64_pair_items(monkeypatch):
    """adversarial_pq "one-code" (every point ties at the bound, so every point passes): the survivors outnumber the
    prefilter's lists.  Device entry: Ok with the host's rows, or a failure status with count 0 for the failed queries;
    host entry: the retry (no bound, the gather scan) returns the oracle's rows.  The contract of
    tests/test_gpu_txh_subspaces.py test_one_code_overflows_the_candidate_lists."""
    n, dim, S, nq = 60000, 64, 32, 65
    cb, codes, rows, q = H.adversarial_pq("one-code", n, dim, S, nq, seed=S)
    kw = H.ah_kwargs_from_codes(rows, cb, codes)
    _env(monkeypatch, 64)
    index = hip.txh_create(**kw)
    index.enable_timing(True)
    o = _opts()
    status, di, dd, dc = H.device_search(index, q, K, o)
    assert index.last_kernel_ms()[1] == NAME
    assert status in (hip.OK, hip.RESOURCE_EXHAUSTED, ABORTED), status
    staged = index.search_batched(q, K, o, stages=True)
    assert index.last_kernel_ms()[1] == (NAME if status == hip.OK else "adc_scan_kernel")
    c = dict(ix=dict(codebook=cb, codes=kw["codes"]), data=kw["data"], stride=kw["stride"])
    _check_oracle(c, q, staged, (0, 31, 32, 63, 64), "one-code")
    idx, dist, cnt = index.search_batched(q, K, o)
    _same_rows((idx, dist, cnt), staged[:3], "one-code fast")
    failed = dc == 0
    if status == hip.OK:
        assert not failed.any(), "count 0 under status Ok"
    else:
        assert failed.any(), "a failure status without a failed query"
    ok = ~failed
    assert np.array_equal(dc[ok], cnt[ok]), "device counts"
    assert np.array_equal(_bits(dd[ok]), _bits(dist[ok])), "device distances"
    for i in np.flatnonzero(ok):
        H.assert_topk_equal_up_to_ties(di[i, :cnt[i]], dd[i, :cnt[i]], idx[i, :cnt[i]], dist[i, :cnt[i]],
                                       what="one-code device q%d" % i)


# ---- the planner's rule -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hasher60k():
    dim, S = 32, 32
    rows, data, stride, ix, kw = H.make_ah_case(60000, dim, S, seed=100 + S, pq_iters=3)
    yield dict(kw=kw, ix=ix, data=data, stride=stride, q=synth.uniform_f32(256, dim, 200 + S))


@pytest.mark.parametrize("nq", [64, 96, 256])
def test_default_rule_returns_the_oracles_rows(hasher60k, nq, monkeypatch):
    """No knob set: whichever form the planner picks (an even number of 32-pair tiles, an odd one, a batch past the
    rule's query count), the sparse prefilter runs and the rows match the oracle.  (Which form ran is not visible from
    outside: the plan has no test hook.)"""
    c = hasher60k
    for name in H.SCAN_KNOBS + ("SCANN_HIP_SP_PAIRS",):
        monkeypatch.delenv(name, raising=False)
    index = hip.txh_create(**c["kw"])
    index.enable_timing(True)
    q, o = c["q"][:nq], _opts()
    staged = index.search_batched(q, K, o, stages=True)
    assert index.last_kernel_ms()[1] == NAME
    _check_oracle(c, q, staged, sorted(set(range(0, nq, 7)) | {nq - 1}), "default nq%d" % nq)
    fast = index.search_batched(q, K, o)
    assert index.last_kernel_ms()[1] == NAME
    _same_rows(fast, staged[:3], "default nq%d fast" % nq)

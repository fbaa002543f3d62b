"""The bitmap form of the sparse prefilter's 64-pair items on flat hashers (SCANN_HIP_SP_BITMAP, default on): the scan
stores each item's survivor bitmap (adc_smfmac_bits_kernel64) and adc_refine_bits_kernel walks the rows, where
SCANN_HIP_SP_BITMAP=0 flushes the survivors into lists inside the scan.  Both must hand the select the same candidates,
so every output is compared with the ORACLE under each knob value, and the two values' outputs with each other.

Shapes as in tests/test_gpu_smfmac_pairs.py, whose helpers these tests use (items of 64 pairs x 1024 points):
  n = 4133   four full ranges plus a 37-point range whose last tile has 5 live rows (words past tile pair 0 are stale)
  n = 5120   whole ranges only
  n = 6145   six full ranges plus a 1-point range (a single odd tile: a word without a high half)
  nq = 33, 64, 65, 96, 130   a second column tile with 1 pair, one full item, a second item with 1 pair, a last item
             whose second column tile is all padding, three items
pre_reorder_k = 250, so that a sampled bound is in force."""
import numpy as np
import pytest

from oracle import pyoracle as orc
from scann_rust_amd import hip, synth
from tests import helpers as H
from tests import sp_bitmap_model as model
from tests.test_gpu_filters import Case
from tests.test_gpu_smfmac_pairs import (ABORTED, K, M, NAME, _bits, _check_oracle, _env, _opts, _same_rows,
                                         hashers)  # noqa: F401  (hashers: a module-scoped fixture)

pytestmark = pytest.mark.gpu

KNOB = "SCANN_HIP_SP_BITMAP"
POINTS, QUERIES = (4133, 5120, 6145), (33, 64, 65, 96, 130)
EDGES = [(n, nq, 32) for n in POINTS for nq in QUERIES] + [(4133, 65, S) for S in (8, 16, 24)]


def _knob(monkeypatch, value, pairs=64, scan="sp-lanes"):
    """the sparse prefilter with the lane-walk flush, 64-pair items, and the knob ("1" / "0"; None: unset)"""
    if scan == "sp-lanes":
        _env(monkeypatch, pairs)
    else:
        H.scan_env(monkeypatch, scan)
        monkeypatch.delenv("SCANN_HIP_SP_PAIRS", raising=False)
        if pairs is not None:
            monkeypatch.setenv("SCANN_HIP_SP_PAIRS", str(pairs))
    monkeypatch.delenv(KNOB, raising=False)
    if value is not None:
        monkeypatch.setenv(KNOB, value)


def _stream():
    import torch
    return torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream


def _cand_sets(staged, nq):
    ci, cc = staged[3][2], staged[3][4]
    return [np.sort(ci[i, :cc[i]]) for i in range(nq)]


def _same_staged(a, b, nq, what):
    """counts and distance bits of the final rows and of the candidate lists equal, candidate SETS equal"""
    _same_rows(a[:3], b[:3], what)
    assert np.array_equal(a[3][4], b[3][4]), what + ": candidate counts"
    sa, sb = _cand_sets(a, nq), _cand_sets(b, nq)
    for i in range(nq):
        assert np.array_equal(sa[i], sb[i]), "%s q%d: candidate sets differ" % (what, i)
        cc = a[3][4][i]
        assert np.array_equal(_bits(a[3][3][i, :cc]), _bits(b[3][3][i, :cc])), "%s q%d: candidate distances" % (what, i)


def _bitmap_bytes(n, nq):
    """size of the survivor bitmaps of a call: [nq rounded up to 64][ranges of 1024 points][32] u32"""
    return -(-nq // 64) * 64 * model.row_words(n) * 4


def _both(monkeypatch, kw, q, o, name=NAME, pairs=64, scan="sp-lanes", bitmap=True, **search):
    """{knob: staged outputs} on a fresh handle per knob value; the named kernel ran and the fast path's rows equal the
    staged ones under each.  Which form ran is read from the handle's workspace: under knob 1 it holds survivor
    bitmaps of exactly the call's size when the plan admits the form (bitmap), else none; under knob 0 none."""
    out = {}
    for knob in ("1", "0"):
        _knob(monkeypatch, knob, pairs, scan)
        index = hip.txh_create(**kw)
        index.enable_timing(True)
        staged = index.search_batched(q, K, o, stages=True, **search)
        assert index.last_kernel_ms()[1] == name, "knob %s: %s" % (knob, index.last_kernel_ms()[1])
        fast = index.search_batched(q, K, o, **search)
        assert index.last_kernel_ms()[1] == name, "knob %s fast" % knob
        _same_rows(fast, staged[:3], "knob %s fast" % knob)
        want = _bitmap_bytes(kw["n_rows"], q.shape[0]) if bitmap and knob == "1" else 0
        assert index.debug_survivor_bitmap_bytes() == want, "knob %s: the plan's form" % knob
        out[knob] = staged
    return out


# ---- item edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nq,S", EDGES)
def test_item_edges_under_both_knob_values(hashers, n, nq, S, monkeypatch):
    """Every query's staged outputs match the oracle under each knob value -- distances bitwise, indices up to ties --
    and the two values' counts, distance bits and candidate sets are equal."""
    c = hashers(n, S)
    q, o = c["q"][:nq], _opts()
    out = _both(monkeypatch, c["kw"], q, o)
    for knob in ("1", "0"):
        _check_oracle(c, q, out[knob], range(nq), "n%d nq%d S%d knob%s" % (n, nq, S, knob))
    _same_staged(out["1"], out["0"], nq, "n%d nq%d S%d" % (n, nq, S))


# ---- allow-lists --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def filtered():
    yield Case("ah", 32, n=4133, nq=65)


@pytest.mark.parametrize("fam", ["f50", "f1"])
def test_shared_allow_list(filtered, fam, monkeypatch):
    """One bitmap for the batch: about half of the points, and about 1 % of them (41 rows, fewer than m: no bound, every
    point passes the prefilter and the refine's allow test alone thins the full rows out).  Every returned index is
    allowed, the staged outputs equal the oracle's over the allowed rows, and the two knob values agree."""
    c = filtered
    words, cap = c.family(fam)
    nq = c.q.shape[0]
    out = _both(monkeypatch, c.kw, c.q, c.opts(), allow=words, allow_bits=cap)
    for knob in ("1", "0"):
        c.check(c.q, words, cap, out[knob], range(nq) if fam == "f50" else (0, 33, 64), "shared %s knob%s" % (fam, knob))
    _same_staged(out["1"], out["0"], nq, "shared " + fam)


def test_one_allow_list_per_query(filtered, monkeypatch):
    """One bitmap per query (allow_bitmap_stride), each a different random half of the points: a refine block that read
    another query's bitmap would return a disallowed row."""
    c = filtered
    nq = c.q.shape[0]
    block = np.stack([c.family("f50", seed=100 + i)[0] for i in range(nq)])
    assert len({b.tobytes() for b in block}) == nq
    out = _both(monkeypatch, c.kw, c.q, c.opts(), allow=block, allow_bits=c.n)
    idx, dist, cnt, (tok, tokd, ci, cd, cc) = out["1"]
    for i in range(nq):
        s = slice(i, i + 1)
        c.check(c.q[s], block[i], c.n, (idx[s], dist[s], cnt[s], (tok[s], tokd[s], ci[s], cd[s], cc[s])), (0,),
                "per-query f50 q%d" % i)
    _same_staged(out["1"], out["0"], nq, "per-query f50")


# ---- full rows, ties, unquantised tables ---------------------------------------------------------------------------
def test_one_code_overflows_the_candidate_lists(monkeypatch):
    """adversarial_pq "one-code" (every point ties at the bound, so every bit of every row is set): the refine's
    survivors outnumber the candidate lists.  The contract of tests/test_gpu_smfmac_pairs.py
    test_one_code_overflows_the_lists_of_64_pair_items: device entry Ok with the host's rows, or a failure status with
    count 0 for the failed queries; host entry: the retry (no bound, the gather scan) returns the oracle's rows."""
    n, dim, S, nq = 60000, 64, 32, 65
    cb, codes, rows, q = H.adversarial_pq("one-code", n, dim, S, nq, seed=S)
    kw = H.ah_kwargs_from_codes(rows, cb, codes)
    _knob(monkeypatch, "1")
    index = hip.txh_create(**kw)
    index.enable_timing(True)
    o = _opts()
    status, di, dd, dc = H.device_search(index, q, K, o)
    assert index.last_kernel_ms()[1] == NAME
    assert index.debug_survivor_bitmap_bytes(_stream()) == _bitmap_bytes(n, nq), "the bitmap form ran"
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


def _flat_case(n, dim, S, nq, seed, values=None):
    """explicit codes over a codebook of 16 rows cut into subspaces; values: draw codewords and queries from these"""
    rng = np.random.default_rng([seed, S])
    dsub = dim // S
    codes = rng.integers(0, 16, (n, S), dtype=np.uint8)
    if values is None:
        rows = synth.uniform_f32(n, dim, seed)
        cb = np.ascontiguousarray(rows[rng.choice(n, 16, replace=False)].reshape(16, S, dsub).transpose(1, 0, 2),
                                  np.float32)
        q = synth.uniform_f32(nq, dim, seed + 1)
    else:
        v = np.asarray(values, np.float32)
        cb = np.ascontiguousarray(rng.choice(v, (S, 16, dsub)), np.float32)
        rows = np.ascontiguousarray(cb[np.arange(S)[None, :], codes].reshape(n, dim), np.float32)
        q = rng.choice(v, (nq, dim))
    return cb, codes, rows, np.ascontiguousarray(q, np.float32)


def test_three_valued_code_rows_tie_at_the_bound(monkeypatch):
    """codewords, rows and queries in {-1, 0, 1}: exact tables and hundreds of points tied with the bound's distance --
    which of them pass is decided by the key's position half, the same under both knob values and in the oracle."""
    n, dim, S, nq = 6145, 64, 32, 65
    cb, codes, rows, q = _flat_case(n, dim, S, nq, 3100, values=(-1.0, 0.0, 1.0))
    t = orc.lut_from_query(cb, q[0]).reshape(S, 16)
    sums = t[np.arange(S)[None, :], codes].sum(1)
    assert np.unique(sums).size * 8 < sums.size, "ties are there"
    kw = H.ah_kwargs_from_codes(rows, cb, codes)
    out = _both(monkeypatch, kw, q, _opts())
    c = dict(ix=dict(codebook=cb, codes=kw["codes"]), data=kw["data"], stride=kw["stride"])
    for knob in ("1", "0"):
        _check_oracle(c, q, out[knob], range(0, nq, 8), "three-valued knob" + knob)
    _same_staged(out["1"], out["0"], nq, "three-valued")


def test_nan_query_and_overflowing_query(monkeypatch):
    """One query with a NaN component, one whose squares overflow to +inf: their tables are not quantised, every point
    passes the prefilter (full rows), and what the refine keeps of them decides the query's status.  The device
    entry's status and rows and the host entry's rows are those of SCANN_HIP_SP_BITMAP=0, for them and their neighbours
    in the item; the neighbours match the oracle."""
    n, dim, S, nq = 6145, 64, 32, 65
    cb, codes, rows, q = _flat_case(n, dim, S, nq, 3200)
    q[3, 5] = np.nan
    q[40, 9] = 1e20
    kw = H.ah_kwargs_from_codes(rows, cb, codes)
    got = {}
    for knob in ("1", "0"):
        _knob(monkeypatch, knob)
        index = hip.txh_create(**kw)
        index.enable_timing(True)
        dev = H.device_search(index, q, K, _opts())
        assert index.last_kernel_ms()[1] == NAME
        assert index.debug_survivor_bitmap_bytes(_stream()) == (_bitmap_bytes(n, nq) if knob == "1" else 0)
        got[knob] = (dev, index.search_batched(q, K, _opts(), stages=True))
    (s1, i1, d1, c1), (s0, i0, d0, c0) = got["1"][0], got["0"][0]
    assert s1 == s0, "device status %d vs %d" % (s1, s0)
    assert np.array_equal(c1, c0), "device counts"   # (count 0: a failed query, whose rows say nothing)
    live = np.flatnonzero(c1)
    assert {0, 2, 4, 39, 41, 64} <= set(live.tolist()), "the neighbours do not fail"
    _same_rows((i1[live], d1[live], c1[live]), (i0[live], d0[live], c0[live]), "nan / huge device")
    _same_rows(got["1"][1][:3], got["0"][1][:3], "nan / huge host")
    c = dict(ix=dict(codebook=cb, codes=kw["codes"]), data=kw["data"], stride=kw["stride"])
    _check_oracle(c, q, got["1"][1], (0, 2, 4, 39, 41, 64), "nan / huge neighbours")


# ---- runs of items ---------------------------------------------------------------------------------------------------
def test_a_wave_keeps_its_tables_over_a_run_of_items(monkeypatch):
    """More items than the scan has waves (251 ranges x 10 pair tiles = 2510 against 2048 on 256 CUs): a wave takes two
    entries of its queue at once and reloads its table fragments only when the pair tile changes.  251 ranges are no
    multiple of 8, so some runs cross from one pair tile to the next, some queues end on half a run, and the last pair
    tile holds a single pair."""
    n, dim, S, nq = 250 * 1024 + 37, 32, 16, 577
    cb, codes, rows, q = _flat_case(n, dim, S, nq, 3500)
    kw = H.ah_kwargs_from_codes(rows, cb, codes)
    out = _both(monkeypatch, kw, q, _opts())
    c = dict(ix=dict(codebook=cb, codes=kw["codes"]), data=kw["data"], stride=kw["stride"])
    _check_oracle(c, q, out["1"], (0, 63, 64, 320, 575, 576), "runs")
    _same_staged(out["1"], out["0"], nq, "runs")


# ---- rows of an earlier call ----------------------------------------------------------------------------------------
def test_no_row_survives_from_an_earlier_call(hashers, monkeypatch):
    """One handle at n = 6145 (its last range is one point): 130 queries, then 64 OTHER queries -- whose rows the first
    call filled with other queries' bits -- then a call that allows the last range's single point alone (no bound:
    the scan sets every bit of every row, and rows 64 .. 129 still hold the first call's).  Each call returns what a
    fresh handle returns, and the last one exactly that point."""
    n, S = 6145, 32
    c = hashers(n, S)
    o = _opts()
    qa, qb = c["q"], np.ascontiguousarray(c["q"][::-1][:64])
    words, cap = H.words_of([n - 1], n)
    calls = [("130", qa, {}), ("64 others", qb, {}), ("last point", qb, dict(allow=words, allow_bits=cap))]
    _knob(monkeypatch, "1")
    used = hip.txh_create(**c["kw"])
    for what, q, search in calls:
        if what != "130":   # (the largest call so far sized the bitmaps)
            assert used.debug_survivor_bitmap_bytes() == _bitmap_bytes(n, 130)
        got = used.search_batched(q, K, o, stages=True, **search)
        fresh = hip.txh_create(**c["kw"]).search_batched(q, K, o, stages=True, **search)
        _same_staged(got, fresh, q.shape[0], "used / fresh handle, " + what)
        if search:
            assert np.all(got[2] == 1) and np.all(got[0][:, 0] == n - 1), "the one allowed point"
        else:
            _check_oracle(c, q, got, range(0, q.shape[0], 9), what)


# ---- the plan -------------------------------------------------------------------------------------------------------
def test_tree_indexes_keep_the_lists(monkeypatch):
    """A tree index with the 64-pair form forced (lane-walk flush): no bitmap form there, whatever the knob says."""
    c = Case("txh", 32, n=20000, nq=65)
    out = _both(monkeypatch, c.kw, c.q, c.opts(), bitmap=False)
    for i in range(0, 65, 16):
        idx, dist, cnt, (tok, tokd, ci, cd, cc) = out["1"]
        H.check_txh_query(c.oix, c.q[i], K, idx[i, :cnt[i]], dist[i, :cnt[i]], tok[i], tokd[i], ci[i, :cc[i]],
                          cd[i, :cc[i]], what="tree q%d" % i)
    _same_staged(out["1"], out["0"], 65, "tree")


@pytest.mark.parametrize("S", [48, 64])
def test_wide_codes_keep_the_lists(S, monkeypatch):
    """S = 48 / 64 have no 64-pair form: the wide kernel and its flush under both knob values."""
    n, dim, nq = 4133, 2 * S, 65
    cb, codes, rows, q = _flat_case(n, dim, S, nq, 3300 + S)
    kw = H.ah_kwargs_from_codes(rows, cb, codes)
    out = _both(monkeypatch, kw, q, _opts(), name=H.sparse_kernel_name(S), bitmap=False)
    c = dict(ix=dict(codebook=cb, codes=kw["codes"]), data=kw["data"], stride=kw["stride"])
    _check_oracle(c, q, out["1"], range(0, nq, 16), "S%d" % S)
    _same_staged(out["1"], out["0"], nq, "S%d" % S)


def test_32_pair_items_keep_the_lists(hashers, monkeypatch):
    c = hashers(4133, 32)
    q = c["q"][:65]
    out = _both(monkeypatch, c["kw"], q, _opts(), pairs=32, bitmap=False)
    _check_oracle(c, q, out["1"], range(0, 65, 16), "pairs 32")
    _same_staged(out["1"], out["0"], 65, "pairs 32")


def test_a_bitmap_over_the_byte_limit_keeps_the_lists(monkeypatch):
    """4160 queries over 1 032 193 points: 4160 rows x 1009 ranges x 128 bytes = 512.4 MiB, past the plan's 512 MiB.
    Both knob values keep the lists (no bitmaps in the workspace); their rows are equal and a sample of them the
    oracle's."""
    n, dim, S, nq = 1032193, 8, 8, 4160
    rng = np.random.default_rng(3400)
    cb = rng.uniform(-1.0, 1.0, (S, 16, 1)).astype(np.float32)
    codes = rng.integers(0, 16, (n, S), dtype=np.uint8)
    rows = np.ascontiguousarray(cb[np.arange(S)[None, :], codes].reshape(n, dim), np.float32)
    rows += np.float32(0.05) * rng.uniform(-1.0, 1.0, (n, dim)).astype(np.float32)
    q = rng.uniform(-1.0, 1.0, (nq, dim)).astype(np.float32)
    kw = H.ah_kwargs_from_codes(rows, cb, codes)
    got = {}
    for knob in ("1", "0"):
        _knob(monkeypatch, knob)
        index = hip.txh_create(**kw)
        index.enable_timing(True)
        got[knob] = index.search_batched(q, K, _opts())
        assert index.last_kernel_ms()[1] == NAME
        assert index.debug_survivor_bitmap_bytes() == 0, "knob %s: lists" % knob
    assert _bitmap_bytes(n, nq) > 512 << 20 >= _bitmap_bytes(n - 1024, nq)
    _same_rows(got["1"], got["0"], "over the limit")
    idx, dist, cnt = got["1"]
    for i in (0, 2079, 4159):
        oi, od = orc.ah_search_with_reordering(cb, kw["codes"], kw["data"], kw["stride"], q[i], K, M)
        assert cnt[i] == oi.size
        H.assert_topk_equal_up_to_ties(idx[i, :cnt[i]], dist[i, :cnt[i]], oi, od, what="over the limit q%d" % i)

"""adc_refine_bits_kernel, stage by stage: the walk over a query's row of the survivor bitmap (one loop over a lane's four
words, the wave's queue filled in rounds), the scoring of the queued points side by side in a lane (neighbours in the
queue, valid next to invalid entries), and their places in the query's candidate list.  Flat hashers with the bitmap form
forced (the knobs and helpers of tests/test_gpu_sp_bitmap.py; the form is read from the handle's workspace); every
output is compared with the ORACLE -- distances bitwise, indices as sets per query up to ties, counts equal -- and with
the list form (SCANN_HIP_SP_BITMAP=0).  The tests pin what the kernel returns, not how: they pass on the kernel that
walked its words slot by slot as on the one that walks them in one loop.  The bitmap form takes batches from 33 queries
(smaller ones go to the gather scan), so 33 is the smallest batch here.

What the shapes reach (txh_prefilter.hip): a wave takes the row 256 words = 8 ranges of 1024 points at a time, a lane four
words = 128 consecutive points, word slot x of a lane the points with (p >> 2 & 1, p >> 6 & 1) = (x & 1, x >> 1); a wave's
queue holds 1024 points and is scored 256 at a time, four to a lane in two pairs, the rest (< 256) at the end.

The bitmaps are written down through the codes: codewords 0 and 1 of every subspace lie at the queries, the others far
away; the `near` points draw their codes from {0, 1}, so the bound of a small pre_reorder_k falls among them, the int8
prefilter (whose step is set by the far codewords) passes all of them and nothing else, and the f32 bound keeps some."""
import numpy as np
import pytest

from scann_rust_amd import hip
from tests import helpers as H
from tests.test_gpu_filters import Case
from tests.test_gpu_smfmac_pairs import ABORTED, K, NAME, _bits, _check_oracle, _same_rows
from tests.test_gpu_sp_bitmap import _bitmap_bytes, _both, _knob, _same_staged, _stream

pytestmark = pytest.mark.gpu

M_SMALL = 20   # pre_reorder_k of the written-down bitmaps: the sampled bound's rank is M_SMALL itself (helpers.sample_rank)


def _opts(m):
    o = hip.default_opts()
    o.pre_reorder_k = m
    return o


def _near_case(n, S, nq, near, seed):
    """flat hasher whose points `near` (bool [n]) alone pass the prefilter of every query"""
    rng = np.random.default_rng([seed, S])
    dim = 2 * S
    cb = rng.uniform(2.0, 3.0, (S, 16, 2)).astype(np.float32)
    cb[:, 0] = rng.uniform(-0.05, 0.05, (S, 2))
    cb[:, 1] = cb[:, 0] + rng.uniform(-0.02, 0.02, (S, 2)).astype(np.float32)
    codes = rng.integers(2, 16, (n, S)).astype(np.uint8)
    codes[near] = rng.integers(0, 2, (int(near.sum()), S)).astype(np.uint8)
    rows = cb[np.arange(S)[None, :], codes].reshape(n, dim)
    rows = np.ascontiguousarray(rows + np.float32(0.01) * rng.uniform(-1.0, 1.0, (n, dim)).astype(np.float32), np.float32)
    q = np.ascontiguousarray(rng.uniform(-0.1, 0.1, (nq, dim)), np.float32)
    assert H.sample_rank(M_SMALL, H.sample_plan(n, 1)[0]) == M_SMALL
    assert int(near[::H.sample_plan(n, 1)[0]].sum()) >= 2 * M_SMALL, "the sampled bound falls among the near points"
    kw = H.ah_kwargs_from_codes(rows, cb, codes)
    return dict(ix=dict(codebook=cb, codes=kw["codes"]), data=kw["data"], stride=kw["stride"], kw=kw, q=q)


def _check(monkeypatch, c, q, m, qs, what):
    out = _both(monkeypatch, c["kw"], q, _opts(m))
    idx, dist, cnt, (tok, tokd, ci, cd, cc) = out["1"]
    for i in qs:
        H.check_ah_query(c["ix"]["codebook"], c["ix"]["codes"], c["data"], c["stride"], q.shape[1], q[i], K, m,
                         idx[i, :cnt[i]], dist[i, :cnt[i]], ci[i, :cc[i]], cd[i, :cc[i]], what="%s q%d" % (what, i))
    _same_staged(out["1"], out["0"], q.shape[0], what)
    return out


def _device_then_host(monkeypatch, c, q, m, qs, what):
    """the bitmap form through the device entry (no retry) and the host entry: the form ran; status Ok with the host's
    rows, or a failure status with count 0 for the failed queries -- never a wrong row; the host entry's staged outputs
    match the oracle.  -> the device status"""
    _knob(monkeypatch, "1")
    index = hip.txh_create(**c["kw"])
    index.enable_timing(True)
    status, di, dd, dc = H.device_search(index, q, K, _opts(m))
    assert index.last_kernel_ms()[1] == NAME, what
    assert index.debug_survivor_bitmap_bytes(_stream()) == _bitmap_bytes(c["kw"]["n_rows"], q.shape[0]), what + ": the form"
    print("%s: device status %d" % (what, status))
    assert status in (hip.OK, hip.RESOURCE_EXHAUSTED, ABORTED), status
    staged = index.search_batched(q, K, _opts(m), stages=True)
    _check_oracle_m(c, q, staged, qs, m, what)
    idx, dist, cnt = staged[:3]
    failed = dc == 0
    assert failed.any() == (status != hip.OK), what + ": status and failed queries"
    ok = ~failed
    assert np.array_equal(dc[ok], cnt[ok]), what + ": device counts"
    assert np.array_equal(_bits(dd[ok]), _bits(dist[ok])), what + ": device distances"
    for i in np.flatnonzero(ok):
        H.assert_topk_equal_up_to_ties(di[i, :cnt[i]], dd[i, :cnt[i]], idx[i, :cnt[i]], dist[i, :cnt[i]],
                                       what="%s device q%d" % (what, i))
    return status


def _check_oracle_m(c, q, staged, qs, m, what):
    idx, dist, cnt, (tok, tokd, ci, cd, cc) = staged
    for i in qs:
        H.check_ah_query(c["ix"]["codebook"], c["ix"]["codes"], c["data"], c["stride"], q.shape[1], q[i], K, m,
                         idx[i, :cnt[i]], dist[i, :cnt[i]], ci[i, :cc[i]], cd[i, :cc[i]], what="%s q%d" % (what, i))


# ---- one lane carries everything -----------------------------------------------------------------------------------
def _lane_pattern(name, n):
    p = np.arange(n)
    if name == "full-lane":    # the four words of ONE lane full (range 1, points 256 .. 383), every other lane empty
        return (p >= 1024 + 256) & (p < 1024 + 384)
    if name == "two-lanes":    # a full lane next to a lane with its last word alone (and its single last bit's neighbours)
        return ((p >= 2048) & (p < 2048 + 128)) | ((p >= 2048 + 128) & (p < 2048 + 256) & ((p & 0x44) == 0x44))
    slot = {"slot0": 0x00, "slot3": 0x44}[name]   # every lane of ranges 1 and 2: that word slot full, the others empty
    return (p >= 1024) & (p < 3072) & ((p & 0x44) == slot)


@pytest.mark.parametrize("pattern,n,nq", [("full-lane", 4133, 33), ("full-lane", 8965, 65), ("two-lanes", 4133, 33),
                                           ("slot0", 4133, 65), ("slot3", 6145, 33)])
def test_one_lane_carries_everything(pattern, n, nq, monkeypatch):
    """128 consecutive survivors in one lane's words beside empty lanes (the walk's trips are that lane's alone, through
    all four of its words), and all survivors of a chunk in word slot 0 / in word slot 3 (three empty words behind / before
    the lane's bits)."""
    near = _lane_pattern(pattern, n)
    c = _near_case(n, 32, nq, near, seed=4100)
    out = _check(monkeypatch, c, c["q"], M_SMALL, range(nq), "%s n%d nq%d" % (pattern, n, nq))
    ci, cc = out["1"][3][2], out["1"][3][4]
    assert all(near[ci[i, :cc[i]]].all() for i in range(nq)), "a candidate outside the written-down bitmap"


# ---- rounds ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1025, 2049, 3073, 6145, 8965])
def test_full_rows_are_pushed_in_rounds(n, monkeypatch):
    """adversarial_pq "flat" (every subspace's codewords equal: tables without a range, every point passes the prefilter,
    every bit of every row is set): a chunk holds up to 8192 points, eight times the queue, and is pushed in rounds.  All
    distances tie and no bound thins them, so the refine keeps more than `cap` and must report it (the device entry:
    RESOURCE_EXHAUSTED, count 0, never a wrong row; the host entry's retry: the oracle's rows).  n = 1024 j + 1: the last
    range is one point, the last chunk's last lane holds a single bit; n = 8965: a second chunk, 773 points."""
    S, nq = 32, 33
    cb, codes, rows, q = H.adversarial_pq("flat", n, 64, S, nq, seed=4200 + n)
    kw = H.ah_kwargs_from_codes(rows, cb, codes)
    c = dict(ix=dict(codebook=cb, codes=kw["codes"]), data=kw["data"], stride=kw["stride"], kw=kw)
    if _device_then_host(monkeypatch, c, q, 250, (0, 16, 32), "flat n%d" % n) == hip.OK:
        _check(monkeypatch, c, q, 250, (0, 16, 32), "flat n%d" % n)


@pytest.mark.parametrize("n", [1025, 2049, 3073, 6145, 8965])
def test_full_rows_thinned_by_the_allow_list(n, monkeypatch):
    """Full rows whose points the refine itself ranks: fewer allowed points than pre_reorder_k, so there is no bound, every
    bit of every row is set, the chunks are pushed in rounds and the allow test alone thins them out -- status Ok, the
    oracle's rows.  n = 1024 j + 1: the one point of the last range is allowed and must be returned."""
    c = Case("ah", 32, n=n, nq=33)
    ids = np.concatenate([np.arange(5, n - 1, 37), [n - 1]])
    assert K < ids.size < 250
    words, cap = H.words_of(ids, c.n)
    out = _both(monkeypatch, c.kw, c.q, c.opts(), allow=words, allow_bits=cap)
    for knob in ("1", "0"):
        c.check(c.q, words, cap, out[knob], (0, 16, 32), "thinned n%d knob%s" % (n, knob))
    ci, cc = out["1"][3][2], out["1"][3][4]
    assert all(np.array_equal(np.sort(ci[i, :cc[i]]), ids) for i in range(33)), "every allowed point is a candidate"
    _same_staged(out["1"], out["0"], 33, "thinned n%d" % n)


# ---- pairs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", [(255, 1, 2, 257), (256, 257, 1, 2), (100, 0, 65, 129)])
def test_survivor_counts_per_wave(counts, monkeypatch):
    """Four chunks of 8192 points, one per wave, with exactly counts[w] survivors in wave w's chunk (spread over its
    lanes from a random start): 1 and 2 (one lane pair, half filled), 255 (the last pair of lane 63 straddles a valid and
    an invalid entry), 256 (one full pop, nothing left), 257 (a pop and a single point), 65 / 100 / 129 (a pair whose
    second point is invalid in some lanes)."""
    n, S, nq = 4 * 8192, 32, 33
    rng = np.random.default_rng([4300, sum(counts)])
    near = np.zeros(n, bool)
    for w, cnt in enumerate(counts):
        pick = rng.choice(8192, cnt, replace=False)
        if w == 0:   # (the sample takes every 8th point: 40 of chunk 0's survivors are sampled ones, so the bound falls there)
            other = np.flatnonzero(np.arange(8192) % 8 != 0)
            pick = np.concatenate([8 * rng.choice(1024, 2 * M_SMALL, replace=False), rng.choice(other, cnt - 2 * M_SMALL, replace=False)])
        near[w * 8192 + pick] = True
    assert [int(near[w * 8192:(w + 1) * 8192].sum()) for w in range(4)] == list(counts)
    c = _near_case(n, S, nq, near, seed=4300)
    out = _check(monkeypatch, c, c["q"], M_SMALL, range(0, nq, 4), "counts %s" % (counts,))
    ci, cc = out["1"][3][2], out["1"][3][4]
    assert all(near[ci[i, :cc[i]]].all() for i in range(nq))


def test_exact_counts_of_255_256_257(monkeypatch):
    """n <= 4096: the sample is every point, the bound the exact rank, and the near points are ONE code row: all of them tie
    and the bitmap of every query holds exactly `cnt` bits in wave 0's chunk, for cnt = 255, 256, 257 in turn."""
    S, nq, n = 32, 33, 4096
    for cnt in (255, 256, 257):
        near = np.zeros(n, bool)
        near[np.random.default_rng(cnt).choice(n, cnt, replace=False)] = True
        c = _near_case(n, S, nq, near, seed=4400 + cnt)
        codes = c["kw"]["codes"].copy()
        codes[near] = 0
        c["kw"] = dict(c["kw"], codes=codes)
        c["ix"] = dict(codebook=c["ix"]["codebook"], codes=codes)
        _check(monkeypatch, c, c["q"], M_SMALL, range(nq), "exactly %d" % cnt)


# ---- adversarial tables -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [8, 16, 24, 32])
@pytest.mark.parametrize("family", ["tiny", "huge", "nonfinite"])
def test_adversarial_tables(family, S, monkeypatch):
    """Table entries that are subnormal or zero ("tiny"), sums that overflow to +inf part of the way through the S terms
    ("huge"), and a +inf entry ("nonfinite"): each point's sum is the reference's sequential f32 sum wherever in a lane's
    group of points it sits.  (Squared-L2 tables hold no -0.0 and no -inf; NaN sums are the next test's.)"""
    n, nq = 4133, 33
    cb, codes, rows, q = H.adversarial_pq(family, n, 2 * S, S, nq, seed=4500 + S)
    kw = H.ah_kwargs_from_codes(rows, cb, codes)
    c = dict(ix=dict(codebook=cb, codes=kw["codes"]), data=kw["data"], stride=kw["stride"], kw=kw)
    if _device_then_host(monkeypatch, c, q, 250, range(0, nq, 4), "%s S%d" % (family, S)) == hip.OK:
        _check(monkeypatch, c, q, 250, range(0, nq, 4), "%s S%d" % (family, S))


@pytest.mark.parametrize("S", [8, 16, 24, 32])
def test_nan_and_inf_sums_next_to_finite_ones(S, monkeypatch):
    """A query with a NaN component (NaN table entries in one subspace: every sum NaN), one whose squares overflow (+inf
    entries), and one with -0.0 components, among ordinary queries of the same item: the device entry's status, counts and
    rows and the host entry's rows equal those of the list form; the ordinary queries match the oracle."""
    n, nq = 4133, 33
    cb, codes, rows, q = H.adversarial_pq("integers", n, 2 * S, S, nq, seed=4600 + S)
    q[3, 1] = np.nan
    q[20, 2] = 1e20
    q[7, :] = -0.0
    kw = H.ah_kwargs_from_codes(rows, cb, codes)
    got = {}
    for knob in ("1", "0"):
        _knob(monkeypatch, knob)
        index = hip.txh_create(**kw)
        index.enable_timing(True)
        dev = H.device_search(index, q, K, _opts(250))
        assert index.last_kernel_ms()[1] == NAME
        assert index.debug_survivor_bitmap_bytes(_stream()) == (_bitmap_bytes(n, nq) if knob == "1" else 0)
        got[knob] = (dev, index.search_batched(q, K, _opts(250), stages=True))
    (s1, i1, d1, c1), (s0, i0, d0, c0) = got["1"][0], got["0"][0]
    assert s1 == s0, "device status %d vs %d" % (s1, s0)
    assert np.array_equal(c1, c0), "device counts"
    live = np.flatnonzero(c1)
    assert {0, 2, 4, 7, 19, 21, 32} <= set(live.tolist()), "the neighbours do not fail"
    _same_rows((i1[live], d1[live], c1[live]), (i0[live], d0[live], c0[live]), "nan / inf device")
    _same_rows(got["1"][1][:3], got["0"][1][:3], "nan / inf host")
    c = dict(ix=dict(codebook=cb, codes=kw["codes"]), data=kw["data"], stride=kw["stride"])
    _check_oracle_m(c, q, got["1"][1], (0, 2, 4, 7, 19, 21, 32), 250, "nan / inf neighbours S%d" % S)


# ---- allow-lists and overflow ------------------------------------------------------------------------------------------
def _every_second_of_pairs(near):
    """allowed ids: the near points but for every second of them (in bitmap order neighbours share a lane's pair often
    enough), plus every far point"""
    ids = np.flatnonzero(near)
    drop = ids[1::2]
    ok = np.ones(near.size, bool)
    ok[drop] = False
    return np.flatnonzero(ok)


def test_allow_lists_clear_one_point_of_a_pair(monkeypatch):
    """515 survivors in wave 0's chunk; a shared allow-list clears every second of them, and per-query lists clear a
    different random half for every query: the cleared point of a lane's pair must neither be kept nor disturb the other."""
    n, S, nq = 4133, 32, 33
    near = np.zeros(n, bool)
    near[np.random.default_rng(4700).choice(4096, 515, replace=False)] = True
    c = _near_case(n, S, nq, near, seed=4700)
    sets = [_every_second_of_pairs(near)]
    rng = np.random.default_rng(4701)
    for i in range(nq):
        ok = np.ones(n, bool)
        ok[np.flatnonzero(near)[rng.random(515) < 0.5]] = False
        sets.append(np.flatnonzero(ok))
    shared, cap = H.words_of(sets[0], n)
    block = np.stack([H.words_of(s, n)[0] for s in sets[1:]])
    for what, search, allowed_of in (("shared", dict(allow=shared, allow_bits=cap), lambda i: sets[0]),
                                     ("per-query", dict(allow=block, allow_bits=n), lambda i: sets[1 + i])):
        out = _both(monkeypatch, c["kw"], c["q"], _opts(M_SMALL), **search)
        idx, dist, cnt, (tok, tokd, ci, cd, cc) = out["1"]
        for i in range(nq):
            allowed = allowed_of(i)
            pos = lambda x: np.searchsorted(allowed, np.asarray(x, np.int64)).astype(np.uint32)
            assert np.isin(ci[i, :cc[i]], allowed).all() and np.isin(idx[i, :cnt[i]], allowed).all(), what + ": disallowed"
            H.check_ah_query(c["ix"]["codebook"], np.ascontiguousarray(c["ix"]["codes"][allowed]),
                             np.ascontiguousarray(c["data"].reshape(n, c["stride"])[allowed]), c["stride"], 2 * S,
                             c["q"][i], K, M_SMALL, pos(idx[i, :cnt[i]]), dist[i, :cnt[i]], pos(ci[i, :cc[i]]),
                             cd[i, :cc[i]], what="%s q%d" % (what, i))
        _same_staged(out["1"], out["0"], nq, what)


def test_survivors_over_cap_report_and_the_retry_returns_the_oracles_rows(monkeypatch):
    """adversarial_pq "one-code" at 40 000 points: every point ties at the bound, the refine keeps more than `cap` of them.
    The device entry reports RESOURCE_EXHAUSTED with count 0 for the failed queries (never a wrong row); the host entry's
    retry returns the oracle's rows."""
    n, dim, S, nq = 40000, 64, 32, 33
    cb, codes, rows, q = H.adversarial_pq("one-code", n, dim, S, nq, seed=4800)
    kw = H.ah_kwargs_from_codes(rows, cb, codes)
    st, j, cap, _ = H.plan_caps(n, 1, 250)
    assert n - n // 1000 - 1 > cap, "the tie group outnumbers the candidate list"
    _knob(monkeypatch, "1")
    index = hip.txh_create(**kw)
    index.enable_timing(True)
    status, di, dd, dc = H.device_search(index, q, K, _opts(250))
    assert index.last_kernel_ms()[1] == NAME
    assert index.debug_survivor_bitmap_bytes(_stream()) == _bitmap_bytes(n, nq), "the bitmap form ran"
    assert status == hip.RESOURCE_EXHAUSTED, status
    assert (dc == 0).any(), "a failure status without a failed query"
    staged = index.search_batched(q, K, _opts(250), stages=True)
    c = dict(ix=dict(codebook=cb, codes=kw["codes"]), data=kw["data"], stride=kw["stride"])
    _check_oracle(c, q, staged, (0, 16, 32), "over cap")
    ok = dc != 0
    assert np.array_equal(dc[ok], staged[2][ok]), "device counts of the queries that did not fail"

"""GPU checks of the register-resident unsorted select (txh.hip K7r, SCANN_HIP_SELECT_REGS) and of the bound of
threshold_tail16_kernel at the edges of its load rounds (written for a one-read form of its sample pass, which did not
measure faster and is not in the library; the cases pin the kernel as it is).

The select: final rows, counts and status of the device entry are equal between SCANN_HIP_SELECT_REGS = 0 (the list
swept four times from global memory) and 1, the host entry's rows are the oracle's; on candidate capacities on both
sides of every instantiation (16, 26 and 36 keys per thread of 512) and of the fall-back above the largest, on tie-heavy
lists (a crowded bin, a range narrower than the histogram), on lists of exactly m, m - 1 and more than `cap` keys, and
under a bitmap that leaves a list shorter than one key per thread.

The bound: read back through debug_filter_bounds, it is bit for bit the gather sample's (SCANN_HIP_SAMPLE_MFMA = 0,
threshold_tail_kernel) at sample rows 1 under, at and 1 over a multiple of 256 x 8 eight-byte words (one round of loads
of the 256 threads), at the longest row the plan makes (32767 samples) and with fewer than J samples present.

Flat hashers, S = 8, dim 32, 40 queries: the staged batched pipeline, whose select reads its list `direct` (cap > 4096)."""
import numpy as np
import pytest

import helpers as H
from oracle import pyoracle as orc
from scann_rust_amd import hip, synth

pytestmark = pytest.mark.gpu

S, DIM, NQ, K = 8, 32, 40, 10
ABORTED = 10   # scann_hip.h SCANN_HIP_ABORTED
KEY_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
REG_THREADS, REG_VPT = 512, (16, 26, 36)   # txh.hip kSelRegThreads and launch_select's instantiations


def _stream():
    import torch
    return torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream


def _opts(m):
    o = hip.default_opts()
    o.pre_reorder_k = m
    return o


def _case(n, seed):
    rng = np.random.default_rng(seed)
    rows = synth.uniform_f32(n, DIM, seed)
    cb = np.ascontiguousarray(rows[rng.choice(n, 16, replace=False)].reshape(16, S, DIM // S).transpose(1, 0, 2),
                              np.float32)
    codes = rng.integers(0, 16, (n, S), dtype=np.uint8)
    return cb, codes, rows, synth.uniform_f32(NQ, DIM, seed + 1)


def _decoded(cb, code_row):
    return np.ascontiguousarray(cb[np.arange(S), code_row].reshape(DIM), np.float32)


def _both(index, q, m, monkeypatch, allow=None, allow_bits=None):
    """{knob: (status, idx, dist, count)} of the device entry under SCANN_HIP_SELECT_REGS = 0 and 1"""
    out = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("SCANN_HIP_SELECT_REGS", knob)
        out[knob] = H.device_search(index, q, K, _opts(m), allow=allow, allow_bits=allow_bits)
    monkeypatch.delenv("SCANN_HIP_SELECT_REGS")
    return out


def _assert_same(out, what):
    (s0, i0, d0, c0), (s1, i1, d1, c1) = out["0"], out["1"]
    print("%s: status %d / %d, counts %s / %s" % (what, s0, s1, np.unique(c0), np.unique(c1)))
    assert s0 == s1, "%s: status %d vs %d" % (what, s0, s1)
    assert np.array_equal(c0, c1), what + ": counts"
    for i in range(c0.size):
        assert np.array_equal(i0[i, :c0[i]], i1[i, :c1[i]]), "%s q%d: indices" % (what, i)
        assert np.array_equal(d0[i, :c0[i]].view(np.uint32), d1[i, :c1[i]].view(np.uint32)), "%s q%d: distances" % (what, i)


def _assert_host_is_oracle(index, kw, cb, codes, q, m, which, what):
    """host entry (it repeats failed queries without a bound), default knobs: the oracle's rows"""
    idx, dist, cnt = index.search_batched(q, K, _opts(m))
    for i in which:
        oi, od = orc.ah_search_with_reordering(cb, codes, kw["data"], kw["stride"], q[i], K, m)
        assert cnt[i] == oi.size, "%s q%d" % (what, i)
        H.assert_topk_equal_up_to_ties(idx[i, :cnt[i]], dist[i, :cnt[i]], oi, od, what="%s q%d" % (what, i))
    return idx, dist, cnt


def _regs_vpt(cap):
    """keys per thread of the instantiation launch_select takes for `cap`; None: the global-memory kernel"""
    return next((v for v in REG_VPT if cap <= v * REG_THREADS), None)


# (n, m) -> cap = (J + 8 sqrt(J) + 16) st + 256: ~5.8 k, ~10.2 k, ~14.5 k, and ~18.5 k (past 36 x 512 = 18432: the
# fall-back; 1.2M rows are the fewest that reach it -- the stride grows with the index, m is at its limit)
CAPS = [(131072, 2000, 16), (262144, 5000, 26), (262144, 8192, 36), (1200000, 8192, None)]


@pytest.mark.parametrize("n,m,vpt", CAPS)
def test_capacities_around_every_instantiation(n, m, vpt, monkeypatch):
    H.scan_env(monkeypatch, "default")
    st, J, cap, _ = H.plan_caps(n, 1, m)
    what = "n%d m%d (st %d, J %d, cap %d)" % (n, m, st, J, cap)
    assert cap > 4096, what + ": the select does not read its list from global memory"
    assert _regs_vpt(cap) == vpt, what
    cb, codes, rows, q = _case(n, 3100 + m)
    kw = H.ah_kwargs_from_codes(rows, cb, codes)
    index = hip.txh_create(**kw)
    out = _both(index, q, m, monkeypatch)
    assert out["1"][0] == hip.OK, what
    assert np.all(out["1"][3] == K), what
    _assert_same(out, what)
    which = (0, NQ // 2, NQ - 1) if n < 1000000 else (NQ // 2,)   # (the oracle walks every row)
    idx, dist, cnt = _assert_host_is_oracle(index, kw, cb, codes, q, m, which, what)
    _, di, dd, dc = out["1"]
    assert np.array_equal(dc, cnt), what
    assert np.array_equal(di, idx) and np.array_equal(dd.view(np.uint32), dist.view(np.uint32)), what + ": device / host"


def test_capacity_table_covers_both_sides_of_every_limit():
    """the shapes above lie on both sides of 16, 26 and 36 keys per thread (no GPU work: the plan mirror only)"""
    caps = [H.plan_caps(n, 1, m)[2] for n, m, _ in CAPS]
    for v in REG_VPT:
        assert any(c <= v * REG_THREADS for c in caps) and any(c > v * REG_THREADS for c in caps), (v, caps)


N_T, M_T = 131072, 2000   # st 16, J 214, cap 5808


def _three_rows_case(seed):
    """Every code row is one of three: A on every 80th position (never a sampled one), B on the other positions below
    16384, C, the farthest, elsewhere.  The first 1024 samples are B -- four in every thread of the tail kernel, fewer
    than its list holds -- so the bound is the J-th of them, at position 3408.  A query keeps B's ~3360 points up to
    there: keys that differ in their low words only, over a range under 4096 (sh == 0).  Where A is nearer than B it
    also keeps A's 1639 points, a distance apart: two crowded bins, the rank's narrowed once."""
    rng = np.random.default_rng(seed)
    cb, codes, rows, q = _case(N_T, seed)
    cand = rng.integers(0, 16, (64, S), dtype=np.uint8)   # A, then the candidate nearest to A as B, the farthest as C
    d = ((cb[np.arange(S), cand].reshape(64, DIM) - _decoded(cb, cand[0])) ** 2).sum(1)
    order = np.argsort(d[1:]) + 1
    three = cand[[0, order[0], order[-1]]]
    pos = np.arange(N_T)
    which = np.where(pos % 80 == 5, 0, np.where(pos < 16384, 1, 2))
    codes = three[which]
    rows = np.ascontiguousarray(cb[np.arange(S)[None, :], codes].reshape(N_T, DIM), np.float32)
    near_a, near_b = _decoded(cb, three[0]), _decoded(cb, three[1])
    q = np.float32(0.01) * q
    q[:NQ // 2] += near_a    # A first, then B
    q[NQ // 2:] += near_b    # B first: one tie group, the rank's range found at once
    return cb, codes, rows, np.ascontiguousarray(q, np.float32)


def test_tie_heavy_lists(monkeypatch):
    H.scan_env(monkeypatch, "default")
    st, J, cap, _ = H.plan_caps(N_T, 1, M_T)
    assert (st, J) == (16, 214) and cap > 4096 and _regs_vpt(cap) == 16
    cb, codes, rows, q = _three_rows_case(3200)
    kw = H.ah_kwargs_from_codes(rows, cb, codes)
    index = hip.txh_create(**kw)
    out = _both(index, q, M_T, monkeypatch)
    bounds = index.debug_filter_bounds(NQ, _stream())
    low = np.uint64(0xFFFFFFFF)
    assert np.all((bounds & low) == np.uint64((J - 1) * st)), "the bound is the J-th sampled B row: %s" % bounds[:4]
    assert out["1"][0] == hip.OK
    _assert_same(out, "three code rows")
    _assert_host_is_oracle(index, kw, cb, codes, q, M_T, (0, NQ // 2, NQ - 1), "three code rows")


def _dup_case(extra, seed, front):
    """Copies of one row: 300 sampled positions (the first ones if `front`, else the last ones) and `extra` unsampled
    positions in the first half; every query sits next to the copies.  The bound is the J-th sampled copy, so a query
    keeps J keys and the original at position 1 (front), or J + extra (the unsampled copies, the original among them,
    lie at lower positions than every sampled one)."""
    cb, codes, rows, q = _case(N_T, seed)
    st = H.sample_stride(N_T)
    sampled = np.arange(0, N_T, st)
    dup = sampled[:300] if front else sampled[-300:]
    unsampled = np.flatnonzero(np.arange(N_T // 2) % st != 0)[:extra]
    proto = codes[1].copy()
    for at in (dup, unsampled):
        codes[at] = proto
    rows[dup] = rows[1]
    rows[unsampled] = rows[1]
    near = _decoded(cb, proto)
    q = np.ascontiguousarray(near + np.float32(0.01) * q, np.float32)
    return cb, codes, rows, q


@pytest.mark.parametrize("name,extra,front,want", [("m", M_T - 214, False, hip.OK), ("m-1", M_T - 215, False, ABORTED),
                                                   ("J", 0, True, ABORTED), ("over-cap", 7000, False, hip.RESOURCE_EXHAUSTED)])
def test_list_of_m_fewer_and_too_many(name, extra, front, want, monkeypatch):
    """cnt == m: everything stays; cnt == m - 1 and cnt == J under a bound: Aborted, count 0; cnt > cap: ResourceExhausted,
    count 0 (7214 keys: under the prefilter's list, over the select's).  The host entry repeats the failed queries."""
    H.scan_env(monkeypatch, "default")
    st, J, cap, cap32 = H.plan_caps(N_T, 1, M_T)
    assert (st, J) == (16, 214) and 4096 < cap < 7000 + J < cap32
    cb, codes, rows, q = _dup_case(extra, 3300, front)
    kw = H.ah_kwargs_from_codes(rows, cb, codes)
    index = hip.txh_create(**kw)
    out = _both(index, q, M_T, monkeypatch)
    _assert_same(out, name)
    status, _, _, dc = out["1"]
    assert status == want, "%s: status %d" % (name, status)
    assert np.all(dc == (K if want == hip.OK else 0)), name
    _assert_host_is_oracle(index, kw, cb, codes, q, M_T, (0, NQ - 1), name)
    host = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("SCANN_HIP_SELECT_REGS", knob)
        host[knob] = index.search_batched(q, K, _opts(M_T))
    for a, b in zip(host["0"], host["1"]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name + ": host entry"


def test_bitmap_that_rejects_most_points(monkeypatch):
    """0.1 % of the rows allowed: fewer than J allowed samples, so no bound, and ~130 candidates per query -- fewer than
    m and fewer than the workgroup has threads"""
    H.scan_env(monkeypatch, "default")
    cb, codes, rows, q = _case(N_T, 3400)
    kw = H.ah_kwargs_from_codes(rows, cb, codes)
    index = hip.txh_create(**kw)
    words, bits = H.allow_family("f0.1", [0, N_T], None, np.zeros((NQ, 1)), K, M_T, H.sample_stride(N_T), 5)
    allowed = H.allowed_ids(words, bits, N_T)
    assert K < allowed.size < REG_THREADS
    out = _both(index, q, M_T, monkeypatch, allow=words, allow_bits=bits)
    assert np.all(index.debug_filter_bounds(NQ, _stream()) == KEY_MAX)
    _assert_same(out, "f0.1")
    status, di, dd, dc = out["1"]
    assert status == hip.OK and np.all(dc == K)
    for i in (0, NQ - 1):   # every allowed point is a candidate: the exact k nearest among them
        d = ((rows[allowed].astype(np.float64) - q[i].astype(np.float64)) ** 2).sum(1)
        assert set(di[i].tolist()) == set(allowed[np.argsort(d, kind="stable")[:K]].tolist()), "f0.1 q%d" % i


# ---- threshold_tail16_kernel: the bound at the edges of the load rounds -----------------------------------------------
def _n_with_words(words):
    """the smallest index size whose sample row is `words` eight-byte words (four u16 samples each) long"""
    for n in range(120000, 160000):
        st, _ = H.sample_plan(n, 1)
        if (-(-n // st) + 3) // 4 == words:
            return n
    raise AssertionError(words)


def _bounds_both_samples(index, q, m, monkeypatch, allow=None, allow_bits=None):
    out = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("SCANN_HIP_SAMPLE_MFMA", knob)
        r = H.device_search(index, q, K, _opts(m), allow=allow, allow_bits=allow_bits)
        out[knob] = r + (index.debug_filter_bounds(q.shape[0], _stream()),)
    monkeypatch.delenv("SCANN_HIP_SAMPLE_MFMA")
    return out


def _assert_bounds_equal(out, what):
    b0, b1 = out["0"][4], out["1"][4]
    bad = np.flatnonzero(b0 != b1)
    assert bad.size == 0, "%s: bounds differ at queries %s: %s vs %s" % (what, bad[:8], b0[bad[:8]], b1[bad[:8]])
    _assert_same({k: v[:4] for k, v in out.items()}, what)


@pytest.mark.parametrize("words", [2047, 2048, 2049])
def test_bound_at_rows_around_a_multiple_of_the_load_round(words, monkeypatch):
    H.scan_env(monkeypatch, "default")
    n = _n_with_words(words)
    cb, codes, rows, q = _case(n, 3500 + words)
    index = hip.txh_create(**H.ah_kwargs_from_codes(rows, cb, codes))
    out = _bounds_both_samples(index, q, M_T, monkeypatch)
    assert out["1"][0] == hip.OK and np.all(out["1"][4] != KEY_MAX), words
    _assert_bounds_equal(out, "n%d: %d words" % (n, words))


@pytest.mark.parametrize("n", [524288, 524272])
def test_bound_of_the_longest_sample_rows(n, monkeypatch):
    """524272 x 32: stride 16, 32767 samples in a row of kSampleTarget entries -- the longest row the plan makes, 8192
    words, four rounds of loads; 524288 rows would need one entry more and take stride 19
    (27595 samples)"""
    H.scan_env(monkeypatch, "default")
    st, scap = H.sample_plan(n, 1)
    assert (st, scap) == ((16, H.SAMPLE_TARGET) if n == 524272 else (19, 27596))
    cb, codes, rows, q = _case(n, 3600)
    index = hip.txh_create(**H.ah_kwargs_from_codes(rows, cb, codes))
    out = _bounds_both_samples(index, q, M_T, monkeypatch)
    assert out["1"][0] == hip.OK and np.all(out["1"][4] != KEY_MAX)
    _assert_bounds_equal(out, "full row")


@pytest.mark.parametrize("fam", ["f1", "unsampled", "f10"])
def test_bound_with_few_samples_present(fam, monkeypatch):
    """allow-bitmaps: 1 % of the rows (fewer than J samples present) and no sampled row at all publish no bound; 10 %
    publish the gather sample's"""
    H.scan_env(monkeypatch, "default")
    cb, codes, rows, q = _case(N_T, 3700)
    index = hip.txh_create(**H.ah_kwargs_from_codes(rows, cb, codes))
    words, bits = H.allow_family(fam, [0, N_T], None, np.zeros((NQ, 1)), K, M_T, H.sample_stride(N_T), 5)
    out = _bounds_both_samples(index, q, M_T, monkeypatch, allow=words, allow_bits=bits)
    assert np.all((out["1"][4] == KEY_MAX) == (fam != "f10")), fam
    _assert_bounds_equal(out, fam)

"""GPU checks of the flat hasher's integer-MFMA sample (txh.hip K5d / K5e, SCANN_HIP_SAMPLE_MFMA): the filter bounds
read back from the workspace are bit-equal to the gather sample's for every query, the rows are the oracle's and equal
between the two knob values on both entries, a flooded list publishes a bound at or above the old one, and the plans
outside the new path's scope (tree index, SCANN_HIP_THR_TAIL=0, byte codes) are untouched by the knob.

Shapes: the smallest where threshold_tail_kernel engages -- N ~ 80 000 (sample stride 16, scap ~ 5004 > 4096) with
m = 1000 (J = 133 <= 384), k = 10."""
import numpy as np
import pytest

import helpers as H
import sample_bound_model as model
from oracle import pyoracle as orc
from scann_rust_amd import hip, synth

pytestmark = pytest.mark.gpu

N, K, M = 80000, 10, 1000
KEY_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


def _stream():
    import torch
    return torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream


def _opts():
    o = hip.default_opts()
    o.pre_reorder_k = M
    return o


def _flat_case(n, dim, S, nq, seed, values=None):
    """codebook = 16 rows cut into subspaces, random codes, queries; values: draw everything from these instead"""
    rng = np.random.default_rng([seed, S])
    dsub = dim // S
    if values is None:
        rows = synth.uniform_f32(n, dim, seed)
        cb = np.ascontiguousarray(rows[rng.choice(n, 16, replace=False)].reshape(16, S, dsub).transpose(1, 0, 2),
                                  np.float32)
        codes = rng.integers(0, 16, (n, S), dtype=np.uint8)
        q = synth.uniform_f32(nq, dim, seed + 1)
    else:
        v = np.asarray(values, np.float32)
        cb = rng.choice(v, (S, 16, dsub))
        codes = rng.integers(0, 16, (n, S), dtype=np.uint8)
        rows = np.ascontiguousarray(cb[np.arange(S)[None, :], codes].reshape(n, dim), np.float32)
        q = rng.choice(v, (nq, dim))
    return cb, codes, rows, np.ascontiguousarray(q, np.float32)


def _both(index, q, monkeypatch, allow=None, allow_bits=None):
    """{knob: (status, idx, dist, count, bounds)} of the device entry under SCANN_HIP_SAMPLE_MFMA = 0 and 1"""
    out = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("SCANN_HIP_SAMPLE_MFMA", knob)
        status, di, dd, dc = H.device_search(index, q, K, _opts(), allow=allow, allow_bits=allow_bits)
        out[knob] = (status, di, dd, dc, index.debug_filter_bounds(q.shape[0], _stream()))
    return out


def _assert_same(out, what, bounds_equal=True):
    (s0, i0, d0, c0, b0), (s1, i1, d1, c1, b1) = out["0"], out["1"]
    if bounds_equal:
        bad = np.flatnonzero(b0 != b1)
        assert bad.size == 0, "%s: bounds differ at queries %s: %s vs %s" % (what, bad[:8], b0[bad[:8]], b1[bad[:8]])
    assert s0 == s1, "%s: status %d vs %d" % (what, s0, s1)
    assert np.array_equal(c0, c1), what + ": counts"
    for i in range(c0.size):
        assert np.array_equal(d0[i, :c0[i]].view(np.uint32), d1[i, :c1[i]].view(np.uint32)), "%s q%d: distances" % (what, i)
        assert np.array_equal(i0[i, :c0[i]], i1[i, :c1[i]]), "%s q%d: indices" % (what, i)


def _assert_oracle(index, kw, cb, codes, q, which, monkeypatch, what):
    """host entry, default knob: the oracle's rows for the queries `which`"""
    monkeypatch.delenv("SCANN_HIP_SAMPLE_MFMA", raising=False)
    idx, dist, cnt = index.search_batched(q, K, _opts())
    for i in which:
        oi, od = orc.ah_search_with_reordering(cb, codes, kw["data"], kw["stride"], q[i], K, M)
        assert cnt[i] == oi.size, "%s q%d" % (what, i)
        H.assert_topk_equal_up_to_ties(idx[i, :cnt[i]], dist[i, :cnt[i]], oi, od, what="%s q%d" % (what, i))
    return idx, dist, cnt


# S, dim, queries, rows: partial pair tiles (33 = 32 + 1, 70 = 2 x 32 + 6: padding columns), a partial last sample
# tile and a partial last group of four (80 037 rows: 5003 samples), dsub = 2 and 4
SHAPES = [(32, 128, 33, N), (24, 96, 70, N), (64, 128, 33, N + 37), (8, 32, 70, N + 37), (32, 128, 70, N + 37)]


@pytest.mark.parametrize("S,dim,nq,n", SHAPES)
def test_bounds_and_rows_equal_the_gather_sample(S, dim, nq, n, monkeypatch):
    H.scan_env(monkeypatch, "default")
    cb, codes, rows, q = _flat_case(n, dim, S, nq, 2100 + S)
    kw = H.ah_kwargs_from_codes(rows, cb, codes)
    index = hip.txh_create(**kw)
    index.enable_timing(True)
    what = "S%d nq%d n%d" % (S, nq, n)
    out = _both(index, q, monkeypatch)
    assert index.last_kernel_ms()[1] == H.sparse_kernel_name(S), what
    assert out["1"][0] == hip.OK, what
    assert np.all(out["1"][4] != KEY_MAX), what + ": every query has a bound"
    _assert_same(out, what)
    idx, dist, cnt = _assert_oracle(index, kw, cb, codes, q, (0, nq // 2, nq - 1), monkeypatch, what)
    _, di, dd, dc, _ = out["1"]   # the device entry's rows are the host entry's
    assert np.array_equal(dc, cnt), what
    for i in range(nq):
        assert np.array_equal(di[i, :cnt[i]], idx[i, :cnt[i]]), "%s q%d device / host" % (what, i)
        assert np.array_equal(dd[i, :cnt[i]].view(np.uint32), dist[i, :cnt[i]].view(np.uint32)), "%s q%d" % (what, i)


def test_three_valued_data_ties_by_slot(monkeypatch):
    """codewords, rows and queries in {-1, 0, 1}: exact tables, thousands of tied sample distances -- the bound's low
    word (the stream position of the J-th key) must come out the same"""
    S, dim, nq = 32, 128, 33
    H.scan_env(monkeypatch, "default")
    cb, codes, rows, q = _flat_case(N, dim, S, nq, 2200, values=(-1.0, 0.0, 1.0))
    kw = H.ah_kwargs_from_codes(rows, cb, codes)
    index = hip.txh_create(**kw)
    out = _both(index, q, monkeypatch)
    b = out["1"][4]
    assert np.all(b != KEY_MAX) and np.all((b & np.uint64(0xFFFFFFFF)) != np.uint64(0xFFFFFFFF)), "no flooded list"
    d = orc.lut_from_query(cb, q[0])   # (ties are there: far fewer distinct sample distances than samples)
    t = d.reshape(S, 16)
    sums = t[np.arange(S)[None, :], codes[::16]].sum(1)
    assert np.unique(sums).size * 8 < sums.size
    _assert_same(out, "three-valued")


def test_unquantised_tables_take_the_f32_passes(monkeypatch):
    """one query with a NaN, one with a component whose square overflows: their tables are not quantised (scale 0) and
    the tail kernel scores their samples in f32 -- the same bounds, for them and for their neighbours"""
    S, dim, nq = 32, 128, 33
    H.scan_env(monkeypatch, "default")
    cb, codes, rows, q = _flat_case(N, dim, S, nq, 2300)
    q[3, 5] = np.nan
    q[7, 9] = 1e20
    for i in (3, 7):   # lut8_build_kernel's quantiser (its numpy statement) gives these tables scale 0, the others not
        assert model.quantise(orc.lut_from_query(cb, q[i]).reshape(S, 16))[2] == 0.0
    assert model.quantise(orc.lut_from_query(cb, q[0]).reshape(S, 16))[2] > 0.0
    index = hip.txh_create(**H.ah_kwargs_from_codes(rows, cb, codes))
    out = _both(index, q, monkeypatch)
    _assert_same(out, "nan / huge")
    assert np.all(np.delete(out["1"][4], [3, 7]) != KEY_MAX)


@pytest.mark.parametrize("fam", ["f10", "f1", "sampled", "unsampled"])
def test_bounds_under_filters(fam, monkeypatch):
    """allow-bitmaps: 10 % and 1 % of the rows (1 %: fewer than J allowed samples, no bound), exactly the sampled rows,
    exactly the others (every sample absent)"""
    S, dim, nq, n = 32, 128, 33, N + 37
    H.scan_env(monkeypatch, "default")
    cb, codes, rows, q = _flat_case(n, dim, S, nq, 2400)
    index = hip.txh_create(**H.ah_kwargs_from_codes(rows, cb, codes))
    words, cap = H.allow_family(fam, [0, n], None, np.zeros((nq, 1)), K, M, H.sample_stride(n), 5)
    out = _both(index, q, monkeypatch, allow=words, allow_bits=cap)
    _assert_same(out, fam)
    if fam in ("f1", "unsampled"):
        assert np.all(out["1"][4] == KEY_MAX), fam
    else:
        assert np.all(out["1"][4] != KEY_MAX), fam


def _flood_case(nq, S=32, dim=128):
    """nine rows in ten are copies of one row and the first half of the queries sit next to its codewords: the J-th
    smallest sample key lies inside a tie group of ~4500 samples, more than the tail kernels' list holds"""
    cb, codes, rows, q = _flat_case(N, dim, S, nq, 2500)
    dup = np.arange(N) % 10 != 0
    codes[dup] = codes[1]
    rows[dup] = rows[1]
    near = cb[np.arange(S), codes[1]].reshape(dim)   # the copies' code row decoded: their approximate distance is ~0
    q[:nq // 2] = near + np.float32(0.01) * q[:nq // 2]
    return S, cb, codes, rows, q


@pytest.mark.parametrize("S,dim", [(8, 32), (24, 96), (32, 128), (64, 128)])
def test_flooded_list_publishes_a_looser_bound(S, dim, monkeypatch):
    """both samples flood on the near queries; the new bound is at or above the old one and the rows stay equal.  At
    every S this is also the witness that the integer sample ran: only it publishes (Dmax, MAX)"""
    nq = 34
    H.scan_env(monkeypatch, "default")
    S, cb, codes, rows, q = _flood_case(nq, S, dim)
    index = hip.txh_create(**H.ah_kwargs_from_codes(rows, cb, codes))
    out = _both(index, q, monkeypatch)
    b0, b1 = out["0"][4], out["1"][4]
    flooded = np.arange(nq) < nq // 2
    low = np.uint64(0xFFFFFFFF)
    assert np.all((b0[flooded] & low) == low) and np.all((b1[flooded] & low) == low), "both lists flood"
    assert np.all(b1 >= b0), "a flooded bound is at or above the gather sample's"
    assert np.any(b1[flooded] > b0[flooded]), "(Dmax, MAX) lies above (pivot, MAX): the integer sample ran"
    exact = (b0 & low) != low   # (a far query's J-th key may fall into the tie group as well)
    assert exact.any() and np.array_equal(b0[exact], b1[exact])
    assert out["0"][0] == out["1"][0]
    host = {}
    for knob in ("0", "1"):   # the host entry repeats overflowing queries without a bound: the same rows
        monkeypatch.setenv("SCANN_HIP_SAMPLE_MFMA", knob)
        host[knob] = index.search_batched(q, K, _opts())
    for a, b in zip(host["0"], host["1"]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_knob_does_not_reach_other_plans(monkeypatch):
    """SCANN_HIP_THR_TAIL=0, a tree index and byte codes keep the gather sample: on the flood case, where the two
    samples publish different bounds, the knob changes nothing; the tree and the byte-code scans read back equal"""
    nq = 34
    H.scan_env(monkeypatch, "default")
    S, cb, codes, rows, q = _flood_case(nq)
    monkeypatch.setenv("SCANN_HIP_THR_TAIL", "0")
    index = hip.txh_create(**H.ah_kwargs_from_codes(rows, cb, codes))
    _assert_same(_both(index, q, monkeypatch), "THR_TAIL=0")
    monkeypatch.delenv("SCANN_HIP_THR_TAIL")
    # tree index over the same rows: four leaves, all probed
    oix, kw = H.txh_from_codes(rows, cb, codes, 4, 4, 1.0, 7, use_residuals=False)
    tree = hip.txh_create(**kw)
    _assert_same(_both(tree, q, monkeypatch), "tree")
    # byte codes (K = 256): the gather scan
    rng = np.random.default_rng(12)
    dim, S8 = 32, 8
    rows8 = synth.uniform_f32(N, dim, 2600)
    cb8 = np.ascontiguousarray(rows8[rng.choice(N, 256, replace=False)].reshape(256, S8, dim // S8).transpose(1, 0, 2),
                               np.float32)
    codes8 = rng.integers(0, 256, (N, S8), dtype=np.uint8)
    flat8 = hip.txh_create(**H.ah_kwargs_from_codes(rows8, cb8, codes8))
    flat8.enable_timing(True)
    out = _both(flat8, synth.uniform_f32(nq, dim, 2601), monkeypatch)
    assert flat8.last_kernel_ms()[1] == "adc_scan_kernel"
    _assert_same(out, "byte codes")

"""Mutable indexes over a STAGED base with a sampled bound, on every integer-MFMA prefilter scan the base can run: the
three-stage route (the live bitmap, or live & user built by live_and_user_words_kernel / live_and_user_gather_kernel,
handed to the base's device entry as a device bitmap) against tests/mutable_model.py.

tests/test_gpu_mutable.py runs that route over bases of 2000 rows and 9 queries: the small pipeline, no bound, the
gather scan.  Here the bases are the shapes of tests/test_gpu_sp_bitmap.py:
  flat  Case("ah", 32, n=4133, nq=65): four full 1024-point ranges plus a 37-point range whose last tile has 5 live
        rows; 65 queries = a second 64-pair item holding one pair; pre_reorder_k = 250, a sampled bound in force
  tree  Case("txh", 32, n=20000, nq=65)
and every test forces one scan and asserts that it ran: scann_hip_index_last_kernel_ms on the base (the mutable handle
calls the base's device entry on a stream of its own; it is the first device stream the base sees, so it runs on the
base's primary workspace, which debug_survivor_bitmap_bytes() reports: bitmaps of the call's size under the bitmap
form, none under the lists).  A fallback to the host entry would name the retry's gather scan, and the precondition
(the bare base's device entry reports Ok under the same bitmap, on a handle of its own) rules it out beforehand.

No tolerance: distances bitwise, ids up to ties of the distance (the model's rows have none: asserted), unused slots
0xFFFFFFFF / +inf; every one of the 65 queries is compared in every search."""
import numpy as np
import pytest

from oracle import pyoracle as orc
from scann_rust_amd import hip, synth
import fold_model as fm
import helpers as H
from test_gpu_filters import Case, K, L, M, P
from test_gpu_mutable import Pair, check_lists
from test_gpu_sp_bitmap import _bitmap_bytes, _knob

pytestmark = pytest.mark.gpu

CAPACITY = 1280
assert CAPACITY >= 1200 and hip.MUTABLE_DELTA_TILE == 1024
# scan name -> (_knob arguments, the kernel the base names, survivor bitmaps in its workspace)
FLAT_SCANS = {
    "bitmap": (dict(value=None), "adc_smfmac_kernel", True),
    "lists": (dict(value="0"), "adc_smfmac_kernel", False),
    "dense32": (dict(value=None, pairs=None, scan="dense32"), "adc_mfma_kernel", False),
    "resident": (dict(value=None, pairs=None, scan="resident"), "adc_scan_res_kernel", False),
}
TREE_SCANS = {
    "sp-words": (dict(value=None, pairs=None, scan="sp-words"), "adc_smfmac_kernel", False),
    "mfma16": (dict(value=None, pairs=None, scan="mfma16"), "adc_mfma16_kernel", False),
}


@pytest.fixture(scope="module")
def cases():
    """the two bases, built once, and the model's expected rows per (kind, phase, filter): they do not depend on the
    scan, so the first test that reaches a search computes them for the others"""
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = (Case("ah", 32, n=4133, nq=65) if kind == "ah" else Case("txh", 32, n=20000, nq=65), {})
        return cache[kind]

    yield get
    cache.clear()


def _rows_of(c):
    return np.ascontiguousarray(c.data.reshape(c.n, c.stride)[:, :c.dim])


def _fresh_rows(c, count, seed):
    """rows of the base's own distribution"""
    if c.kind == "ah":
        return synth.uniform_f32(count, c.dim, seed)
    return synth.clustered_f32(count, c.dim, seed, n_clusters=L)[0]


def _removal_set(c, protect, seed):
    """~5 % of the base rows: the range and word edges 1023 / 1024 / 4095 / 4096, rows of the last 37 points (of the
    flat hasher's tail range: its first, two of the last tile's 5 live rows), a true top-1 row, and a random rest"""
    n = c.n
    edge = np.unique([1023, 1024, 4095, 4096, n - 37, n - 36, n - 5, n - 1, int(c.topk[2][0])])
    rest = np.setdiff1d(np.arange(n), np.concatenate([edge, protect]))
    rm = np.concatenate([edge, np.random.default_rng(seed).choice(rest, n // 20 - edge.size, replace=False)])
    assert np.unique(rm).size == rm.size == n // 20 and not np.intersect1d(rm, protect).size
    return rm


def mutate(p, c, seed):
    """the script on a Pair over base `c`: removes ~5 % of the base rows; updates 40 base rows (tombstone + delta row
    under the old id), among them the true top-1 row of query 0 (to a far row) and of query 1 (to a row next to the
    query); adds a row next to each of 8 queries; adds 1000 more rows, so that the delta holds more than one
    SCANN_HIP_MUTABLE_DELTA_TILE.  Returns (removed ids, updated ids, ids next to queries)."""
    dim, q = c.dim, c.q
    top0, top1 = int(c.topk[0][0]), int(c.topk[1][0])
    assert top0 != top1
    rm = _removal_set(c, np.array([top0, top1]), seed)
    p.remove(rm)
    fresh = _fresh_rows(c, 1100, seed + 1)
    noise = np.float32(1e-3) * synth.uniform_f32(16, dim, seed + 2)
    others = np.setdiff1d(np.arange(c.n), np.concatenate([rm, [top0, top1]]))[7::97][:38]
    up = np.concatenate([[top0, top1], others])
    upr = fresh[:40].copy()
    upr[1] = q[1] + noise[1]
    p.update(up, upr)
    near = p.add(q[8:16] + noise[8:16])
    p.add(fresh[40:1040])
    assert len(p.model.delta_ids) == 1048 > hip.MUTABLE_DELTA_TILE + 1
    return rm, up, near


def mutate_again(p, c, ei):
    """after a rebase onto base_ids `ei`: removals at the NEW base's word / range edges (rows 63 / 64 / 1023 / 1024 of
    the new base, whose ids differ from their row numbers) and every 41st row, updates of base rows, rows next to four
    queries and 60 more.  Returns (removed ids, ids next to queries)."""
    n2 = ei.size
    rows2 = np.array([63, 64, 1023, 1024, n2 - 1] + list(range(5, n2, 41)))
    rm2 = ei[rows2]
    assert np.any(rm2 != rows2)
    p.remove(rm2)
    live2 = np.setdiff1d(ei, rm2)
    p.update(live2[3::211], _fresh_rows(c, live2[3::211].size, 901))
    near2 = p.add(c.q[20:24] + np.float32(1e-3) * synth.uniform_f32(4, c.dim, 902))
    p.add(_fresh_rows(c, 60, 903))
    return rm2, near2


def _filters(p, removed):
    """(name, words, capacity) over external ids: none; about half of them, with a capacity that ends inside the delta
    ids; only removed ids"""
    nxt = p.model.next_index
    first_delta = int(p.model.base_ids[-1]) + 1
    half = np.flatnonzero(np.random.default_rng(77).random(nxt) < 0.5)
    cap = first_delta + (nxt - first_delta) // 2
    assert first_delta < cap < nxt and np.any(half >= cap) and np.any((half >= first_delta) & (half < cap))
    gone = [int(i) for i in removed if not p.model.exists(int(i))]
    assert len(gone) >= 10
    return [("no filter", None, None), ("half", H.words_of(half, nxt)[0], cap),
            ("only removed", H.words_of(gone, nxt)[0], nxt)]


def _want(p, c, oix, codes, allow, allow_bits):
    if c.kind == "ah":
        return p.model.search_ah(c.cb, codes, c.q, K, M, allow, allow_bits)
    return p.model.search_txh(oix, c.q, K, allow, allow_bits, pre_reorder_k=M)


def _precondition(kw, c, words_list, n, name, what):
    """on a handle of its own (so that the mutable handle's stream stays the base's first device stream): the bare
    base's device entry reports Ok under each bitmap -- the three-stage route, not the host repeat, is what runs"""
    bare = hip.txh_create(**kw)
    bare.enable_timing(True)
    for words in words_list:
        status = H.device_search(bare, c.q, K, c.opts(), allow=words, allow_bits=n)[0]
        assert status == hip.OK, "%s: the bare base's device entry reports %d" % (what, status)
        assert bare.last_kernel_ms()[1] == name, what
    return bare


def _searches(p, c, base, oix, codes, kw, removed, phase, name, bitmap, expected):
    """the three filters through the mutable handle, every query against the model; the scan that ran"""
    n_base = p.model.base_ids.size
    filters = _filters(p, removed)
    base_words = [p.model.base_allow_words(w, cap)[0] for _, w, cap in filters]
    bare = _precondition(kw, c, base_words, n_base, name, phase)
    for (fname, words, cap), bw in zip(filters, base_words):
        what = "%s %s %s" % (c.kind, phase, fname)
        got = p.mut.search_batched(c.q, K, opts=c.opts(), allow=words, allow_bits=cap)
        assert base.last_kernel_ms()[1] == name, "%s: ran %s" % (what, base.last_kernel_ms()[1])
        assert base.debug_survivor_bitmap_bytes() == (_bitmap_bytes(n_base, c.q.shape[0]) if bitmap else 0), what
        key = (phase, fname)
        if key not in expected:
            expected[key] = _want(p, c, oix, codes, words, cap)
        check_lists(got, expected[key], K, what)
        if fname == "only removed":
            assert not got[2].any(), what
        else:
            assert np.all(got[2] == K), what
        if phase == "script":
            # the base's own filtered answer under live & user, against the oracle as tests/test_gpu_filters.py reads it
            staged = bare.search_batched(c.q, K, c.opts(), stages=True, allow=bw, allow_bits=n_base)
            assert bare.last_kernel_ms()[1] == name, what + " bare"
            c.check(c.q, bw, n_base, staged, (0, 33, 64), what + " bare")
    bare.close()


def _run(c, expected, scan, monkeypatch):
    knob, name, bitmap = (FLAT_SCANS if c.kind == "ah" else TREE_SCANS)[scan]
    _knob(monkeypatch, **knob)
    base = hip.txh_create(**c.kw)
    base.enable_timing(True)
    p = Pair(base, _rows_of(c), CAPACITY)
    rm, up, near = mutate(p, c, 500)
    _searches(p, c, base, c.oix, getattr(c, "codes", None), c.kw, rm, "script", name, bitmap, expected)
    got = p.mut.search_batched(c.q, K, opts=c.opts())
    assert got[0][1, 0] == up[1], "the updated top-1 row of query 1 answers from the delta under its old id"
    assert up[0] not in got[0][0].tolist() and c.topk[2][0] not in got[0][2].tolist()
    assert np.array_equal(got[0][8:16, 0], near), "the rows added next to queries 8 .. 15"

    # ---- an explicit rebase: export_live, a new base built from the exported rows (base rows keep their codes and
    # leaves, delta rows get the frozen model's: tests/fold_model.py), rebase under strictly ascending base_ids that
    # are not the identity -- external ids now cross 64-bit words and 1024-point ranges at other places than datapoint
    # indices do, and a user bitmap goes through live_and_user_gather_kernel
    er, ei = p.mut.export_live()
    if c.kind == "ah":
        ix = dict(kind="ah", codebook=c.cb, codes=c.codes)
    else:
        ix = dict(kind="txh", centers=c.kw["centers"], leaf_off=c.kw["leaf_offsets"], leaf_ids=c.kw["leaf_ids"],
                  codebook=c.cb, codes=c.kw["codes"], use_residuals=True, P=P, mult=M / K)
    f = fm.fold(p.model, ix)
    assert np.array_equal(ei, f["base_ids"]) and np.array_equal(er.view(np.uint32), f["rows"].view(np.uint32))
    assert np.all(np.diff(ei.astype(np.int64)) > 0) and not np.array_equal(ei, np.arange(ei.size))
    n2 = ei.size
    if c.kind == "ah":
        kw2, oix2, codes2 = H.ah_kwargs_from_codes(f["rows"], c.cb, f["codes"]), None, f["codes"]
    else:
        data, stride = orc.to_strided(f["rows"])
        oix2 = orc.TxhIndex(data, stride, c.dim, f["centers"], f["leaf_off"], f["leaf_ids"], c.cb, f["codes"],
                            use_residuals=True, partitions_to_search=P, pre_reorder_multiplier=M / K)
        kw2 = dict(c.kw, data=data, n_rows=n2, stride=stride, leaf_offsets=f["leaf_off"], leaf_ids=f["leaf_ids"],
                   codes=f["codes"])
        codes2 = None
    base2 = hip.txh_create(**kw2)
    base2.enable_timing(True)
    p.mut.rebase(base2, ei)
    fm.apply(p.model, f)
    p.same_counters()
    assert p.mut.pending() == 0 and not p.model.identity
    rm2, near2 = mutate_again(p, c, ei)
    # (the filters take the removed ids of both rounds: all of them are gone now)
    _searches(p, Rebased(c, n2), base2, oix2, codes2, kw2, np.concatenate([rm, rm2]), "rebased", name, bitmap, expected)
    got = p.mut.search_batched(c.q, K, opts=c.opts())
    assert np.array_equal(got[0][20:24, 0], near2)
    p.close()


class Rebased:
    """the Case behind a rebased base: its queries, opts and codebook, the new row count"""

    def __init__(self, c, n):
        self.kind, self.q, self.cb, self.dim, self.opts, self.n = c.kind, c.q, c.cb, c.dim, c.opts, n


@pytest.mark.parametrize("scan", sorted(FLAT_SCANS))
def test_flat_hasher_base(cases, scan, monkeypatch):
    c, expected = cases("ah")
    assert c.n % 1024 == 37 and c.q.shape[0] == 65 and H.sample_rank(M, c.st) < M   # a statistical bound
    _run(c, expected, scan, monkeypatch)


@pytest.mark.parametrize("scan", sorted(TREE_SCANS))
def test_tree_base(cases, scan, monkeypatch):
    c, expected = cases("txh")
    _run(c, expected, scan, monkeypatch)

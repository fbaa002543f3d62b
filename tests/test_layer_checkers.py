"""CPU checks of the checkers behind tests/test_gpu_layers_*.py: each one accepts the model's own answer, and raises
when two rows of different distance are swapped in it and when an id the layer had removed (a tombstoned row, a row
the filter disallows, a row over its crowd's limit) is put back.  And the seed / tie premises of those GPU tests that
need no GPU: the oracle rows reference (B) of the diversify tests reads are tie-free at depth + 1.

No GPU and no library: the answers handed to the checkers are made from the oracle and the models."""
import numpy as np
import pytest

import crowding_model as CM
import diversify_model as DM
import helpers as H
import mutable_model as mm
from oracle import pyoracle as orc
from test_gpu_crowding import check_rows
from test_gpu_diversify import check_against
from test_gpu_filters import Case, K, M
from test_gpu_mutable import check_lists

EMPTY = 0xFFFFFFFF


def _rows(want, k):
    """(idx, dist, cnt) arrays, as a search returns them, of per-query (ids, dists)"""
    nq = len(want)
    idx = np.full((nq, k), EMPTY, np.uint32)
    dist = np.full((nq, k), np.inf, np.float32)
    cnt = np.zeros(nq, np.uint32)
    for i, (wi, wd) in enumerate(want):
        idx[i, :wi.size], dist[i, :wi.size], cnt[i] = wi, wd, wi.size
    return idx, dist, cnt


def _swapped(got, i=0, a=2, b=3):
    """rows a and b of query i change places (ids and distances: the row is no longer sorted), and ids alone"""
    both = tuple(x.copy() for x in got)
    for x in both[:2]:
        x[i, [a, b]] = x[i, [b, a]]
    ids = tuple(x.copy() for x in got)
    ids[0][i, [a, b]] = ids[0][i, [b, a]]
    assert got[1][i, a] != got[1][i, b]
    return both, ids


def _refused(check, answers):
    for got in answers:
        with pytest.raises(AssertionError):
            check(got)


@pytest.fixture(scope="module")
def flat():
    return Case("ah", 8, n=1500, nq=6)


@pytest.fixture(scope="module")
def tree():
    return Case("txh", 8, n=3000, nq=6)


# ---- section 1: check_lists against the mutable model --------------------------------------------------------------
def test_check_lists_refuses_a_swap_and_a_removed_id(flat):
    c = flat
    rows = np.ascontiguousarray(c.data.reshape(c.n, c.stride)[:, :c.dim])
    model = mm.MutableModel(rows, 64)
    before = model.search_ah(c.cb, c.codes, c.q, K, M)
    top = int(before[0][0][0])
    model.remove([top, 7, 64])
    model.add(c.q[1] + np.float32(1e-3))
    want = model.search_ah(c.cb, c.codes, c.q, K, M)
    assert top not in want[0][0].tolist()
    good = _rows(want, K)
    check_lists(good, want, K, "good")
    put_back = _rows([before[0]] + want[1:], K)          # query 0 answers as if its top row had not been removed
    _refused(lambda got: check_lists(got, want, K, "bad"), list(_swapped(good)) + [put_back])
    short = tuple(x.copy() for x in good)                  # a row that lost its last entry
    short[0][2, K - 1], short[1][2, K - 1], short[2][2] = EMPTY, np.inf, K - 1
    _refused(lambda got: check_lists(got, want, K, "bad"), [short])


# ---- sections 1 and 2: Case.check (check_ah_query / check_txh_query under a filter) ----------------------------------
def _staged(c, words, cap):
    """the oracle's staged outputs under the filter, shaped as search_batched(stages=True) returns them"""
    nq = c.q.shape[0]
    allowed = H.allowed_ids(words, cap, c.n)
    P = c.tokens.shape[1]
    idx, dist, cnt = np.full((nq, K), EMPTY, np.uint32), np.full((nq, K), np.inf, np.float32), np.zeros(nq, np.uint32)
    tok, tokd = np.zeros((nq, P), np.uint32), np.zeros((nq, P), np.float32)
    ci, cd, cc = np.zeros((nq, M), np.uint32), np.zeros((nq, M), np.float32), np.zeros(nq, np.uint32)
    for i in range(nq):
        if c.kind == "ah":
            sub_codes = np.ascontiguousarray(c.codes[allowed])
            sub_data = np.ascontiguousarray(c.data.reshape(c.n, c.stride)[allowed])
            oci, ocd = orc.ah_search(c.cb, sub_codes, c.q[i], M)
            oi, od = orc.ah_search_with_reordering(c.cb, sub_codes, sub_data, c.stride, c.q[i], K, M)
            oci, oi = allowed[oci], allowed[oi]
        else:
            c.oix.allow = H.masked_words(words, cap, c.n)
            try:
                oi, od, otok, otokd, oci, ocd = orc.txh_search(c.oix, c.q[i], K, stages=True)
            finally:
                c.oix.allow = None
            tok[i], tokd[i] = otok, otokd
        idx[i, :oi.size], dist[i, :oi.size], cnt[i] = oi, od, oi.size
        ci[i, :oci.size], cd[i, :oci.size], cc[i] = oci, ocd, oci.size
    return idx, dist, cnt, (tok, tokd, ci, cd, cc)


@pytest.mark.parametrize("kind", ["ah", "txh"])
def test_case_check_refuses_a_swap_and_a_disallowed_id(kind, flat, tree):
    c = flat if kind == "ah" else tree
    words, cap = c.family("f50")
    good = _staged(c, words, cap)
    qs = range(c.q.shape[0])
    c.check(c.q, words, cap, good, qs, "good")
    assert np.all(good[2] == K)
    both, ids = _swapped(good[:3])
    disallowed = np.setdiff1d(np.arange(c.n), H.allowed_ids(words, cap, c.n))
    back = tuple(x.copy() for x in good[:3])
    back[0][0, K - 1] = disallowed[0]
    cand = tuple(x.copy() for x in good[3])
    cand[2][0, 5] = disallowed[1]                           # a disallowed row among the candidates
    answers = [both + (good[3],), ids + (good[3],), back + (good[3],), good[:3] + (cand,)]
    _refused(lambda got: c.check(c.q, words, cap, got, qs, "bad"), answers)


# ---- section 3: check_rows and check_against against the crowding / MMR models -------------------------------------
def _depth_rows(c, depth):
    rows = []
    for i in range(c.q.shape[0]):
        oi, od = orc.ah_search_with_reordering(c.cb, c.codes, c.data, c.stride, c.q[i], depth, 3 * depth)
        assert np.all(np.diff(od) > 0)
        rows.append((oi, od))
    return rows


def test_check_rows_refuses_a_swap_and_a_row_over_the_limit(flat):
    c, depth, nq = flat, 40, flat.q.shape[0]
    rows = _depth_rows(c, depth)
    attrs = np.arange(c.n, dtype=np.uint64) % np.uint64(3)
    want = [CM.apply_fast(ri, rd, attrs, 2, K) for ri, rd in rows]
    assert all(wi.size == 6 for wi, _ in want)
    good = _rows(want, K)
    check = lambda got: check_rows(got, lambda i: rows[i], attrs, 2, K, nq, "checker")
    check(good)
    # a row the limit had dropped is put back: the first three of the plain row always hold a third of some attribute
    over = [CM.apply_fast(ri, rd, attrs, 3, K) for ri, rd in rows]
    _refused(check, list(_swapped(good)) + [_rows([over[0]] + want[1:], K)])


def test_check_against_refuses_a_swap_and_a_row_over_the_limit(flat):
    c, depth, nq = flat, 40, flat.q.shape[0]
    rows = _depth_rows(c, depth)
    i = np.arange(c.n, dtype=np.uint64)
    attrs = np.stack([i % np.uint64(3), i % np.uint64(5)])
    md = lambda lim: (lambda ri, rd: DM.md_apply(ri, rd, attrs, lim, K))
    good = _rows([md([2, 1])(*r) for r in rows], K)
    check = lambda got: check_against(got, nq, K, lambda q: rows[q], lambda q: rows[q], md([2, 1]), "checker")
    check(good)
    over = _rows([md([2, 2])(*rows[0])] + [md([2, 1])(*r) for r in rows[1:]], K)
    assert not np.array_equal(over[0][0], good[0][0])
    _refused(check, list(_swapped(good, a=1, b=2)) + [over])
    # MMR: rows come back in selection order, so "swapped" is two entries of the selection
    mmr = lambda ri, rd: DM.mmr_apply_rows(ri, rd, K, 0.5, c.data, c.stride, c.dim, orc.SQUARED_L2)[:2]
    good = _rows([mmr(*r) for r in rows], K)
    check = lambda got: check_against(got, nq, K, lambda q: rows[q], None, mmr, "checker")
    check(good)
    plain = _rows([(ri[:K], rd[:K]) for ri, rd in rows], K)      # no diversification at all: the rows MMR passed over
    assert not np.array_equal(plain[0], good[0])
    _refused(check, list(_swapped(good)) + [plain])


# ---- premises of the GPU tests that need no GPU ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ah", "txh"])
def test_the_diversify_seeds_give_tie_free_oracle_rows(kind):
    """reference (B) of tests/test_gpu_layers_diversify.py: 101 strictly increasing distances per query, unfiltered,
    under the shared filter and under every query's own"""
    import test_gpu_layers_diversify as D
    c = Case(kind, 32, **D.SHAPES[kind])
    nq = c.q.shape[0]
    D.oracle_rows(c)
    words, cap = c.family("f50", seed=D.SHARED_SEED)
    D.oracle_rows(c, allowed=H.allowed_ids(words, cap, c.n))
    D.oracle_rows(c, allowed=[H.allowed_ids(c.family("f50", seed=D.PER_QUERY_SEED + i)[0], c.n, c.n) for i in range(nq)])


def test_the_mutable_script_fits_its_shapes():
    """tests/test_gpu_layers_mutable.py on the model alone: the removal set holds the range edges and the tail range,
    the delta passes one tile, the filters' capacity ends inside the delta ids, and the model's rows are tie-free"""
    import test_gpu_layers_mutable as T
    from test_gpu_mutable import _no_ties

    class ModelOnly:
        def __init__(self, rows, capacity):
            self.model = mm.MutableModel(rows, capacity)
            self.add, self.remove, self.update = self.model.add, self.model.remove, self.model.update

    c = Case("ah", 32, n=4133, nq=65)
    p = ModelOnly(T._rows_of(c), T.CAPACITY)
    rm, up, near = T.mutate(p, c, 500)
    assert {1023, 1024, 4095, 4096, 4128, 4132} <= set(rm.tolist()) and rm.size == c.n // 20
    assert sum(1 for i in rm if i >= 4096) >= 3
    codes = c.codes
    for phase in ("script", "rebased"):
        for name, words, cap in T._filters(p, rm):
            want = p.model.search_ah(c.cb, codes, c.q, K, M, words, cap)
            _no_ties(want)
            assert all(wi.size == (0 if name == "only removed" else K) for wi, _ in want), (phase, name)
        if phase == "script":
            import fold_model as fm
            f = fm.fold(p.model, dict(kind="ah", codebook=c.cb, codes=c.codes))
            fm.apply(p.model, f)
            assert not p.model.identity
            codes = f["codes"]
            rm = np.concatenate([rm, T.mutate_again(p, c, f["base_ids"])[0]])

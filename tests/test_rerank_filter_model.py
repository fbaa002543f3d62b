"""CPU tests of tests/rerank_filter_model.py on the row families of tests/helpers.py rerank_rows: the bracket of the
re-rank row filter holds around the oracle's exact f32 distance for every row store, each of its three parts is needed
by some family, a candidate whose d~ overflowed gets an unbounded bracket whatever the sign of the NaN, and the
selection rules keep the exact top k."""
import numpy as np
import pytest

from oracle import pyoracle as orc
from tests import helpers as H
from tests import rerank_filter_model as RM

N, DIM, NQ = 9000, 64, 24
STORES = ("i8-row", "i8-one", "fp8")


@pytest.fixture(scope="module")
def fam():
    cache = {}

    def get(family):
        if family not in cache:
            cache[family] = H.rerank_rows(family, N, DIM, NQ, seed=5)
        return cache[family]

    yield get
    cache.clear()


def _exact(rows, q):
    data, stride = orc.to_strided(rows)
    return orc.one_to_many(q, data, stride, rows.shape[0], 0)


def _failures(d, store, qs, **kw):
    st = RM.make_store(store, d["rows"])
    bad = 0
    for qi in qs:
        L, U = RM.bracket(RM.approx_distances(st, d["queries"][qi]), st.E, DIM, **kw)
        bad += int(RM.bracket_holds(L, U, _exact(d["rows"], d["queries"][qi])).sum())
    return bad


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("family", H.RERANK_FAMILIES)
def test_bracket_holds_in_float64(fam, family, store):
    """every row of the family (a superset of every candidate list) lies inside its bracket, for six queries"""
    d = fam(family)
    assert _failures(d, store, range(6)) == 0


@pytest.mark.parametrize("family,drop,store", [("permuted", "f32sum", "i8-row"), ("offset", "error", "i8-row"),
                                               ("duplicates", "error", "fp8"), ("tiny", "floor", "i8-row")])
def test_each_part_of_the_bracket_is_needed(fam, family, drop, store):
    """dropping one part of the slack breaks the bracket on the family built for it: the f32-sum term on permuted rows
    (x~ = x, the distances tie in real arithmetic), the 2 sqrt(d~) E + E^2 term wherever rows are quantised, the 1e-30
    floor on rows x 2^-70 (e^2 underflows to 0)"""
    d = fam(family)
    assert _failures(d, store, range(6)) == 0
    terms = tuple(t for t in RM.TERMS if t != drop)
    assert _failures(d, store, range(6), terms=terms) > 0


@pytest.mark.parametrize("nan_sign", [+1, -1])
@pytest.mark.parametrize("family", ["overflow-all", "overflow-most", "near-overflow"])
def test_overflowed_distance_gets_unbounded_bracket(fam, family, nan_sign):
    """d~ = +inf makes slack = +inf and L = inf - inf = NaN.  With the fix the bracket is (-inf, +inf) whichever sign
    the NaN has; without it, the positive NaN orders above every tau and the candidate leaves the shortlist, which
    then holds fewer than k rows (the defect), and the negative NaN orders below -inf (the candidate stays)."""
    d = fam(family)
    st = RM.make_store("i8-row", d["rows"])
    k = 10
    for qi in range(4):
        acc = RM.approx_distances(st, d["queries"][qi])
        over = np.isinf(acc)
        assert over.any()
        L, U = RM.bracket(acc, st.E, DIM, nan_sign=nan_sign)
        assert (L[over] == -np.inf).all() and (U[over] == np.inf).all()
        assert not np.isnan(L).any() and not np.isnan(U).any()
        keep = RM.shortlist(L, U, k)
        assert keep.sum() >= k and keep[over].all()
        Lb, Ub = RM.bracket(acc, st.E, DIM, nan_sign=nan_sign, overflow_fix=False)
        assert np.isnan(Lb[over]).all()
        kb = RM.shortlist(Lb, Ub, k)
        if nan_sign > 0:
            assert not kb[over].any()
            if family != "near-overflow":
                assert kb.sum() < k and RM.final_path(int(kb.sum()), acc.size, k) == "unfiltered"
        else:
            assert kb[over].all()


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("family", [f for f in H.RERANK_FAMILIES if f != "nonfinite"])
def test_filter_keeps_the_exact_top_k(fam, family, store):
    """the model's pipeline on the oracle's candidate lists: tau, shortlist, the k best of the shortlist by (exact, key)
    equal the k best of all candidates; the predicted paths are the ones the GPU tests count on"""
    d = fam(family)
    st = RM.make_store(store, d["rows"])
    for k, m in ((1, 8), (10, 1025), (10, 8192)):
        for qi in range(3):
            q = d["queries"][qi]
            ci, _ = orc.ah_search(d["codebook"], d["codes"], q, m)
            acc = RM.approx_distances(st, q, ci)
            L, U = RM.bracket(acc, st.E[ci], DIM)
            ex = _exact(d["rows"], q)[ci]
            keys = np.arange(ci.size, dtype=np.uint64)   # candidate order = merge-key order
            keep = RM.shortlist(L, U, k)
            want = RM.topk_by_exact_key(ex, keys, k)
            got = np.nonzero(keep)[0][RM.topk_by_exact_key(ex[keep], keys[keep], k)]
            assert np.array_equal(got, want), (family, store, k, m, qi)
            path = RM.final_path(int(keep.sum()), ci.size, k)
            if family == "offset":
                assert keep.all() and path == ("fast" if m <= RM.SHORT_MAX_FAST else "fallback")
            if family == "duplicates" and store == "i8-row" and m == 8192:
                assert keep.sum() <= RM.SHORT_MAX_FAST // 4 and path == "fast"


def test_overflow_all_returns_first_k_candidates(fam):
    """every exact distance is +inf: the k best by (exact, key) are the first k candidates, in order"""
    d = fam("overflow-all")
    q = d["queries"][0]
    ci, _ = orc.ah_search(d["codebook"], d["codes"], q, 512)
    oi, od = orc.ah_search_with_reordering(d["codebook"], d["codes"], *orc.to_strided(d["rows"]), q, 10, 512)
    assert np.isinf(od).all() and np.array_equal(oi, ci[:10])


def test_uniform_store_rule():
    """one scale for rows whose largest scale is within 2 % of the mean (every row finite), per-row scales otherwise;
    under one scale every row's E is the largest ||x - x~||"""
    rng = np.random.default_rng(3)
    x = rng.uniform(-1.0, 1.0, (4000, 32)).astype(np.float32)
    x[:, 0] = 1.0
    one = RM.i8_store_chosen(x)
    assert one.uniform and np.all(one.deq == one.deq[0]) and np.all(one.E == one.E.max())
    two = x.copy()
    two[::2] *= np.float32(2.0)
    assert not RM.i8_store_chosen(two).uniform
    assert RM.i8_store_chosen(two, mode=2).uniform
    assert not RM.i8_store_chosen(two, mode=0).uniform
    bad = x.copy()
    bad[5, 3] = np.inf
    assert not RM.i8_store_chosen(bad, mode=2).uniform
    # the one-scale error bound still brackets every row
    q = rng.uniform(-1.0, 1.0, 32).astype(np.float32)
    st = RM.i8_store_chosen(two, mode=2)
    L, U = RM.bracket(RM.approx_distances(st, q), st.E, 32)
    assert not RM.bracket_holds(L, U, _exact(two, q)).any()


@pytest.mark.parametrize("family", ["offset", "overflow-most", "duplicates", "permuted", "nonfinite"])
def test_local_prune_rule(fam, family):
    """the local stage's rule on key-ordered lists: the first 256 entries are always kept, and every pruned entry is
    dominated by k of them in (exact, key) order"""
    d = fam(family)
    st = RM.make_store("i8-row", d["rows"])
    k = 10
    for qi in range(4):
        q = d["queries"][qi]
        ci, _ = orc.ah_search(d["codebook"], d["codes"], q, 1500)
        L, U = RM.bracket(RM.approx_distances(st, q, ci), st.E[ci], DIM)
        keep = RM.shortlist(L, U, k, head=RM.LOCAL_HEAD)
        assert keep[:RM.LOCAL_HEAD].all()
        ex = _exact(d["rows"], q)[ci]
        assert RM.pruned_dominated(ex, np.arange(ci.size), ~keep, k) == []
        if family in ("duplicates", "permuted"):
            assert (~keep).sum() > 0 or family == "permuted"


def test_filter_conditions():
    assert RM.filter_applies(64) and RM.filter_applies(144) and not RM.filter_applies(40)
    assert not RM.filter_applies(64, measure=2)

"""CPU tests of tests/rerank_expand_model.py: the expanded bracket of the int8 row filter holds in float64 around the
oracle's exact f32 distance on every row family, at the dims where the kernel changes path (16: one lane of eight,
128: one full pass, 144 / 272: a partial last pass, 272 also beyond the register forms), with per-row scales and with
one scale; its cancellation term B is needed; and it shortlists no more than the per-dimension bracket does + 10 %."""
import numpy as np
import pytest

from oracle import pyoracle as orc
from tests import rerank_expand_model as XM
from tests import rerank_filter_model as RM

N, NQ = 3000, 9
DIMS = (16, 128, 144, 272)
STORES = ("i8-row", "i8-one")


@pytest.fixture(scope="module")
def fam():
    cache = {}

    def get(family, dim):
        if (family, dim) not in cache:
            d = XM.expand_rows(family, N, dim, NQ, seed=5)
            data, stride = orc.to_strided(d["rows"])
            d["exact"] = np.stack([orc.one_to_many(q, data, stride, N, 0) for q in d["queries"]])
            cache[family, dim] = d
        return cache[family, dim]

    yield get
    cache.clear()


def _failures(d, store, dim, **kw):
    st = RM.make_store(store, d["rows"])
    bad = 0
    for qi in range(NQ):
        acc, B = XM.expanded(st, d["queries"][qi])
        L, U = XM.bracket(acc, st.E, B, dim, **kw)
        assert not np.isnan(L).any() and not np.isnan(U).any()
        bad += int(RM.bracket_holds(L, U, d["exact"][qi]).sum())
    return bad


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("family", XM.FAMILIES)
def test_expanded_bracket_holds_in_float64(fam, family, dim, store):
    """L <= exact <= U for every row of the family (a superset of every candidate list) and every query"""
    assert _failures(fam(family, dim), store, dim) == 0


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("dim", DIMS)
def test_cancellation_term_is_needed(fam, dim, store):
    """without B the bracket of a row next to its query is narrower than the rounding of Q2 - 2 s D + s^2 N"""
    d = fam("cancel", dim)
    terms = tuple(t for t in XM.TERMS if t != "cancel")
    assert _failures(d, store, dim, terms=terms) > 0


def test_offset_family_shortlists_everything(fam):
    """|q|^2 >> d: B is wider than the candidates' spread, as the per-dimension bracket already was"""
    d = fam("offset", 128)
    st = RM.make_store("i8-row", d["rows"])
    for qi in range(3):
        acc, B = XM.expanded(st, d["queries"][qi])
        L, U = XM.bracket(acc, st.E, B, 128)
        assert RM.shortlist(L, U, 10).all()


@pytest.mark.parametrize("store", STORES)
def test_shortlist_is_at_most_a_tenth_longer(store):
    """uniform rows, lists of 5000 candidates, k = 10: the expanded bracket keeps at most 1.1 x the rows that the
    per-dimension bracket keeps (a cap: B is ~ 1 % of the quantisation term there)"""
    rng = np.random.default_rng(77)
    dim, n = 128, 5000
    rows = rng.uniform(-1.0, 1.0, (n, dim)).astype(np.float32)
    st = RM.make_store(store, rows)
    for qi in range(6):
        q = rng.uniform(-1.0, 1.0, dim).astype(np.float32)
        Lo, Uo = RM.bracket(RM.approx_distances(st, q), st.E, dim)
        acc, B = XM.expanded(st, q)
        Ln, Un = XM.bracket(acc, st.E, B, dim)
        old, new = int(RM.shortlist(Lo, Uo, 10).sum()), int(RM.shortlist(Ln, Un, 10).sum())
        print("query %d: shortlist %d rows per dimension, %d expanded" % (qi, old, new))
        assert 10 <= new <= 1.1 * old


def test_ordered_round_trip():
    v = np.array([-np.inf, -3.5, -0.0, 0.0, 1e-30, 7.0, np.inf], np.float32)
    assert np.array_equal(XM.from_ordered(RM.ordered(v)).view(np.uint32), v.view(np.uint32))

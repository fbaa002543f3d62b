"""Sparse brute force (hip.SparseIndex) against the numpy model of tests/sparse_model.py, bit for bit:
the scan alone through `distances`, then selection, the tie rule, the filter and the argument checks.

Values are uniform in [-1, 1] with both signs (a wrong summation order shows in the last bits) and about 5 % of the
stored values are exactly 0 (Jaccard and NonZeroIntersect then differ).  The scan case draws its row lengths from
{0, 1, 2, 63, 64, 65, 130} -- empty rows, a fetch boundary inside a row, rows longer than a fetch -- over D = 160
dimensions: a strictly ascending row of 130 entries needs at least 130 of them, so D = 64 cannot hold these lengths.
Queries of 20 to 60 of the 160 dimensions keep the overlap dense: a tile's union covers nearly all of them, so nearly
every element hits."""
import functools

import numpy as np
import pytest

from scann_rust_amd import hip
from tests import sparse_model as M

pytestmark = pytest.mark.gpu

MEASURES = [hip.DOT_PRODUCT, hip.COSINE, hip.SPARSE_JACCARD, hip.SPARSE_DICE, hip.SPARSE_NONZERO_INTERSECT]
measures = pytest.mark.parametrize("measure", MEASURES)


def lists(rng, lengths, pool):
    """one (dims, vals) pair per length: dims drawn ascending from `pool`, values in [-1, 1], 5 % exactly 0"""
    out = []
    for ln in lengths:
        v = rng.uniform(-1, 1, ln).astype(np.float32)
        v[rng.random(ln) < 0.05] = 0
        out.append((np.sort(rng.choice(pool, ln, replace=False)).astype(np.uint32), v))
    return M.csr(out)


def same_bits(got, want):
    assert got.shape == want.shape
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert bad.size == 0, "%d of %d differ, first at %d: %r != %r" % (bad.size, got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


def check_scan(measure, rows, queries, D):
    ix = hip.SparseIndex(*rows, dimensionality=D, measure=measure)
    try:
        same_bits(ix.distances(queries), M.distances(measure, rows, queries))
        return ix.last_plan()
    finally:
        ix.close()


@measures
@pytest.mark.parametrize("nq", [1, 17, 40])
def test_scan_bitwise(measure, nq):
    rng = np.random.default_rng(7)
    D = 160
    rows = lists(rng, rng.choice([0, 1, 2, 63, 64, 65, 130], 3000), np.arange(D))
    qlen = rng.integers(20, 61, nq)
    if nq > 1:
        qlen[[3, nq - 1]] = 0
    plan = check_scan(measure, rows, lists(rng, qlen, np.arange(D)), D)
    assert plan["tiles"] == -(-nq // hip.SPARSE_TILE_QUERIES) and plan["chunks"] == 2


@measures
def test_map_collisions_large_d(measure):
    """every query dimension has the same home in the map: each insert and each probe walks the chain; the rows also
    hold dimensions that share that home, or fall inside the chain, and are in no query"""
    rng = np.random.default_rng(11)
    D, S = 1 << 20, hip.SPARSE_MAP_SIZE
    chain = 5 + S * np.arange(D // S)
    in_q, absent = chain[::2], np.concatenate([chain[1::2], chain + 1, chain + 40])
    queries = lists(rng, rng.integers(30, 50, 20), in_q)
    rows = lists(rng, rng.integers(0, 60, 500), np.concatenate([in_q, absent]))
    check_scan(measure, rows, queries, D)


def test_tile_split_by_capacity():
    rng = np.random.default_rng(13)
    D = 4096
    rows = lists(rng, rng.integers(0, 100, 300), np.arange(D))
    plan = check_scan(hip.DOT_PRODUCT, rows, lists(rng, rng.integers(580, 620, 5), np.arange(D)), D)
    assert plan["tiles"] == 5
    ix = hip.SparseIndex(*rows, dimensionality=D)
    with pytest.raises(hip.ScannError) as e:
        ix.search_batched(lists(rng, [hip.SPARSE_TILE_SLOTS + 1], np.arange(D)), 3)
    assert e.value.code == hip.UNIMPLEMENTED
    ix.close()


@functools.lru_cache(maxsize=None)
def selection_data(n):
    rng = np.random.default_rng(17 + n)
    return lists(rng, rng.integers(0, 17, n), np.arange(5000)), lists(rng, np.concatenate([rng.integers(1, 30, 19), [0]]), np.arange(5000))


@pytest.fixture(scope="module")
def selection_case():
    """(measure, n) -> an index of n rows of about 8 entries over D = 5000, 20 queries and the model's distances: most
    rows share no dimension with a query and tie (at -0.0 for DotProduct).  Made once, closed with the module."""
    made = {}

    def get(measure, n):
        if (measure, n) not in made:
            rows, queries = selection_data(n)
            made[measure, n] = hip.SparseIndex(*rows, dimensionality=5000, measure=measure), queries, M.distances(measure, rows, queries)
        return made[measure, n]
    yield get
    for ix, _, _ in made.values():
        ix.close()


def check_search(case, measure, n, k, allow=None, allow_bits=None):
    ix, queries, dist = case(measure, n)
    idx, d, cnt = ix.search_batched(queries, k, allow=allow, allow_bits=allow_bits)
    allowed = None
    if allow is not None:
        bits = np.unpackbits(allow.view(np.uint8), bitorder="little")[:n].astype(bool)
        allowed = np.concatenate([bits, np.zeros(n - bits.size, bool)]) & (np.arange(n) < (n if allow_bits is None else allow_bits))
    widx, wd, wcnt = M.search(dist, k, allowed)
    assert np.array_equal(cnt, wcnt)
    assert np.array_equal(idx, widx)
    same_bits(d, wd)   # (slots past count: NaN of one bit pattern on both sides)
    return ix.last_plan()


@measures
@pytest.mark.parametrize("k", [1, 10, 256])
def test_selection_and_ties(selection_case, measure, k):
    assert check_search(selection_case, measure, 20000, k)["chunks"] > 1


@measures
def test_k_above_n(selection_case, measure):
    check_search(selection_case, measure, 50, 55)


@measures
@pytest.mark.parametrize("which", ["every_third", "none", "bits_below_n"])
def test_filter(selection_case, measure, which):
    n = 20000
    words = np.zeros((n + 63) // 64, np.uint64)
    bits = None
    if which == "every_third":
        np.bitwise_or.at(words, np.arange(0, n, 3) // 64, np.uint64(1) << (np.arange(0, n, 3) % 64).astype(np.uint64))
    elif which == "bits_below_n":
        words[:], bits = ~np.uint64(0), 7777
    check_search(selection_case, measure, n, 10, allow=words, allow_bits=bits)


def test_validation():
    f, u = np.float32, np.uint32
    good = dict(offsets=[0, 2, 4], dims=[1, 5, 0, 7], vals=[1, 2, 3, 4])
    bad = [dict(good, dims=[5, 1, 0, 7]), dict(good, dims=[1, 1, 0, 7]), dict(good, dims=[1, 5, 0, 8]),
           dict(good, vals=[1, np.nan, 3, 4]), dict(good, offsets=[0, 3, 2, 4], dims=[1, 5, 6, 7])]
    for kw in bad:
        with pytest.raises(hip.ScannError) as e:
            hip.SparseIndex(dimensionality=8, **kw)
        assert e.value.code == hip.INVALID_ARGUMENT, kw
    with pytest.raises(hip.ScannError) as e:
        hip.SparseIndex(dimensionality=8, measure=hip.SQUARED_L2, **good)
    assert e.value.code == hip.UNIMPLEMENTED
    ix = hip.SparseIndex(dimensionality=8, **good)
    for q in ([(u([2, 1]), f([1, 1]))], [(u([1, 1]), f([1, 1]))], [(u([8]), f([1]))], [(u([1]), f([np.inf]))]):
        with pytest.raises(hip.ScannError) as e:
            ix.search_batched(q, 1)
        assert e.value.code == hip.INVALID_ARGUMENT, q
    idx, dist, cnt = ix.search_batched([(u([1, 7]), f([1, 1]))], 2)
    assert idx.tolist() == [[1, 0]] and dist.tolist() == [[-4.0, -1.0]] and cnt.tolist() == [2]
    ix.close()
    empty = hip.SparseIndex(offsets=[0], dims=[], vals=[], dimensionality=8)
    idx, dist, cnt = empty.search_batched([(u([1]), f([1]))], 4)
    assert empty.size() == 0 and cnt.tolist() == [0] and empty.distances([(u([1]), f([1]))]).shape == (1, 0)
    assert idx.tolist() == [[0xFFFFFFFF] * 4] and dist.view(np.uint32).tolist() == [[0x7FFFFFFF] * 4]   # nothing launched: filled all the same
    empty.close()

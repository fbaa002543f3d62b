"""The posting-list route of sparse brute force (SparseIndex.build_postings) against the numpy model of
tests/sparse_model.py, bit for bit: sums that cross many lists and all waves' cuts, directory misses, the running top-k
across blocks and chunks, ties among untouched rows, the filter and the edges.  Data as in tests/test_gpu_sparse.py:
values in [-1, 1] of both signs, about 5 % exact zeros."""
import numpy as np
import pytest

from scann_rust_amd import hip
from tests import sparse_model as M
from tests.test_gpu_sparse import check_search, lists, measures, same_bits

pytestmark = pytest.mark.gpu
B = hip.SPARSE_BLOCK_ROWS


def check_scan(measure, rows, queries, D):
    ix = hip.SparseIndex(*rows, dimensionality=D, measure=measure, inverted=True)
    try:
        assert ix.postings_info()["blocks"] == -(-(rows[0].size - 1) // B)
        same_bits(ix.distances(queries), M.distances(measure, rows, queries))
    finally:
        ix.close()


def with_dim(row, d, present):
    dims, vals = row
    keep = dims != d
    dims, vals = dims[keep], vals[keep]
    if present:
        at = np.searchsorted(dims, d)
        dims, vals = np.insert(dims, at, d), np.insert(vals, at, np.float32(0.37))
    return dims.astype(np.uint32), vals


@pytest.fixture(scope="module")
def scan_rows():
    """2 B + 37 rows over D = 160: dimension 0 in every row of block 1 (a list of B postings: every wave's cut is full),
    dimension 159 in the first and the last row of block 0 alone (cuts empty for all waves but two)"""
    rng = np.random.default_rng(23)
    n = 2 * B + 37
    off, dims, vals = lists(rng, rng.choice([0, 1, 2, 63, 64, 65, 130], n), np.arange(160))
    rows = [(dims[off[i]:off[i + 1]], vals[off[i]:off[i + 1]]) for i in range(n)]
    for i in range(B, 2 * B):
        if rows[i][0].size == 0 or rows[i][0][0] != 0:
            rows[i] = with_dim(rows[i], 0, True)
    for i in range(B):
        if i in (0, B - 1) or (rows[i][0].size and rows[i][0][-1] == 159):
            rows[i] = with_dim(rows[i], 159, i in (0, B - 1))
    return M.csr(rows)


@measures
@pytest.mark.parametrize("nq", [1, 17])
def test_scan_bitwise(scan_rows, measure, nq):
    rng = np.random.default_rng(29 + nq)
    qlen = rng.integers(20, 61, nq)
    if nq > 1:
        qlen[[3, nq - 1]] = 0
    check_scan(measure, scan_rows, lists(rng, qlen, np.arange(160)), 160)


@measures
def test_directory_misses_large_d(measure):
    """query dimensions below every stored one, above every one, between stored ones, and stored ones"""
    rng = np.random.default_rng(31)
    D = 1 << 20
    stored = np.arange(5000, 900000, 64)
    rows = lists(rng, rng.integers(0, 60, 500), stored)
    pool = np.concatenate([np.arange(0, 5000, 97), np.arange(900000, D, 1001), stored[::3] + 1, stored[::2]])
    check_scan(measure, rows, lists(rng, rng.integers(30, 50, 20), pool), D)


@pytest.fixture(scope="module")
def selection_case():
    """(measure, n) -> an index with postings of n rows of exactly 4 entries over D = 5000 (one dimension per quarter:
    ascending by construction), 4 queries of at most 10 entries, the model's distances.  Most rows tie at -0.0."""
    made = {}

    def get(measure, n):
        if (measure, n) not in made:
            rng = np.random.default_rng(37 + n)
            dims = (np.arange(4) * 1250 + rng.integers(0, 1250, (n, 4))).astype(np.uint32).ravel()
            vals = rng.uniform(-1, 1, dims.size).astype(np.float32)
            vals[rng.random(dims.size) < 0.05] = 0
            rows = (np.arange(n + 1, dtype=np.uint64) * 4, dims, vals)
            queries = lists(rng, [10, 7, 1, 10], np.arange(5000))
            made[measure, n] = (hip.SparseIndex(*rows, dimensionality=5000, measure=measure, inverted=True), queries,
                                M.distances(measure, rows, queries))
        return made[measure, n]
    yield get
    for ix, _, _ in made.values():
        ix.close()


N = 34 * B + 5


@measures
@pytest.mark.parametrize("k", [1, 10, 256])
def test_selection_and_ties(selection_case, measure, k):
    assert check_search(selection_case, measure, N, k) == dict(tiles=0, chunks=0, elements=0, probes=0, hits=0)
    info = selection_case(measure, N)[0].postings_info()
    assert info["blocks"] == 35 and info["block_rows"] == B and 1 < info["chunks"] <= 35
    if k == 256:   # the merge bound forces chunks of more than one block: the top-k runs on across blocks
        assert info["chunks"] < info["blocks"]


@measures
@pytest.mark.parametrize("which", ["every_third", "none", "bits_inside_block_1"])
def test_filter(selection_case, measure, which):
    words = np.zeros((N + 63) // 64, np.uint64)
    bits = None
    if which == "every_third":
        np.bitwise_or.at(words, np.arange(0, N, 3) // 64, np.uint64(1) << (np.arange(0, N, 3) % 64).astype(np.uint64))
    elif which == "bits_inside_block_1":
        words[:], bits = ~np.uint64(0), B + 777
    check_search(selection_case, measure, N, 10, allow=words, allow_bits=bits)


@measures
def test_k_above_n_and_rebuild(selection_case, measure):
    check_search(selection_case, measure, 50, 55)
    ix, queries, _ = selection_case(measure, 50)
    before = ix.search_batched(queries, 7)
    ix.build_postings()   # idempotent
    for x, y in zip(before, ix.search_batched(queries, 7)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_empty_index_and_long_query():
    f, u = np.float32, np.uint32
    empty = hip.SparseIndex(offsets=[0], dims=[], vals=[], dimensionality=8, inverted=True)
    idx, dist, cnt = empty.search_batched([(u([1]), f([1]))], 4)
    assert empty.postings_info()["blocks"] == 0 and cnt.tolist() == [0]
    assert idx.tolist() == [[0xFFFFFFFF] * 4] and dist.view(u).tolist() == [[0x7FFFFFFF] * 4]
    empty.close()
    rng = np.random.default_rng(41)
    ix = hip.SparseIndex(*lists(rng, rng.integers(0, 100, 300), np.arange(4096)), dimensionality=4096, inverted=True)
    with pytest.raises(hip.ScannError) as e:
        ix.search_batched(lists(rng, [hip.SPARSE_TILE_SLOTS + 1], np.arange(4096)), 3)
    assert e.value.code == hip.UNIMPLEMENTED
    ix.close()

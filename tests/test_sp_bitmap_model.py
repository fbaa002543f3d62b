"""CPU-only: the (word, bit) -> point map of the sparse prefilter's survivor bitmap (tests/sp_bitmap_model.py) is a
bijection onto the 1024 points of a range, and it is the `jrel` expression of the kernels for every bit."""
import numpy as np

from tests import sp_bitmap_model as M


def _all_bits():
    w, b = np.meshgrid(np.arange(M.WORDS), np.arange(32), indexing="ij")
    return w.ravel(), b.ravel()


def test_the_map_is_a_bijection_onto_the_range():
    w, b = _all_bits()
    p = M.point_of(w, b)
    assert p.shape == (M.RANGE,)
    assert np.array_equal(np.sort(p), np.arange(M.RANGE))


def test_the_map_is_the_kernels_expression_for_every_bit():
    w, b = _all_bits()
    assert np.array_equal(M.point_of(w, b), M.jrel(w >> 1, w & 1, b))


def test_the_inverse_inverts_it():
    w, b = _all_bits()
    w2, b2 = M.word_bit_of(M.point_of(w, b))
    assert np.array_equal(w2, w) and np.array_equal(b2, b)


def test_a_tile_fills_one_half_of_two_words():
    """Tile t of a range owns the low (t even) or high (t odd) halves of words 2 (t >> 1) and 2 (t >> 1) + 1, lane half
    h taking the rows with (row >> 2) & 1 == h: what the tile loop's one store per two tiles writes."""
    for t in range(2 * M.TILE_PAIRS):
        w, b = M.word_bit_of(np.arange(t * 32, t * 32 + 32))
        assert set(w.tolist()) == {2 * (t >> 1), 2 * (t >> 1) + 1}
        assert np.all((b >> 4) == (t & 1))
        rows = np.arange(32)
        assert np.array_equal(w & 1, (rows >> 2) & 1)


def test_rows_round_trip_at_the_edges_of_a_range():
    """n = 4133 (a 37-point last range: 2 tiles, the second with 5 rows), 5120 (whole ranges), 6145 (a 1-point range)."""
    rng = np.random.default_rng(7)
    for n in (4133, 5120, 6145):
        pts = np.unique(np.concatenate([rng.integers(0, n, 60), [0, n - 1, (n - 1) // M.RANGE * M.RANGE]]))
        row = M.encode_row(pts, n)
        assert row.size == M.row_words(n) and row.size % M.WORDS == 0
        assert np.array_equal(M.decode_row(row), pts)
        # the words past the last item's live tile pairs stay zero
        last = n - (n - 1) // M.RANGE * M.RANGE
        dead = row[-M.WORDS:][2 * M.live_tile_pairs(last):]
        assert not dead.any()


def test_live_tile_pairs():
    assert [M.live_tile_pairs(x) for x in (1, 32, 33, 37, 64, 65, 1024)] == [1, 1, 1, 1, 1, 2, 16]

"""Numpy model of the survivor bitmap the sparse prefilter's 64-pair items store for a flat hasher
(txh_prefilter.hip sp_store_item_bits) and adc_refine_bits_kernel walks.

A query's row holds 32 words per range of 1024 points, in the order the tile loop keeps them in LDS: word w = 2 tt + h
is the word of tile pair tt (tiles 2 tt and 2 tt + 1 of the range, 32 points each) of lane half h.  Its low 16 bits are
the mask of tile 2 tt, its high 16 bits that of tile 2 tt + 1; result register r of a tile (MFMA row
(r & 3) + 8 (r >> 2) + 4 h) sits at bit 15 - r of its mask."""
import numpy as np

RANGE = 1024           # points per item (kSpRange64)
WORDS = 32             # words per (query, range)
TILE_PAIRS = 16        # tile pairs per item


def point_of(word, bit):
    """Point of the range that bit `bit` of word `word` stands for, built from the layout above (arrays or scalars)."""
    word, bit = np.asarray(word), np.asarray(bit)
    tt, h = word >> 1, word & 1
    tile = 2 * tt + (bit >> 4)              # low half: the even tile, high half: the odd one
    r = 15 - (bit & 15)                     # result register
    row = (r & 3) + 8 * (r >> 2) + 4 * h    # MFMA row of (register, lane half)
    return tile * 32 + row


def jrel(tt, h, bpos):
    """The expression of the kernels, as sp_flush_item_lanes and adc_refine_bits_kernel write it."""
    tt, h, bpos = np.asarray(tt), np.asarray(h), np.asarray(bpos)
    r = 15 - (bpos & 15)
    return (2 * tt + (bpos >> 4)) * 32 + 4 * h + (r & 3) + ((r >> 2) << 3)


def word_bit_of(point):
    """Inverse of point_of: (word, bit) of a point of the range."""
    point = np.asarray(point)
    tile, row = point >> 5, point & 31
    h = (row >> 2) & 1
    r = (row & 3) + 4 * (row >> 3)
    return 2 * (tile >> 1) + h, 16 * (tile & 1) + 15 - r


def row_words(n):
    """Words of a query's row over n points."""
    return (n + RANGE - 1) // RANGE * WORDS


def decode_row(words):
    """Points (ascending) whose bits are set in a query's row of uint32 words."""
    words = np.ascontiguousarray(words, np.uint32)
    w, b = np.nonzero((words[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1)
    return np.sort((w // WORDS) * RANGE + point_of(w % WORDS, b))


def encode_row(points, n):
    """A query's row over n points with exactly the bits of `points` set."""
    out = np.zeros(row_words(n), np.uint32)
    points = np.asarray(points, np.int64)
    w, b = word_bit_of(points % RANGE)
    np.bitwise_or.at(out, (points // RANGE) * WORDS + w, (np.uint32(1) << b.astype(np.uint32)))
    return out


def live_tile_pairs(npts):
    """Tile pairs an item of npts points writes; a row's words past them are zero."""
    return ((npts + 31) // 32 + 1) // 2

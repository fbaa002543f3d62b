"""High-precision statement of the index-build rules that have no bit-level oracle: the k-means++ seeding of
scann_hip_kmeans_init_pp (include/scann_hip.h).  The checker of tests/test_gpu_build.py.

The seeding rule, as the header documents it:

  random stream   splitmix64(seed): output 0 mod n is the first seed; every later seed c consumes two outputs in
                  order, u = (z >> 11) 2^-53 and fallback = z mod n
  min_d[i]        the smallest squared distance of row i to a chosen seed, in the reference's f32 arithmetic
                  (sequential scalar sum below simd_threshold dims, squared_l2_avx2's order with its unfused tail from
                  there on), updated with a strict '<' (a NaN minimum therefore stays)
  pick            the first row i whose cumulative sum C(i) = min_d[0] + ... + min_d[i] reaches u T, T = C(n - 1)
  T == 0          rows[fallback]
  T == +inf       the rule read in the extended reals: u T = +inf, and C(i) is +inf from the first infinite min_d on
  T is NaN        rows[fallback]  (the library's rule; the reference's loop would select row 0)

The library evaluates C and T in f64 with a reduction tree, so the model does NOT mirror its sums: it evaluates them
EXACTLY (every f32 is an integer multiple of 2^-149: Python integers) and admits every row that a correctly rounded
f64 evaluation in ANY summation order could pick.  A f64 sum of n non-negative terms, in any order, is within
(n - 1) 2^-53 of the exact sum, relatively; that applies once to T and once to the cumulative sum, and u T adds one
rounding: delta = (n + 1) 2^-52 covers all three.  Row i is admissible when

    min_d[i] > 0,   C(i) >= u T (1 - delta),   C(i - 1) < u T (1 + delta).

The band is a cap, not a tolerance: tests use inputs whose every band holds exactly one row and demand that row.
"""
import bisect
import ctypes as C
import itertools

import numpy as np

from oracle import pyoracle as orc
from scann_rust_amd import synth

SIMD_THRESHOLD = 128      # KMeansConfig::default().simd_threshold
_SUB_ULP_EXP = 149        # every f32 is a multiple of 2^-149


def _distance_fn(avx):
    """the oracle's single-pair SquaredL2 (addresses in, Python float out) in one of the two summation orders"""
    proto = C.CFUNCTYPE(C.c_float, C.c_void_p, C.c_void_p, C.c_size_t)
    return proto(("or_squared_l2_avx2" if avx else "or_squared_l2_sequential", orc.lib()))


def distances_to_row(window, j, avx):
    """[n] f32: the reference's squared distance of every row of `window` (C-contiguous [n, sub] f32) to row j"""
    n, sub = window.shape
    fn = _distance_fn(avx)
    base, step = window.ctypes.data, sub * 4
    cj = base + j * step
    return np.fromiter((fn(base + i * step, cj, sub) for i in range(n)), np.float32, n)


def exact_units(v):
    """Python integers: the finite non-negative f32 values v in units of 2^-149 (exact)"""
    m, e = np.frexp(np.asarray(v, np.float64))          # v = m 2^e, m in [0.5, 1) or 0
    mi = (m * float(1 << 24)).astype(np.int64)          # 24 significant bits: exact
    sh = (e.astype(np.int64) - 24 + _SUB_ULP_EXP)
    out = []
    for a, s in zip(mi.tolist(), sh.tolist()):
        out.append(a << s if s >= 0 else a >> -s)       # (a subnormal's low bits are zero: the shift is exact)
    return out


def stream(seed, n, k):
    """(first, [(u_int, fallback)] for seeds 1 .. k-1): u = u_int 2^-53"""
    z = synth.splitmix64(seed, 0, 2 * k - 1)
    first = int(z[0] % np.uint64(n))
    rest = [(int(z[2 * c - 1] >> np.uint64(11)), int(z[2 * c] % np.uint64(n))) for c in range(1, k)]
    return first, rest


def band(min_d, u_int, fallback):
    """(rows, kind): the admissible rows of one pick and the branch of the rule that produced them"""
    n = min_d.size
    if np.isnan(min_d).any():
        return np.array([fallback]), "nan-total"
    inf = np.flatnonzero(np.isinf(min_d))
    if inf.size:
        return inf[:1], "inf-total"
    cum = list(itertools.accumulate(exact_units(min_d)))
    T = cum[-1]
    if T == 0:
        return np.array([fallback]), "zero-total"
    # thr = u_int 2^-53 T; delta = (n + 1) 2^-52.  Compare C 2^105 with T u_int (2^52 -+ (n + 1)).
    lo = T * u_int * ((1 << 52) - (n + 1))
    hi = T * u_int * ((1 << 52) + (n + 1))
    scaled = _Scaled(cum, 105)
    i_lo = bisect.bisect_left(scaled, lo)                 # first i with C(i) >= thr (1 - delta)
    i_hi = bisect.bisect_left(scaled, hi)                 # first i with C(i) >= thr (1 + delta): C(i_hi - 1) < it
    i_hi = min(i_hi, n - 1)
    rows = np.arange(i_lo, i_hi + 1)
    return rows[min_d[rows] > 0], "sampled"


class _Scaled:
    """cum[i] << shift as a lazy sequence (bisect reads O(log n) of them)"""

    def __init__(self, cum, shift):
        self.cum, self.shift = cum, shift

    def __len__(self):
        return len(self.cum)

    def __getitem__(self, i):
        return self.cum[i] << self.shift


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32),
                          np.ascontiguousarray(b, np.float32).view(np.uint32))


def seeding_reference(rows_window, k, seed, simd_threshold=SIMD_THRESHOLD, picks=None):
    """The bands of the k seeds of `rows_window` ([n, sub] f32: the column window the seeding reads).

    picks None: the model follows its own picks (the first row of every band).  picks [k, sub] f32 (the centres a
    library returned): the model follows THOSE, so that every band is the one the library faced; a centre that is not
    in its band is still followed (through any row with its bits) and reported by the caller's comparison.

    Returns a list of k dicts: rows (the admissible row indices), kind ('first' | 'sampled' | 'zero-total' |
    'inf-total' | 'nan-total') and followed (the row index the model went on with, None if the pick is no row)."""
    win = np.ascontiguousarray(rows_window, np.float32)
    n, sub = win.shape
    avx = sub >= simd_threshold
    first, rest = stream(seed, n, k)
    out = []
    min_d = None
    for c in range(k):
        if c == 0:
            rows, kind = np.array([first]), "first"
        else:
            rows, kind = band(min_d, *rest[c - 1])
        follow = int(rows[0]) if rows.size else None
        if picks is not None:
            match = [int(i) for i in rows if same_bits(win[i], picks[c])]
            if match:
                follow = match[0]
            else:
                eq = np.flatnonzero((win.view(np.uint32) == np.ascontiguousarray(picks[c], np.float32)
                                     .view(np.uint32)[None]).all(1))
                follow = int(eq[0]) if eq.size else None
        out.append(dict(rows=rows, kind=kind, followed=follow))
        if follow is None:
            break                                          # the pick is no row: nothing to follow
        if c + 1 < k:
            d = distances_to_row(win, follow, avx)
            with np.errstate(invalid="ignore"):
                min_d = d if min_d is None else np.where(d < min_d, d, min_d)   # strict '<': a NaN minimum stays
    return out


# ---- the seeding inputs of tests/test_gpu_build.py (tests/test_build_model.py proves every band holds one row) ------
def _strided(rows, stride):
    n, dim = rows.shape
    data = np.zeros((n, stride), np.float32)
    data[:, :dim] = rows
    return data


def _clustered(n, dim, seed, clusters):
    return synth.clustered_f32(n, dim, seed, n_clusters=clusters)[0]


def seeding_case(name):
    """dict(data [n, stride] f32, n, dim, stride, col, sub, k, seed, thr) of one seeding input.  stride None in the
    table = the library's compute_stride(dim) (a multiple of 16); otherwise a tight stride."""
    from tests import helpers as H
    rng = np.random.default_rng([31, sorted(SEEDING_CASES).index(name)])
    thr, col, sub, stride, seed = SIMD_THRESHOLD, 0, None, None, 1000 + len(name)
    if name == "clustered":
        rows, k = _clustered(3000, 8, 21, 16), 16
    elif name == "uniform-70000":            # > 65 536 rows: the one-block pick's chunks hold two partials each
        rows, k = synth.uniform_f32(70000, 4, 22), 8
    elif name == "integers":                 # exact arithmetic, many zero and tied minimum distances
        rows, k = rng.integers(-3, 4, (2000, 16)).astype(np.float32), 12
    elif name == "copies":                   # k > the number of distinct rows: picks 26 .. 40 are fallback rows
        rows, k = np.tile(rng.uniform(-1.0, 1.0, (25, 6)).astype(np.float32), (600, 1)), 40
    elif name == "avx-tail-window":          # AVX2 order with a 3-wide tail, through an unaligned column window
        rows, k, col, sub = _clustered(1500, 140, 23, 10), 10, 5, 131
    elif name == "avx-tail-only":            # threshold 0 at 5 dims: no whole chunk, the unfused tail alone; odd stride
        rows, k, thr, stride = _clustered(2000, 5, 24, 9), 9, 0, 5
    elif name == "window-unaligned":
        rows, k, col, sub = _clustered(2500, 12, 25, 8), 8, 3, 7
    elif name == "tight-odd-stride":
        rows, k, stride = _clustered(2000, 7, 26, 8), 8, 7
    elif name == "one-row":                  # n = 1 (and k > n)
        rows, k = rng.uniform(-1.0, 1.0, (1, 3)).astype(np.float32), 3
    elif name == "one-seed":
        rows, k = _clustered(500, 8, 27, 4), 1
    elif name == "more-seeds-than-rows":
        rows, k = rng.uniform(-1.0, 1.0, (5, 4)).astype(np.float32), 9
    elif name == "all-zero":
        rows, k = np.zeros((300, 4), np.float32), 5
    elif name == "all-equal":
        rows, k = H.build_rows("all-equal", 300, 4, 28), 5
    elif name == "overflow":                 # an infinite total: the first infinite min_d row
        rows, k = H.build_rows("overflow", 1000, 8, 29), 7
    elif name == "scaled-70":                # subnormal minimum distances
        rows, k = H.build_rows("scaled-70", 1000, 8, 30), 6
    elif name == "avx-tail-subnormal":       # AVX2 order, tail only, squared differences of 3 significant bits
        rows = H.build_rows("signed", 2000, 5, 32) * np.float32(2.0 ** -73)
        k, thr, stride = 8, 0, 5
    elif name == "nan":                      # a NaN total: every later pick is the fallback draw
        rows, k = H.build_rows("nan", 400, 8, 31), 6
    else:
        raise ValueError(name)
    n, dim = rows.shape
    st = int(orc.compute_stride(dim)) if stride is None else stride
    sub = dim if sub is None else sub
    return dict(data=_strided(rows, st), n=n, dim=dim, stride=st, col=col, sub=sub, k=k, seed=seed, thr=thr)


SEEDING_CASES = ("clustered", "uniform-70000", "integers", "copies", "avx-tail-window", "avx-tail-only",
                 "window-unaligned", "tight-odd-stride", "one-row", "one-seed", "more-seeds-than-rows", "all-zero",
                 "all-equal", "overflow", "scaled-70", "nan", "avx-tail-subnormal")


def seeding_window(case):
    return np.ascontiguousarray(case["data"][:, case["col"]:case["col"] + case["sub"]])


"""The index-build kernels on adversarial data, at every kernel path: scann_hip_bf_assign_nearest, scann_hip_kmeans_lloyd,
scann_hip_kmeans_init_pp, scann_hip_encode and the plain scann_hip_lut_from_query.

Every output of every row is compared bitwise with the CPU oracle (orc.partition, orc.kmeans_lloyd, orc.encode_many,
orc.lut_from_query); NaN outputs compare by position (a NaN's payload is not part of the contract).  The k-means++
seeds, which have no bit-level oracle, are compared with the high-precision reference of tests/build_model.py: every
input's admissible band holds exactly one row (tests/test_build_model.py proves it on the CPU), so the seeds must equal
those rows.

Shapes are the smallest that cross a boundary of the kernels: the 16- and 8-centre LDS tiles (15/16/17, 7/8/9), the
256-row block (255/256/257), the 32-value register slab and the float4 loads (dims 1..100, strides that are no multiple
of 4, unaligned column windows), the narrow/wide switch of km_update_kernel (63/64/65) and its 256-dimension slabs
(257, 300, 513), clusters longer than an LDS tile, the one-block pick's two-partial chunks (70 000 rows), encode's
grid-stride wrap (n S > 4 194 304) and the 160 KB LDS limit."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as orc
from scann_rust_amd import hip, synth, trainer
from tests import build_model as BM
from tests import helpers as H

pytestmark = pytest.mark.gpu

SEQ, AVX = 1 << 30, 0          # simd_threshold: never / always the AVX2 summation order


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_f32(got, want, what=""):
    """bitwise equal, NaNs by position"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN positions differ" % what
    bad = np.flatnonzero((bits(got) != bits(want)).ravel() & ~nan.ravel())
    assert bad.size == 0, "%s: %d values differ, first at %d: %r vs %r" % (
        what, bad.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


def strided(rows, stride=None):
    """([n, stride] f32 zero-padded copy, stride): stride None = the library's compute_stride(dim)"""
    n, dim = rows.shape
    st = hip.compute_stride(dim) if stride is None else stride
    data = np.zeros((n, st), np.float32)
    data[:, :dim] = rows
    return data, st


def bf_index(rows, stride=None):
    data, st = strided(rows, stride)
    return hip.bf_create(data, rows.shape[0], rows.shape[1], st, hip.SQUARED_L2), data, st


# ---- scann_hip_bf_assign_nearest ------------------------------------------------------------------------------------
def nearest_reference(rows, centers):
    """(token [n], dist [n] f32) of TreePartitioner::partition(x, 1) for every row"""
    tok = np.empty(rows.shape[0], np.uint32)
    dist = np.empty(rows.shape[0], np.float32)
    for i, r in enumerate(rows):
        t, d = orc.partition(centers, r, 1)
        tok[i], dist[i] = t[0], d[0]
    return tok, dist


def check_assign(index, n, centers, want_tok, want_dist, what):
    tok, dist = hip.bf_assign_nearest(index, centers)
    assert np.array_equal(tok, want_tok[:n]), "%s: tokens differ at rows %s" % (
        what, np.flatnonzero(tok != want_tok[:n])[:8])
    # a row whose every distance is NaN: the partitioner reports NaN, assign_clusters' min_dist stays +inf -- the
    # library's value is +inf (scann_hip.h)
    want = np.where(np.isnan(want_dist[:n]), np.float32(np.inf), want_dist[:n])
    assert np.array_equal(bits(dist), bits(want)), "%s: distances differ at rows %s" % (
        what, np.flatnonzero(bits(dist) != bits(want))[:8])
    assert np.array_equal(hip.bf_assign_nearest(index, centers, want_dist=False), tok), "%s: out_dist = NULL" % what


@pytest.mark.parametrize("k", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("dim,tight", [(1, False), (3, False), (7, False), (7, True), (31, False), (32, False),
                                       (33, False), (33, True), (64, False), (100, False)])
def test_assign_nearest_shape_grid(dim, tight, k):
    """every row of n = 1, 255, 256, 257 and 3000; tight = stride == dim (no multiple of 4: the non-vector loads)"""
    rows = H.build_rows("signed", 3000, dim, 100 + dim)
    centers = H.build_rows("signed", k, dim, 200 + dim + k)
    want_tok, want_dist = nearest_reference(rows, centers)
    for n in (1, 255, 256, 257, 3000):
        index, _, _ = bf_index(rows[:n], dim if tight else None)
        check_assign(index, n, centers, want_tok, want_dist, "n=%d" % n)
        index.close()


@pytest.mark.parametrize("dim,tight", [(7, True), (33, True), (33, False), (64, False)])
@pytest.mark.parametrize("family", H.BUILD_FAMILIES)
def test_assign_nearest_families(family, dim, tight):
    """centres drawn from the rows (distance 0 hits) with duplicated centres: NaN distances order last, every tie goes
    to the lowest centre index"""
    n, k = 700, 17
    rows = H.build_rows(family, n, dim, 300 + dim)
    centers = H.centers_from_rows(rows, k, 301)
    want_tok, want_dist = nearest_reference(rows, centers)
    index, _, _ = bf_index(rows, dim if tight else None)
    check_assign(index, n, centers, want_tok, want_dist, family)
    if family == "nan":
        whole = H.nan_whole_row(n)
        tok, dist = hip.bf_assign_nearest(index, centers)
        assert tok[whole] == 0 and np.isposinf(dist[whole]) and np.isnan(want_dist[whole])
    if family == "all-equal":
        assert not want_tok.any() and not want_dist.any()
    if family == "integers" and dim == 7:      # exact ties between DIFFERENT centres exist (and go to the lower index)
        d = ((rows[:, None, :].astype(np.float64) - centers[None].astype(np.float64)) ** 2).sum(2)
        assert any(len({centers[c].tobytes() for c in np.flatnonzero(r == r.min())}) > 1 for r in d)


# ---- scann_hip_kmeans_lloyd -----------------------------------------------------------------------------------------
def lloyd_raw(index, init, max_iterations, convergence_threshold, col, thr, null=()):
    """scann_hip_kmeans_lloyd with the outputs named in `null` passed as NULL"""
    c = np.array(init, np.float32, copy=True, order="C")
    k, sd = c.shape
    n = index.size()
    assign = np.zeros(n, np.uint32); sizes = np.zeros(k, np.uint32)
    inertia = C.c_double(-1.0); iters = C.c_uint32(99999); conv = C.c_int(-1)
    hip.check(hip.load().scann_hip_kmeans_lloyd(
        index.h, col, sd, hip.ptr(c, hip.f32p), k, max_iterations, C.c_double(convergence_threshold), thr,
        None if "assign" in null else hip.ptr(assign, hip.u32p), None if "sizes" in null else hip.ptr(sizes, hip.u32p),
        None if "inertia" in null else C.byref(inertia),
        None if "iterations" in null else C.cast(C.byref(iters), hip.u32p), None if "converged" in null else C.byref(conv)))
    return dict(centers=c, assign=assign, sizes=sizes, inertia=inertia.value, iterations=iters.value,
                converged=conv.value)


def check_lloyd(index, data, n, stride, init, col=0, thr=hip.KMEANS_SIMD_THRESHOLD, max_iterations=5,
                convergence_threshold=1e-5, what=""):
    """centres, assignment, sizes, the f64 inertia bits, the iteration count and the converged flag against the oracle;
    returns the oracle's tuple"""
    sub = init.shape[1]
    g = hip.kmeans_lloyd(index, init, max_iterations=max_iterations, convergence_threshold=convergence_threshold,
                         col_offset=col, simd_threshold=thr)
    o = orc.kmeans_lloyd(data, n, stride, sub, init, max_iterations=max_iterations,
                         convergence_threshold=convergence_threshold, col_offset=col, simd_threshold=thr)
    assert (g[4], g[5]) == (o[4], o[5]), "%s: iterations / converged %s vs %s" % (what, g[4:], o[4:])
    assert np.array_equal(g[1], o[1]), "%s: assignment differs at rows %s" % (what, np.flatnonzero(g[1] != o[1])[:8])
    assert np.array_equal(g[2], o[2]), "%s: sizes" % what
    assert_same_f32(g[0], o[0], what + " centres")
    gi, oi = np.float64(g[3]), np.float64(o[3])
    assert (np.isnan(gi) and np.isnan(oi)) or gi.view(np.uint64) == oi.view(np.uint64), \
        "%s: inertia %r vs %r" % (what, g[3], o[3])
    return o


def seeds_of(rows_window, k, seed):
    """k initial centres drawn from the window's rows by a fixed stream (distinct picks are not required)"""
    pick = (synth.splitmix64(seed, 0, k) % np.uint64(rows_window.shape[0])).astype(np.int64)
    return np.ascontiguousarray(rows_window[pick], np.float32)


@pytest.mark.parametrize("thr", [AVX, SEQ], ids=["avx", "seq"])
@pytest.mark.parametrize("sub", [1, 2, 63, 64, 65, 257, 300, 513])
def test_lloyd_sub_dims_both_orders(sub, thr):
    """the narrow / wide switch of km_update_kernel (63, 64, 65) and its second and third 256-dimension slab, in both
    summation orders; clusters of ~225 members span several LDS tiles in both branches"""
    n, k = 900, 4
    rows, _ = synth.clustered_f32(n, sub, 400 + sub, n_clusters=4)
    index, data, st = bf_index(rows)
    check_lloyd(index, data, n, st, seeds_of(rows, k, 7), thr=thr, what="sub %d" % sub)


@pytest.mark.parametrize("sub", [128, 131])
def test_lloyd_default_threshold(sub):
    n, k = 900, 5
    rows, _ = synth.clustered_f32(n, sub + 9, 420 + sub, n_clusters=5)
    index, data, st = bf_index(rows)
    check_lloyd(index, data, n, st, seeds_of(rows[:, 4:4 + sub], k, 8), col=4, what="sub %d" % sub)
    check_lloyd(index, data, n, st, seeds_of(rows[:, :127], k, 8), col=0, what="sub 127 (sequential)")


@pytest.mark.parametrize("thr", [AVX, SEQ], ids=["avx", "seq"])
@pytest.mark.parametrize("col", [0, 1, 5])
@pytest.mark.parametrize("tight", [False, True], ids=["padded", "tight-odd"])
def test_lloyd_column_windows_and_strides(tight, col, thr):
    """a 9- and a 19-wide window (one AVX2 chunk + a tail of 1, two chunks + 3) of 25-wide rows, at stride 32 and at
    the tight odd stride 25: aligned and unaligned windows, vector and non-vector loads"""
    n, dim, k = 800, 25, 6
    rows, _ = synth.clustered_f32(n, dim, 431, n_clusters=6)
    index, data, st = bf_index(rows, dim if tight else None)
    for sub in (9, 19):
        check_lloyd(index, data, n, st, seeds_of(rows[:, col:col + sub], k, 9), col=col, thr=thr,
                    what="col %d sub %d" % (col, sub))


@pytest.mark.parametrize("thr", [AVX, SEQ], ids=["avx", "seq"])
@pytest.mark.parametrize("n", [1, 255, 257])
def test_lloyd_few_rows_many_clusters(n, thr):
    """k = 1, n and n + 4: clusters c >= n start as copies of rows c % n, lose every tie and are empty (they take row
    c % n); 7, 8, 9 and 15, 16, 17 centres are the tile boundaries of the two assign kernels"""
    dim = 12
    rows = H.build_rows("signed", n, dim, 440 + n)
    index, data, st = bf_index(rows)
    for k in sorted({1, n, n + 4, 7, 8, 9, 15, 16, 17}):
        init = np.ascontiguousarray(rows[np.arange(k) % n])
        o = check_lloyd(index, data, n, st, init, thr=thr, max_iterations=3, what="n %d k %d" % (n, k))
        if k > n:
            assert not o[2][n:].any() and np.array_equal(bits(o[0][n:]), bits(rows[np.arange(n, k) % n]))


@pytest.mark.parametrize("sub", [3, 96])
def test_lloyd_one_cluster_holds_every_row(sub):
    """centres 1.. lie far away: cluster 0 holds all 6000 rows (many LDS tiles, in the narrow and in the wide branch
    of km_update_kernel) in the first update, every other cluster is empty there"""
    n, k = 6000, 5
    rows = H.build_rows("signed", n, sub, 450 + sub)
    index, data, st = bf_index(rows)
    init = np.full((k, sub), 1000.0, np.float32) * np.arange(k, dtype=np.float32)[:, None]
    for thr in (AVX, SEQ):
        o = check_lloyd(index, data, n, st, init, thr=thr, max_iterations=1, what="sub %d thr %d" % (sub, thr))
        # the one update saw all rows in cluster 0 (the oracle itself: their mean) and clusters 1.. empty: rows 1..
        assert np.allclose(o[0][0], rows.astype(np.float64).sum(0) / n, rtol=1e-6, atol=1e-9)
        assert np.array_equal(bits(o[0][1:]), bits(rows[1:k]))
        check_lloyd(index, data, n, st, init, thr=thr, max_iterations=0, what="sub %d thr %d: no update" % (sub, thr))
        check_lloyd(index, data, n, st, init, thr=thr, max_iterations=3, what="sub %d thr %d: 3 rounds" % (sub, thr))


def test_lloyd_iteration_and_convergence_settings():
    n, dim, k = 1500, 16, 8
    rows, _ = synth.clustered_f32(n, dim, 461, n_clusters=8)
    index, data, st = bf_index(rows)
    init = seeds_of(rows, k, 11)
    o = check_lloyd(index, data, n, st, init, max_iterations=0, what="max_iterations 0")
    assert o[4] == 0 and not o[5] and np.array_equal(bits(o[0]), bits(init))      # the final assignment only
    o = check_lloyd(index, data, n, st, init, max_iterations=6, convergence_threshold=0.0, what="threshold 0")
    assert o[4] == 6 and not o[5]                                                  # rel < 0 never holds
    o = check_lloyd(index, data, n, st, init, max_iterations=6, convergence_threshold=2.0, what="threshold 2")
    assert o[4] == 2 and o[5]                      # iteration 1: |inf - x| / inf is NaN; iteration 2: rel <= 1 < 2
    check_lloyd(index, data, n, st, init, max_iterations=40, what="to convergence")


@pytest.mark.parametrize("dim,tight,thr", [(7, True, SEQ), (33, True, AVX), (33, False, SEQ), (64, False, AVX),
                                           (64, False, SEQ)])
@pytest.mark.parametrize("family", H.BUILD_FAMILIES)
def test_lloyd_families(family, dim, tight, thr):
    n, k = 600, 6
    rows = H.build_rows(family, n, dim, 470 + dim)
    index, data, st = bf_index(rows, dim if tight else None)
    init = H.centers_from_rows(rows, k, 471)
    o = check_lloyd(index, data, n, st, init, thr=thr, max_iterations=5, what=family)
    if family == "overflow":       # four rows overflow every distance: inertia +inf on the sequential chain, and
        assert np.isposinf(o[3]) and not o[5] and o[4] == 5          # |inf - inf| / inf never converges
    if family == "nan":            # a NaN row joins cluster 0 (no distance is < +inf) and poisons its centre
        assert np.isnan(o[0][0]).any() and np.isposinf(o[3])
    if family == "all-equal":
        assert o[3] == 0.0 and o[5] and o[4] == 2 and o[2][0] == n
    if family == "scaled-70":      # subnormal terms in the exactness test of the inertia tree
        assert 0.0 < o[3] < float(np.finfo(np.float32).tiny) * n


def test_lloyd_null_outputs():
    n, dim, k = 700, 10, 5
    rows, _ = synth.clustered_f32(n, dim, 481, n_clusters=5)
    index, data, st = bf_index(rows)
    init = seeds_of(rows, k, 12)
    full = lloyd_raw(index, init, 4, 1e-5, 0, SEQ)
    oc, oa, os_, oi, oit, oconv = orc.kmeans_lloyd(data, n, st, dim, init, max_iterations=4, simd_threshold=SEQ)
    assert np.array_equal(full["assign"], oa) and np.array_equal(full["sizes"], os_) and full["iterations"] == oit
    assert full["converged"] == int(oconv) and full["inertia"] == oi
    outs = ("assign", "sizes", "inertia", "iterations", "converged")
    for null in [(o,) for o in outs] + [outs]:
        r = lloyd_raw(index, init, 4, 1e-5, 0, SEQ, null=null)
        assert np.array_equal(bits(r["centers"]), bits(oc)), null
        for o in outs:
            if o in null:       # untouched
                assert np.array_equal(r[o], dict(assign=np.zeros(n), sizes=np.zeros(k), inertia=-1.0, iterations=99999,
                                                 converged=-1)[o]), (null, o)
            else:
                assert np.array_equal(r[o], full[o]), (null, o)


# ---- scann_hip_kmeans_init_pp ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BM.SEEDING_CASES)
def test_init_pp_matches_the_seeding_reference(name):
    """every seed equals the single admissible row of its band; the model follows the library's own earlier picks.
    Row VALUES are compared, so that duplicated rows stay unambiguous."""
    case = BM.seeding_case(name)
    index = hip.bf_create(case["data"], case["n"], case["dim"], case["stride"], hip.SQUARED_L2)
    got = hip.kmeans_init_pp(index, case["k"], case["seed"], col_offset=case["col"], sub_dim=case["sub"],
                             simd_threshold=case["thr"])
    win = BM.seeding_window(case)
    ref = BM.seeding_reference(win, case["k"], case["seed"], case["thr"], picks=got)
    assert len(ref) == case["k"], "seed %d is no row of the input" % (len(ref) - 1)
    for c, r in enumerate(ref):
        assert r["rows"].size == 1, "seed %d: band %s" % (c, r["rows"])
        assert np.array_equal(bits(got[c]), bits(win[r["rows"][0]])), "seed %d (%s): not row %d" % (
            c, r["kind"], r["rows"][0])
    assert np.array_equal(bits(got), bits(hip.kmeans_init_pp(index, case["k"], case["seed"], col_offset=case["col"],
                                                             sub_dim=case["sub"], simd_threshold=case["thr"])))
    if name == "nan":              # the pinned rule: a NaN total takes the fallback draw (scann_hip.h, DEVIATION)
        first, rest = BM.stream(case["seed"], case["n"], case["k"])
        assert all(r["kind"] == "nan-total" for r in ref[1:])
        assert np.array_equal(bits(got[1:]), bits(win[[fb for _, fb in rest]]))


# ---- scann_hip_encode -----------------------------------------------------------------------------------------------
def check_encode(cb, rows, centers=None, leaf=None, strides=None, what=""):
    S, K, dsub = cb.shape
    dim = S * dsub
    resid = rows if centers is None else rows - centers[leaf]
    want = orc.encode_many(cb, resid)
    for st in strides or (dim, dim + 1, hip.compute_stride(dim)):
        data, _ = strided(rows, st)
        got = hip.encode(cb, data, stride=st, centers=centers, leaf_of_row=leaf)
        assert np.array_equal(got, want), "%s stride %d: codes differ at %s" % (
            what, st, np.argwhere(got != want)[:6].tolist())
    assert np.array_equal(trainer.encode(cb, resid, chunk=1024), want), "%s: trainer.encode" % what
    return want


@pytest.mark.parametrize("S,K,dsub", [(1, 1, 1), (8, 16, 1), (64, 16, 1), (32, 16, 4), (8, 256, 8), (4, 64, 8),
                                      (16, 17, 2), (2, 100, 32), (8, 256, 1)])
def test_encode_shapes(S, K, dsub):
    dim = S * dsub
    rng = np.random.default_rng([500, S, K, dsub])
    cb = rng.uniform(-1, 1, (S, K, dsub)).astype(np.float32)
    rows = rng.uniform(-1, 1, (4000, dim)).astype(np.float32)
    centers = rng.uniform(-0.5, 0.5, (5, dim)).astype(np.float32)
    leaf = rng.integers(0, 5, 4000).astype(np.uint32)
    for n in (1, 4000):
        check_encode(cb, rows[:n], what="n %d" % n)
        check_encode(cb, rows[:n], centers, leaf[:n], what="n %d residual" % n)


@pytest.mark.parametrize("S,K,dsub", [(8, 256, 4), (16, 16, 3)])
@pytest.mark.parametrize("family", H.ENCODE_FAMILIES)
def test_encode_families(family, S, K, dsub):
    cb, rows = H.encode_inputs(family, S, K, dsub, 500, seed=510)
    want = check_encode(cb, rows, what=family)
    if family == "equal":
        assert not want.any()
    if family == "nan-code":
        assert not (want[:, :S - 2] == 0).any() and (want[:, S - 2] == K - 1).all() and not want[:, S - 1].any()
    rng = np.random.default_rng(511)
    centers = (rng.uniform(-0.5, 0.5, (3, S * dsub)) * (2.0 ** -70 if family == "tiny" else 1.0)).astype(np.float32)
    check_encode(cb, rows, centers, rng.integers(0, 3, 500).astype(np.uint32), what=family + " residual")


@pytest.mark.parametrize("S,K,dsub", [(8, 256, 1), (16, 256, 2)])
def test_encode_residual_is_taken_before_the_codeword_difference(S, K, dsub):
    """rows = a centre near +-1000 plus a unit-scale residual: (x - centre) - codeword keeps the residual's bits,
    (x - codeword) - centre would round it to an ulp of 1000 first and move codes between close codewords"""
    n, dim = 4000, S * dsub
    rng = np.random.default_rng([515, S])
    cb = rng.uniform(-1, 1, (S, K, dsub)).astype(np.float32)
    centers = (rng.choice([-1000.0, 1000.0], (6, dim)) + rng.uniform(-50, 50, (6, dim))).astype(np.float32)
    leaf = rng.integers(0, 6, n).astype(np.uint32)
    rows = (centers[leaf] + rng.uniform(-1, 1, (n, dim)).astype(np.float32)).astype(np.float32)
    want = check_encode(cb, rows, centers, leaf, what="offset")
    x, c = rows.reshape(n, S, 1, dsub), centers[leaf].reshape(n, S, 1, dsub)
    wrong = (((x - cb[None]) - c) ** 2).sum(3, dtype=np.float32).argmin(2)
    assert (wrong != want).sum() >= 5, "the two orders agree on this input"


def test_encode_grid_stride_wrap():
    """n S = 4 480 000 > 16384 blocks x 256 threads: the tail of the elements is reached by the grid-stride step"""
    n, S, K, dsub = 70000, 64, 16, 1
    rng = np.random.default_rng(520)
    cb = rng.uniform(-1, 1, (S, K, dsub)).astype(np.float32)
    rows = rng.uniform(-1, 1, (n, S)).astype(np.float32)
    assert n * S > 16384 * 256
    check_encode(cb, rows, strides=(S,), what="wrap")


# ---- scann_hip_lut_from_query ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dsub", [1, 4, 16])
@pytest.mark.parametrize("K", [1, 16, 17, 100, 256])
def test_lut_from_query_shapes_and_queries(K, dsub):
    S = 8 if K <= 16 else 4
    dim, n, L = S * dsub, 96, 4
    rng = np.random.default_rng([530, K, dsub])
    cb = rng.uniform(-1, 1, (S, K, dsub)).astype(np.float32)
    rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    codes = rng.integers(0, K, (n, S)).astype(np.uint8)
    oix, kw = H.txh_from_codes(rows, cb, codes, L, P=2, mult=2.0, seed=531)
    index = hip.txh_create(**kw)
    qs = [H.adversarial_queries(f, 4, dim, 532, rows)
          for f in ("signed", "scaled-70", "scaled+56", "spread", "integers", "zero")]
    q = np.concatenate(qs + [rng.uniform(-1, 1, (3, dim)).astype(np.float32)])
    q[-3, dim // 2] = np.nan                      # one NaN element: its subspace's table row is NaN
    q[-2] = np.nan
    q[-1] *= np.float32(1e20)                     # entries overflow to +inf
    q = np.ascontiguousarray(q, np.float32)
    want = np.stack([orc.lut_from_query(cb, qi) for qi in q])
    assert np.isnan(want[-3]).any() and not np.isnan(want[-3]).all() and np.isposinf(want[-1]).any()
    assert_same_f32(hip.lut_from_query(index, q, S, K), want, "plain")
    leaves = (np.arange(q.shape[0]) % L).astype(np.uint32)
    want = np.stack([orc.lut_from_query(cb, qi - oix.centers[l]) for qi, l in zip(q, leaves)])
    assert_same_f32(hip.lut_from_query(index, q, S, K, leaf_for_query=leaves), want, "residual")


# ---- the whole chain (the steps of tools/time_build.py) -------------------------------------------------------------
def test_build_chain_matches_oracle_step_by_step():
    n, dim, L, S, K, k = 3000, 32, 8, 8, 16, 10
    dsub = dim // S
    rows, _ = synth.clustered_f32(n, dim, 541, n_clusters=L)
    index, data, st = bf_index(rows)
    seeds = hip.kmeans_init_pp(index, L, seed=42)
    win = np.ascontiguousarray(rows)
    ref = BM.seeding_reference(win, L, 42, picks=seeds)
    assert all(r["rows"].size == 1 and np.array_equal(bits(seeds[c]), bits(win[r["rows"][0]]))
               for c, r in enumerate(ref))
    oc, oa, _, _, _, _ = check_lloyd(index, data, n, st, seeds, max_iterations=20, what="partitioner")
    resid = rows - oc[oa]
    rindex, rdata, _ = bf_index(resid)
    cb = np.zeros((S, K, dsub), np.float32)
    for s in range(S):
        c0 = hip.kmeans_init_pp(rindex, K, seed=42 + s, col_offset=s * dsub, sub_dim=dsub)
        assert all((bits(resid[:, s * dsub:(s + 1) * dsub]) == bits(c)[None]).all(1).any() for c in c0)
        cb[s] = check_lloyd(rindex, rdata, n, st, c0, col=s * dsub, max_iterations=8, what="subspace %d" % s)[0]
    codes = hip.encode(cb, data, stride=st, centers=oc, leaf_of_row=oa)
    assert np.array_equal(codes, orc.encode_many(cb, resid))
    order = np.argsort(oa, kind="stable").astype(np.uint32)
    leaf_off = np.zeros(L + 1, np.uint32)
    leaf_off[1:] = np.cumsum(np.bincount(oa, minlength=L))
    kw = dict(data=data, n_rows=n, dim=dim, stride=st, centers=oc, leaf_offsets=leaf_off, leaf_ids=order, codebook=cb,
              codes=codes[order], partitions_to_search=3, pre_reorder_multiplier=4.0)
    tree = hip.txh_create(**kw)
    oix = orc.TxhIndex(data, st, dim, oc, leaf_off, order, cb, codes[order], partitions_to_search=3,
                       pre_reorder_multiplier=4.0)
    q = rows[::n // 16][:16] + np.float32(0.01)
    o = hip.default_opts()
    o.partitions_to_search, o.pre_reorder_k = 3, orc.pre_reorder_k(k, 4.0)
    idx, dist, cnt, (tok, tokd, ci, cd, cc) = tree.search_batched(q, k, o, stages=True)
    for i in range(q.shape[0]):
        H.check_txh_query(oix, q[i], k, idx[i, :cnt[i]], dist[i, :cnt[i]], tok[i], tokd[i], ci[i, :cc[i]],
                          cd[i, :cc[i]], what="q%d" % i)


# ---- the LDS limit --------------------------------------------------------------------------------------------------
def test_assign_nearest_lds_limit():
    """16 centres x ceil(dim / 4) x 16 B of LDS: 160 KB at dim 2560; above it 8 centres per tile, 160 KB at dim 5120;
    above that ResourceExhausted, no launch error"""
    n, k = 64, 3
    rng = np.random.default_rng(550)
    for dim, ok in ((2560, True), (2564, True), (5120, True), (5124, False)):
        rows = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
        centers = rng.uniform(-1, 1, (k, dim)).astype(np.float32)
        index, _, _ = bf_index(rows)
        if ok:
            want_tok, want_dist = nearest_reference(rows, centers)
            check_assign(index, n, centers, want_tok, want_dist, "dim %d" % dim)
        else:
            with pytest.raises(hip.ScannError) as e:
                hip.bf_assign_nearest(index, centers)
            assert e.value.code == hip.RESOURCE_EXHAUSTED, e.value
        index.close()


def test_kmeans_lds_limit():
    """the AVX2-order kernel stages 8 centres: 160 KB at sub_dim 5120; the sequential one 16 up to 2560 and 8 above"""
    n, k = 64, 3
    rng = np.random.default_rng(551)
    rows = rng.uniform(-1, 1, (n, 5128)).astype(np.float32)
    index, data, st = bf_index(rows)
    check_lloyd(index, data, n, st, seeds_of(rows[:, :5120], k, 13), thr=AVX, max_iterations=2, what="avx 5120")
    check_lloyd(index, data, n, st, seeds_of(rows[:, 8:2568], k, 13), col=8, thr=SEQ, max_iterations=2,
                what="seq 2560")
    check_lloyd(index, data, n, st, seeds_of(rows[:, 4:2568], k, 13), col=4, thr=SEQ, max_iterations=2,
                what="seq 2564")
    check_lloyd(index, data, n, st, seeds_of(rows[:, 8:5128], k, 13), col=8, thr=SEQ, max_iterations=2,
                what="seq 5120")
    for sub, thr in ((5128, AVX), (5124, SEQ)):
        with pytest.raises(hip.ScannError) as e:
            hip.kmeans_lloyd(index, seeds_of(rows[:, :sub], k, 13), max_iterations=2, simd_threshold=thr)
        assert e.value.code == hip.RESOURCE_EXHAUSTED, e.value

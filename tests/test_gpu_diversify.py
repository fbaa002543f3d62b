"""Multi-attribute crowded searches and MMR searches (include/scann_hip.h "multi-attribute crowding", "MMR").

Every search-backed case is checked two ways, as in test_gpu_crowding.py whose data, seeds and helpers are reused:
  (A) diversify_model over the GPU's own plain search_batched at k = depth: indices, distance bits, counts bitwise;
  (B) the same model over the oracle's row at k = depth, after asserting that the oracle's depth + 1 distances are
      strictly increasing.  (Where the two rows are bit-equal the model runs once.)
"""
import ctypes
import functools

import numpy as np
import pytest

import diversify_model as DM
import helpers as H
from oracle import pyoracle as orc
from scann_rust_amd import hip, synth
from test_gpu_bf_filters import allow_of
from test_gpu_crowding import (DEPTHS, DIM, HASHED, SEEDS, SENT, U64, Case, bf_case, bits, graded_queries, graded_rows,
                               int8_case, ks_of)

pytestmark = pytest.mark.gpu

N = 3001
MAX_KEYS = 6144
MODULI = (7, 5, 3, 11, 13, 2, 17, 19)
MD_FAMILIES = ("mod", "mixed", "short", "chain", "one-dim-binds")
MMR_DEPTHS = (1, 2, 63, 64, 65, 257, 1000, 2048)
LAMBDAS = (0.0, 0.25, 0.5, 0.7, 1.0)
BIG = 2 ** 32 - 1


def same_row(a, b):
    return a[0].size == b[0].size and np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


def check_against(got, nq, k, rows_a, rows_b, model, what):
    """got = (idx, dist, cnt) of a staged call; rows_a(i) / rows_b(i) -> (idx, dist) of the GPU's plain row and of the
    oracle's row of query i (rows_b None: check A only); model(idx, dist) -> (idx, dist) the stage must return"""
    gi, gd, gc = got
    assert gi.shape == (nq, k) and gd.shape == (nq, k)
    for i in range(nq):
        ra = rows_a(i)
        wants = [("A", model(*ra))]
        if rows_b is not None:
            rb = rows_b(i)
            wants.append(("B", wants[0][1] if same_row(ra, rb) else model(*rb)))
        c = int(gc[i])
        for tag, (wi, wd) in wants:
            assert c == wi.size, (tag, what, i, c, wi.size)
            assert np.array_equal(gi[i, :c], wi), (tag, what, i)
            assert np.array_equal(bits(gd[i, :c]), bits(wd)), (tag, what, i)
        assert np.all(gi[i, c:] == SENT) and np.all(np.isposinf(gd[i, c:])), (what, i)


def plain_rows(p):
    pi, pd, pc = p
    return lambda i: (pi[i, :pc[i]], pd[i, :pc[i]])


# ---- multi-attribute crowding -----------------------------------------------------------------------------------------
def md_attrs(family, n, n_dims, near):
    """([n_dims][n_attrs] uint64, fixed limits or None).  near: query 0's row (datapoint indices, nearest first)."""
    i = np.arange(n, dtype=np.uint64)
    if family == "mod":
        return np.stack([i % np.uint64(MODULI[j]) for j in range(n_dims)]), None
    if family == "mixed":      # dimension 0: equal low words, different high words; dimension 1: 0 and 2^64 - 1
        a = [((i % np.uint64(9)) << np.uint64(32)) | np.uint64(0xDEADBEEF), np.where(i % np.uint64(2) == 0, np.uint64(0), U64)]
        a += [i % np.uint64(MODULI[j]) for j in range(2, n_dims)]
        return np.stack(a[:n_dims]), None
    if family == "short":      # half the index has no entry: attribute 0 in every dimension
        return np.stack([i[:n // 2] % np.uint64(3 + j) for j in range(n_dims)]), None
    pos = np.full(n, -1, np.int64)          # position in query 0's row; rows past it keep distinct attributes
    pos[near] = np.arange(near.size)
    p = np.where(pos >= 0, pos, n + np.arange(n)).astype(np.uint64)
    if family == "chain":      # dimension 0 = p // 2, dimension 1 = (p + 1) // 2, the rest distinct; limits 1
        a = [p // np.uint64(2), (p + np.uint64(1)) // np.uint64(2)] + [p + np.uint64(j) for j in range(2, n_dims)]
        return np.stack(a[:n_dims]), [1] * n_dims
    assert family == "one-dim-binds"      # dimension 1 all equal with limit 3, every other dimension distinct
    a = [i + np.uint64(1000 * j) for j in range(n_dims)]
    if n_dims > 1:
        a[1] = np.full(n, 42, np.uint64)
    return np.stack(a), [BIG, 3][:n_dims] + [1] * max(0, n_dims - 2)


def md_limit_draws(rng, depth, n_dims, fixed):
    pool = [0, 1, 2, depth, BIG]
    draws = [[int(x) for x in rng.choice(pool[1:], n_dims)], [int(x) for x in rng.choice(pool, n_dims)]]
    return ([fixed] if fixed is not None else [[2] * n_dims]) + draws


def md_sweep(case, nq, n_dims, family, depths=DEPTHS):
    index = case.index
    attrs, fixed = md_attrs(family, case.n, n_dims, case.oi[0])
    index.set_crowding_attributes_md(attrs)
    rng = np.random.default_rng([n_dims, nq, MD_FAMILIES.index(family)])
    for depth in depths:
        plain = case.plain(nq, depth)
        for k in ks_of(depth):
            if n_dims * k > MAX_KEYS:
                continue
            for limits in md_limit_draws(rng, depth, n_dims, fixed):
                what = (family, n_dims, depth, k, limits)
                got = index.search_crowded_md(case.q[:nq], k, depth, limits)
                check_against(got, nq, k, plain_rows(plain), lambda i: case.oracle(i, depth),
                              lambda ri, rd: DM.md_apply(ri, rd, attrs, limits, k), what)
                if min(limits) == 0:
                    assert not got[2].any()
                if family == "chain" and limits == fixed:       # exactly the even positions of query 0's row
                    want = case.oi[0][0:min(depth, case.n):2][:k]
                    assert got[2][0] == want.size and np.array_equal(got[0][0, :want.size], want), what
                if family == "one-dim-binds" and limits == fixed and n_dims > 1:
                    assert np.all(got[2] == min(3, k)), what


@pytest.mark.parametrize("family", MD_FAMILIES)
@pytest.mark.parametrize("n_dims", [1, 2, 8])
@pytest.mark.parametrize("nq", [3, 64])
def test_bf_crowded_md(nq, n_dims, family):
    md_sweep(bf_case(N, hip.SQUARED_L2), nq, n_dims, family)


def test_bf_crowded_md_dot_product():
    md_sweep(bf_case(N, hip.DOT_PRODUCT), 64, 2, "chain", depths=(65, 1000))
    md_sweep(bf_case(N, hip.DOT_PRODUCT), 3, 8, "mod", depths=(10, 64))


@pytest.mark.parametrize("nq", [3, 64])
def test_one_dimension_equals_search_crowded(nq):
    """n_dims = 1: bit for bit what the one-attribute stage returns; the two attribute arrays are independent"""
    case = bf_case(N, hip.SQUARED_L2)
    index = case.index
    i = np.arange(N, dtype=np.uint64)
    attrs = i % np.uint64(7)
    index.set_crowding_attributes(attrs)
    index.set_crowding_attributes_md(attrs[None])
    for depth in DEPTHS:
        for k in ks_of(depth):
            for limit in sorted({0, 1, 2, depth, BIG}):
                a = index.search_crowded(case.q[:nq], k, depth, limit)
                b = index.search_crowded_md(case.q[:nq], k, depth, [limit])
                assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2]), \
                    (depth, k, limit)
    # replacing one array leaves the other in place
    want = index.search_crowded(case.q[:nq], 10, 64, 1)
    index.set_crowding_attributes_md(np.stack([i % np.uint64(3), i % np.uint64(2)]))
    got = index.search_crowded(case.q[:nq], 10, 64, 1)
    assert all(np.array_equal(x, y) for x, y in zip(want, got))
    index.set_crowding_attributes(i % np.uint64(2))
    got = index.search_crowded_md(case.q[:nq], 10, 64, [1, BIG])
    assert np.all(got[2] == 3)


@pytest.mark.parametrize("kind", ["ah", "txh"])
def test_hashed_crowded_md(kind):
    """a flat hasher and a Tree-X-Hybrid handle (the small cases of the crowding tests), check (A)"""
    make, opts = HASHED[kind]
    kw, q, _, n = make()
    index = hip.txh_create(**kw)
    depth, k = 100, 10
    i = np.arange(n, dtype=np.uint64)
    attrs = np.stack([i % np.uint64(7), ((i % np.uint64(13)) << np.uint64(32)) | np.uint64(1), i % np.uint64(2)])
    index.set_crowding_attributes_md(attrs)
    for nq in (3, 64):
        plain = index.search_batched(q[:nq], depth, opts=opts())
        for limits in ([1, 1, 1], [3, 2, 4], [BIG, 1, 3]):
            got = index.search_crowded_md(q[:nq], k, depth, limits, opts=opts())
            check_against(got, nq, k, plain_rows(plain), None, lambda ri, rd: DM.md_apply(ri, rd, attrs, limits, k),
                          (kind, nq, limits))


def test_bf_crowded_md_with_allow_bitmap():
    case = bf_case(N, hip.SQUARED_L2)
    index = case.index
    nq, k, depth = 64, 10, 64
    words, cap = allow_of("f50", N, k)
    i = np.arange(N, dtype=np.uint64)
    attrs = np.stack([i % np.uint64(4) + np.uint64(1), i % np.uint64(3)])
    index.set_crowding_attributes_md(attrs)
    plain = index.search_batched(case.q[:nq], depth, allow=words, allow_bits=cap)
    allowed = set(H.allowed_ids(words, cap, N).tolist())
    for limits in ([1, 1], [2, 3], [depth, 1]):
        got = index.search_crowded_md(case.q[:nq], k, depth, limits, allow=words, allow_bits=cap)
        check_against(got, nq, k, plain_rows(plain), None, lambda ri, rd: DM.md_apply(ri, rd, attrs, limits, k), limits)
        assert all(int(x) in allowed for x in got[0][got[0] != SENT])


def test_crowd_md_apply_on_crafted_rows():
    """short counts and empty rows: walked to their count; slots past the count are never looked up"""
    case = bf_case(N, hip.SQUARED_L2)
    index = case.index
    rng = np.random.default_rng(5)
    nq, depth = 9, 70
    i = np.arange(N, dtype=np.uint64)
    attrs = np.stack([i % np.uint64(5), i % np.uint64(3)])
    attrs[:, 0] = np.uint64(0xABCDEF)         # what a looked-up sentinel (clamped or wrapped to 0) would most plausibly hit
    index.set_crowding_attributes_md(attrs)
    ri = np.stack([rng.permutation(np.arange(1, N))[:depth] for _ in range(nq)]).astype(np.uint32)
    rd = np.sort(rng.random((nq, depth)).astype(np.float32), axis=1)
    rc = np.array([0, 1, 9, 63, 64, 65, 69, 70, 0], np.uint32)
    for q in range(nq):
        ri[q, rc[q]:] = SENT
        rd[q, rc[q]:] = np.inf
    for k, limits in ((10, [1, 2]), (70, [2, 2]), (1, [1, 1]), (10, [BIG, BIG]), (10, [0, 5])):
        got = index.crowd_md_apply(ri, rd, rc, k, limits)
        check_against(got, nq, k, lambda q: (ri[q, :rc[q]], rd[q, :rc[q]]), None,
                      lambda a, b: DM.md_apply(a, b, attrs, limits, k), (k, limits))
        assert got[2][0] == 0 and got[2][8] == 0


def _ptr(t):
    return t.data_ptr()


def _two_streams(index, q, nq, k, depth, host, device, reserve, params, opts=None):
    """after `reserve`, on two streams: the device entry's rows equal the host entry's for every parameter value, with
    no allocation once each stream has bound its workspace"""
    import torch
    dev = torch.device("cuda:0")
    L = hip.load()
    want = {p: host(p) for p in params}
    qd = torch.from_numpy(np.ascontiguousarray(q[:nq])).to(dev)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    outs = [(torch.zeros((nq, k), dtype=torch.int32, device=dev), torch.zeros((nq, k), dtype=torch.float32, device=dev),
             torch.zeros(nq, dtype=torch.int32, device=dev)) for _ in streams]
    reserve()
    for s, o in zip(streams, outs):
        device(params[0], qd, o, s.cuda_stream)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(dev)[0]
    for p in list(params) + [params[0]]:
        for s, o in zip(streams, outs):
            device(p, qd, o, s.cuda_stream)
        for s, o in zip(streams, outs):
            assert L.scann_hip_index_last_device_status(index.h, ctypes.c_void_p(s.cuda_stream)) == hip.OK
            s.synchronize()
            gi, gd, gc = (t.cpu().numpy() for t in o)
            assert np.array_equal(gi.view(np.uint32), want[p][0]), p
            assert np.array_equal(bits(gd), bits(want[p][1])), p
            assert np.array_equal(gc.view(np.uint32), want[p][2]), p
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(dev)[0] == free0


def test_crowded_md_device_entry_two_streams():
    case = bf_case(N, hip.SQUARED_L2)
    index, nq, k, depth = case.index, 64, 10, 512
    i = np.arange(N, dtype=np.uint64)
    index.set_crowding_attributes_md(np.stack([i % np.uint64(7), i % np.uint64(4)]))
    L = hip.load()
    _two_streams(index, case.q, nq, k, depth,
                 host=lambda lim: index.search_crowded_md(case.q[:nq], k, depth, list(lim)),
                 device=lambda lim, qd, o, st: index.search_crowded_md_device(_ptr(qd), nq, DIM, k, depth, list(lim),
                                                                             _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), st),
                 reserve=lambda: hip.check(L.scann_hip_index_reserve_crowded(index.h, nq, k, depth, None)),
                 params=[(1, 1), (3, 2), (BIG, 1)])


# ---- MMR ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mmr_case(measure, dim=DIM):
    """(case, data, stride): the graded brute-force case of the crowding tests; Cosine and dim = 35 are built here"""
    if dim == DIM and (N, measure) in SEEDS:
        seed = SEEDS[(N, measure)]
        data, stride = orc.to_strided(graded_rows(N, DIM, seed))
        return bf_case(N, measure), data, stride
    if dim == DIM:
        rows, q = graded_rows(N, dim, 1), graded_queries(64, dim, 1)
    else:
        rows, q = synth.uniform_f32(N, dim, 5), synth.uniform_f32(64, dim, 6)
    data, stride = orc.to_strided(rows)
    oi, od, _ = orc.bf_search_batched(data, N, dim, stride, measure, q[:3], 258)
    return Case(lambda: hip.bf_create(data, N, dim, stride, measure), q, oi, od, N), data, stride


def mmr_sweep(measure, nq, lam, depths, ks, dim=DIM):
    case, data, stride = mmr_case(measure, dim)
    index = case.index
    for depth in depths:
        plain = case.plain(nq, depth)
        for k in ks(depth):
            got = index.search_mmr(case.q[:nq], k, depth, lam)
            check_against(got, nq, k, plain_rows(plain), lambda i: case.oracle(i, depth),
                          lambda ri, rd: DM.mmr_apply_rows(ri, rd, k, lam, data, stride, dim, measure)[:2],
                          (measure, nq, lam, depth, k))
            assert np.array_equal(got[0][:, 0], plain[0][:, 0])          # entry 0 of the row is selected first
            if lam == 1.0 and measure == hip.SQUARED_L2:                 # finite similarities: the first k of the row
                assert np.array_equal(got[0], plain[0][:, :k])


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("measure", [hip.SQUARED_L2, hip.DOT_PRODUCT])
def test_bf_mmr_few_queries(measure, lam):
    mmr_sweep(measure, 3, lam, MMR_DEPTHS, ks_of)


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("measure", [hip.SQUARED_L2, hip.DOT_PRODUCT])
def test_bf_mmr_batch(measure, lam):
    mmr_sweep(measure, 64, lam, MMR_DEPTHS, lambda depth: sorted({1, min(10, depth), min(64, depth)}))


@pytest.mark.parametrize("measure", [hip.L1, hip.COSINE])
def test_bf_mmr_l1_cosine(measure):
    for lam in (0.25, 0.7):
        mmr_sweep(measure, 3, lam, (2, 64, 65), ks_of)


def test_bf_mmr_scalar_tail_dim_35():
    for measure in (hip.SQUARED_L2, hip.DOT_PRODUCT):
        mmr_sweep(measure, 3, 0.5, (40, 257), lambda depth: (10, depth), dim=35)


def test_mmr_clamps_lambda_and_depth_zero_means_k():
    case, _, _ = mmr_case(hip.SQUARED_L2)
    index, q = case.index, case.q[:3]
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))
    assert same(index.search_mmr(q, 10, 64, -3.0), index.search_mmr(q, 10, 64, 0.0))
    assert same(index.search_mmr(q, 10, 64, 9.0), index.search_mmr(q, 10, 64, 1.0))
    assert same(index.search_mmr(q, 10, 0, 0.5), index.search_mmr(q, 10, 10, 0.5))
    gi, gd, gc = index.search_mmr(q, 0, 0, 0.5)
    assert gi.shape == (3, 0) and not gc.any()


def test_mmr_duplicates_lowest_position_wins():
    """every dataset row stored three times: scores tie exactly and the lowest position must win -- (A) only"""
    base = synth.uniform_f32(1000, DIM, 9)
    rows = np.concatenate([base, base, base])
    data, stride = orc.to_strided(rows)
    q = synth.uniform_f32(64, DIM, 10)
    for measure in (hip.SQUARED_L2, hip.DOT_PRODUCT):
        index = hip.bf_create(data, 3000, DIM, stride, measure)
        for nq, depth, k in ((3, 66, 66), (64, 257, 30)):
            plain = index.search_batched(q[:nq], depth)
            assert np.any(np.diff(plain[1], axis=1) == 0)
            for lam in (0.0, 0.5, 1.0):
                got = index.search_mmr(q[:nq], k, depth, lam)
                check_against(got, nq, k, plain_rows(plain), None,
                              lambda ri, rd: DM.mmr_apply_rows(ri, rd, k, lam, data, stride, DIM, measure)[:2],
                              (measure, nq, depth, k, lam))


def test_mmr_overflowing_similarities_take_the_fallback():
    """DotProduct, queries at scale 2^-50, a third of the rows at scale 2^63: query-to-row distances stay finite,
    row-to-row dots are +-inf.  At lambda = 1 the -inf similarity leaves max_sim at f32::MIN, the +inf one makes the
    score NaN (0 * inf), and a round whose scores are all NaN takes the lowest remaining position -- (A) only"""
    rng = np.random.default_rng(11)
    n = 3000
    rows = rng.uniform(-1, 1, (n, DIM)).astype(np.float32)
    rows[::3] *= np.float32(2.0 ** 63)
    q = (rng.uniform(-1, 1, (64, DIM)) * 2.0 ** -50).astype(np.float32)
    data, stride = orc.to_strided(rows)
    index = hip.bf_create(data, n, DIM, stride, hip.DOT_PRODUCT)
    for nq, depth, k in ((64, 10, 10), (3, 65, 20)):
        plain = index.search_batched(q[:nq], depth)
        assert np.all(np.isfinite(plain[1]))
        for lam in (1.0, 0.5):
            falls = [DM.mmr_apply_rows(plain[0][i, :plain[2][i]], plain[1][i, :plain[2][i]], k, lam, data, stride, DIM,
                                       hip.DOT_PRODUCT)[2] for i in range(nq)]
            if lam == 1.0 and depth == 10:      # (every entry of these short rows is one of the large rows)
                assert max(falls) > 0, "no query takes the f32::MIN fall-back: the case would pass vacuously"
            got = index.search_mmr(q[:nq], k, depth, lam)
            check_against(got, nq, k, plain_rows(plain), None,
                          lambda ri, rd: DM.mmr_apply_rows(ri, rd, k, lam, data, stride, DIM, hip.DOT_PRODUCT)[:2],
                          (nq, depth, k, lam))


def test_mmr_apply_on_short_rows():
    case, data, stride = mmr_case(hip.SQUARED_L2)
    index = case.index
    rng = np.random.default_rng(12)
    k, depth = 12, 40
    rc = np.array([0, 1, k - 1, k, depth, 0], np.uint32)
    nq = rc.size
    ri = np.stack([rng.permutation(N)[:depth] for _ in range(nq)]).astype(np.uint32)
    rd = np.sort(rng.random((nq, depth)).astype(np.float32), axis=1)
    for i in range(nq):
        ri[i, rc[i]:] = SENT
        rd[i, rc[i]:] = np.inf
    for lam in (0.0, 0.5):
        got = index.mmr_apply(ri, rd, rc, k, lam)
        check_against(got, nq, k, lambda i: (ri[i, :rc[i]], rd[i, :rc[i]]), None,
                      lambda a, b: DM.mmr_apply_rows(a, b, k, lam, data, stride, DIM, hip.SQUARED_L2)[:2], lam)
        assert got[2].tolist() == [0, 1, k - 1, k, k, 0]


@pytest.mark.parametrize("kind", ["txh", "partitioned"])
def test_hashed_mmr(kind):
    """a Tree-X-Hybrid and a Partitioned handle with `data` in datapoint order -- (A) over the handle's own plain row"""
    make, opts = HASHED[kind]
    kw, q, _, n = make()
    index = hip.txh_create(**kw)
    data, stride, dim = kw["data"], kw["stride"], kw["dim"]
    measure = kw.get("distance_measure", hip.SQUARED_L2)
    depth, k = 100, 10
    for nq in (3, 64):
        plain = index.search_batched(q[:nq], depth, opts=opts())
        for lam in (0.25, 0.7):
            got = index.search_mmr(q[:nq], k, depth, lam, opts=opts())
            check_against(got, nq, k, plain_rows(plain), None,
                          lambda ri, rd: DM.mmr_apply_rows(ri, rd, k, lam, data, stride, dim, measure)[:2], (kind, nq, lam))


def test_mmr_device_entry_two_streams():
    case, _, _ = mmr_case(hip.SQUARED_L2)
    index, nq, k, depth = case.index, 64, 10, 257
    _two_streams(index, case.q, nq, k, depth,
                 host=lambda lam: index.search_mmr(case.q[:nq], k, depth, lam),
                 device=lambda lam, qd, o, st: index.search_mmr_device(_ptr(qd), nq, DIM, k, depth, lam, _ptr(o[0]),
                                                                      _ptr(o[1]), _ptr(o[2]), st),
                 reserve=lambda: index.reserve_mmr(nq, k, depth), params=[0.25, 0.7, 1.0])


def test_host_cpp_diversify_through_handles():
    """scann.hpp: search_with_crowding_md and search_with_mmr on the reference's vectors"""
    import os
    import subprocess
    from scann_rust_amd import build
    exe = os.path.join(os.path.dirname(os.path.abspath(build.__file__)), "host", "diversify_test")
    if not os.path.exists(exe):
        build.build_host()
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "diversify_test ok" in r.stdout


# ---- errors -----------------------------------------------------------------------------------------------------------
def _code(fn):
    try:
        fn()
    except hip.ScannError as e:
        return e.code
    return hip.OK


def test_errors():
    case = bf_case(N, hip.SQUARED_L2)
    q = case.q[:3]
    data, stride = orc.to_strided(graded_rows(300, DIM, 1))
    index = hip.bf_create(data, 300, DIM, stride, hip.SQUARED_L2)
    i = np.arange(300, dtype=np.uint64)
    # multi-attribute crowding
    assert _code(lambda: index.search_crowded_md(q, 5, 10, [1, 1])) == hip.FAILED_PRECONDITION
    index.set_crowding_attributes(i % np.uint64(3))          # the one-attribute array does not count
    assert _code(lambda: index.search_crowded_md(q, 5, 10, [1])) == hip.FAILED_PRECONDITION
    assert _code(lambda: index.set_crowding_attributes_md(np.zeros((9, 300), np.uint64))) == hip.INVALID_ARGUMENT
    assert _code(lambda: index.set_crowding_attributes_md(np.zeros((0, 300), np.uint64), n_dims=0)) == hip.INVALID_ARGUMENT
    index.set_crowding_attributes_md(np.stack([i % np.uint64(3), i % np.uint64(2)]))
    assert _code(lambda: index.search_crowded_md(q, 5, 10, [1, 1])) == hip.OK
    assert _code(lambda: index.search_crowded_md(q, 5, 10, [1])) == hip.INVALID_ARGUMENT
    assert _code(lambda: index.search_crowded_md(q, 5, 10, [1, 1, 1])) == hip.INVALID_ARGUMENT
    assert _code(lambda: index.search_crowded_md(q, 11, 10, [1, 1])) == hip.INVALID_ARGUMENT
    assert _code(lambda: index.search_crowded_md(q, 5, 2049, [BIG, BIG])) == hip.OK      # host path: walked to the count
    big = case.index
    big.set_crowding_attributes_md(np.zeros((8, N), np.uint64))
    assert _code(lambda: big.search_crowded_md(q, 5, 2049, [1] * 8)) == _code(lambda: big.search_batched(q, 2049)) \
        == hip.UNIMPLEMENTED
    assert _code(lambda: big.search_crowded_md(q, 769, 1000, [1] * 8)) == hip.UNIMPLEMENTED     # 8 * 769 > 6144
    assert _code(lambda: big.search_crowded_md(q, 768, 1000, [1] * 8)) == hip.OK
    ri, rd, rc = np.zeros((2, 10), np.uint32), np.zeros((2, 10), np.float32), np.array([10, 11], np.uint32)
    assert _code(lambda: index.crowd_md_apply(ri, rd, rc, 5, [1, 1])) == hip.INVALID_ARGUMENT   # rows_count > depth
    index.set_crowding_attributes_md(None)
    assert _code(lambda: index.search_crowded_md(q, 5, 10, [1, 1])) == hip.FAILED_PRECONDITION
    # MMR
    assert _code(lambda: index.search_mmr(q, 5, 10, 0.5)) == hip.OK
    assert _code(lambda: index.search_mmr(q, 11, 10, 0.5)) == hip.INVALID_ARGUMENT
    assert _code(lambda: index.search_mmr(q, 5, 10, float("nan"))) == hip.INVALID_ARGUMENT
    assert _code(lambda: index.search_mmr(q, 5, 2049, 0.5)) == hip.UNIMPLEMENTED
    assert _code(lambda: index.reserve_mmr(4, 5, 2049)) == hip.UNIMPLEMENTED
    assert _code(lambda: index.reserve_mmr(4, 5, 4)) == hip.INVALID_ARGUMENT
    rc = np.array([10, 3], np.uint32)
    assert _code(lambda: index.mmr_apply(ri, rd, rc, 5, 0.5)) == hip.OK
    bad = ri.copy()
    bad[1, 2] = 300                                              # an index that is no datapoint, below the count
    assert _code(lambda: index.mmr_apply(bad, rd, rc, 5, 0.5)) == hip.INVALID_ARGUMENT
    bad[1, 2], bad[1, 3] = 0, SENT                               # at the count: never looked up
    assert _code(lambda: index.mmr_apply(bad, rd, rc, 5, 0.5)) == hip.OK
    assert _code(lambda: index.mmr_apply(ri, rd, np.array([10, 11], np.uint32), 5, 0.5)) == hip.INVALID_ARGUMENT
    assert _code(lambda: index.mmr_apply(ri, rd, rc, 5, float("nan"))) == hip.INVALID_ARGUMENT
    assert _code(lambda: int8_case().index.search_mmr(int8_case().q, 5, 10, 0.5)) == hip.UNIMPLEMENTED
    # a hashed handle without data; rows held in CSR order
    kw, hq, _, n = HASHED["ah"][0]()
    nodata = dict(kw, data=None)
    ah = hip.txh_create(**nodata)
    o = hip.default_opts()
    o.exact_reorder = 0
    assert _code(lambda: ah.search_mmr(hq[:3], 5, 10, 0.5, opts=o)) == hip.FAILED_PRECONDITION


def test_device_errors():
    import torch
    dev = torch.device("cuda:0")
    data, stride = orc.to_strided(graded_rows(300, DIM, 1))
    index = hip.bf_create(data, 300, DIM, stride, hip.SQUARED_L2)
    qd = torch.zeros((4, DIM), dtype=torch.float32, device=dev)
    o = (torch.zeros((4, 8), dtype=torch.int32, device=dev), torch.zeros((4, 8), dtype=torch.float32, device=dev),
         torch.zeros(4, dtype=torch.int32, device=dev))
    st = torch.cuda.current_stream(dev).cuda_stream
    md = lambda k, depth, lim: _code(lambda: index.search_crowded_md_device(_ptr(qd), 4, DIM, k, depth, lim, _ptr(o[0]),
                                                                            _ptr(o[1]), _ptr(o[2]), st))
    mmr = lambda k, depth, lam: _code(lambda: index.search_mmr_device(_ptr(qd), 4, DIM, k, depth, lam, _ptr(o[0]),
                                                                      _ptr(o[1]), _ptr(o[2]), st))
    assert md(8, 16, [1, 1]) == hip.FAILED_PRECONDITION
    i = np.arange(300, dtype=np.uint64)
    index.set_crowding_attributes_md(np.stack([i % np.uint64(3), i % np.uint64(2)]))
    assert md(8, 4, [1, 1]) == hip.INVALID_ARGUMENT
    assert md(8, 16, [1]) == hip.INVALID_ARGUMENT
    assert md(8, 9000, [1, 1]) == hip.UNIMPLEMENTED
    assert md(8, 16, [1, 1]) == hip.OK
    assert mmr(8, 4, 0.5) == hip.INVALID_ARGUMENT
    assert mmr(8, 16, float("nan")) == hip.INVALID_ARGUMENT
    assert mmr(8, 2049, 0.5) == hip.UNIMPLEMENTED
    assert mmr(8, 16, 0.5) == hip.OK
    torch.cuda.synchronize()

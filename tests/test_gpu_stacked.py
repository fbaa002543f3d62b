"""Stacked / additive quantizer handles (hip.StackedIndex, csrc/stacked.hip) against a float32 restatement of the three
rules of include/scann_hip.h: encode, decode, distance.  Everything is compared bit for bit."""
import numpy as np
import pytest

from scann_rust_amd import hip

pytestmark = pytest.mark.gpu
F = np.float32


def seqsum(p):
    """sum over the last axis, sequential from 0.0f in ascending order"""
    acc = np.zeros(p.shape[:-1], F)
    for j in range(p.shape[-1]):
        acc = acc + p[..., j]
    return acc


def picked(cb, c):
    """the centroids of codes c [n, S] as rows [n, dim]"""
    return cb[np.arange(cb.shape[0])[None, :], c].reshape(c.shape[0], cb.shape[0] * cb.shape[2])


def m_encode(cbs, X):
    R, codes = X.astype(F), []
    with np.errstate(all="ignore"):
        for cb in cbs:
            diff = R.reshape(R.shape[0], cb.shape[0], 1, cb.shape[2]) - cb[None]
            d = seqsum(diff * diff)
            d[np.isnan(d)] = np.inf          # strict < from +inf never takes a NaN; nothing below +inf -> code 0
            codes.append(d.argmin(2))
            R = R - picked(cb, codes[-1])
        return np.concatenate(codes, 1).astype(np.uint8), seqsum(R * R)


def m_decode(cbs, codes):
    x, t = np.zeros((codes.shape[0], cbs[0].shape[0] * cbs[0].shape[2]), F), 0
    for cb in cbs:
        x, t = x + picked(cb, codes[:, t:t + cb.shape[0]]), t + cb.shape[0]
    return x


def m_distances(cbs, codes, Q, measure):
    acc, t = np.zeros((Q.shape[0], codes.shape[0]), F), 0
    for cb in cbs:
        lut = seqsum(Q.reshape(Q.shape[0], cb.shape[0], 1, cb.shape[2]) * cb[None])      # [nq, S, K]
        for s in range(cb.shape[0]):
            acc, t = acc + lut[:, s, codes[:, t]], t + 1
    if measure == hip.DOT_PRODUCT:
        return -acc
    xh = m_decode(cbs, codes)
    return (seqsum(Q * Q)[:, None] + seqsum(xh * xh)[None, :]) - F(2.0) * acc


def m_search(D, k, allowed):
    o, u = D.view(np.uint32).astype(np.uint64), np.uint64
    key = (np.where(o >> u(31), o ^ u(0xFFFFFFFF), o | u(0x80000000)) << u(32)) | np.arange(D.shape[1], dtype=u)
    idx, dist = np.full((D.shape[0], k), 0xFFFFFFFF, np.uint32), np.full((D.shape[0], k), np.nan, F)
    rows = np.flatnonzero(allowed)
    for q in range(D.shape[0]):
        best = rows[np.argsort(key[q, rows])][:k]
        idx[q, :best.size], dist[q, :best.size] = best, D[q, best]
    return idx, dist, np.full(D.shape[0], min(k, rows.size), np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def books(dim, S, K, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((s, k, dim // s)).astype(F) for s, k in zip(S, K)]


def wide(rng, n, dim, pad=3):
    """rows of stride dim + pad whose tail columns must not be read as data"""
    a = rng.standard_normal((n, dim + pad)).astype(F)
    a[:, dim:] = 1e30
    return a


SHAPES = [(16, (4, 4), (16, 16)),              # the reference's own shape
          (96, (8, 4, 12), (256, 16, 5)),
          (64, (1, 1, 1), (256, 256, 7)),      # additive: a subspace's centroids pass the stage in runs of codes
          (256, (1, 2), (256, 256))]           # additive, several runs per subspace at both levels


@pytest.mark.parametrize("n", [1, 63, 65, "tile+1"])
@pytest.mark.parametrize("dim,S,K", SHAPES)
def test_encode_and_decode_match_the_model(dim, S, K, n):
    cbs = books(dim, S, K)
    sq = hip.StackedIndex(cbs)
    n = sq.info()["tile_rows"] + 1 if n == "tile+1" else n
    X = wide(np.random.default_rng(n), n, dim)
    codes, res = sq.encode(X, residual_sq=True)
    want, want_res = m_encode(cbs, X[:, :dim])
    assert np.array_equal(codes, want)
    assert same_bits(res, want_res)
    assert same_bits(sq.decode(codes), m_decode(cbs, want))


def test_encode_ties_zero_residuals_and_nan():
    dim, S, K = 96, (8, 4, 12), (256, 16, 5)
    cbs = books(dim, S, K, seed=1)
    cbs[0][:, 200] = cbs[0][:, 7]            # duplicated centroids: the lower code wins
    cbs[1][:, 9] = cbs[1][:, 2]
    rng = np.random.default_rng(2)
    X = rng.standard_normal((70, dim)).astype(F)
    X[:20] = picked(cbs[0], np.where(rng.random((20, 8)) < 0.5, 200, rng.integers(0, 256, (20, 8))))   # zero level-0 residual
    X[30, 5] = np.nan
    sq = hip.StackedIndex(cbs)
    codes, res = sq.encode(X, residual_sq=True)
    want, want_res = m_encode(cbs, X)
    assert np.array_equal(codes, want) and same_bits(res, want_res)
    assert not (codes[:, :8] == 200).any() and (codes[:20, :8] == 7).any()
    assert codes[30, 0] == 0 and codes[30, 8] == 0 and codes[30, 12] == 0 and np.isnan(res[30])


def quantizer(dim, S, K, n, measure, seed=3):
    rng = np.random.default_rng(seed)
    cbs = books(dim, S, K, seed)
    codes = np.stack([rng.integers(0, k, n) for s, k in zip(S, K) for _ in range(s)], 1).astype(np.uint8).reshape(n, sum(S))
    sq = hip.StackedIndex(cbs, measure=measure)
    sq.set_codes(codes)
    return rng, cbs, codes, sq


@pytest.mark.parametrize("measure", [hip.DOT_PRODUCT, hip.SQUARED_L2])
@pytest.mark.parametrize("nq", [1, 4, 5, 9])
@pytest.mark.parametrize("n", [1, 64, 65, "chunk+1"])
def test_distances_match_the_model(n, nq, measure):
    """dim 12, S = (4, 3): T = 7, so the last code dword carries one pad position"""
    dim, S, K = 12, (4, 3), (16, 16)
    cbs = books(dim, S, K, seed=4)
    sq = hip.StackedIndex(cbs, measure=measure)
    if n == "chunk+1":
        sq.set_codes(np.zeros((1, 7), np.uint8))
        sq.distances(np.zeros((1, dim), F))
        n = sq.info()["chunk_rows"] + 1
    rng = np.random.default_rng(n + nq)
    X, Q = wide(rng, n, dim), wide(rng, nq, dim, pad=1)
    sq.set_rows(X)
    codes = m_encode(cbs, X[:, :dim])[0]
    want = m_distances(cbs, codes, Q[:, :dim], measure)
    assert same_bits(sq.distances(Q), want)
    sq.set_codes(codes)
    assert same_bits(sq.distances(Q), want)


@pytest.mark.parametrize("measure", [hip.DOT_PRODUCT, hip.SQUARED_L2])
def test_distances_walk_table_slabs(measure):
    """4 levels x 16 subspaces x 256 codes: 256 KB of tables per query quad, far more than the two 32 KB buffers"""
    rng, cbs, codes, sq = quantizer(64, (16,) * 4, (256,) * 4, 300, measure)
    Q = rng.standard_normal((5, 64)).astype(F)
    assert same_bits(sq.distances(Q), m_distances(cbs, codes, Q, measure))
    assert sq.info()["slabs"] > 1


@pytest.mark.parametrize("measure", [hip.DOT_PRODUCT, hip.SQUARED_L2])
def test_distances_are_close_to_float64(measure):
    """Against float64 ||q - x^||^2 / -<q, x^> on the f32-decoded rows x^.  With C_j = sum_l |c_l[j]| (>= |x^_j| up to
    rounding): acc = sum_t lut_t passes every product q_j * c_l[j] through one rounding of the product, at most dsub_l - 1
    additions inside its table entry and T - 1 additions across entries, so |acc - sum_j q_j sum_l c_l[j]| <=
    gamma_(dim+T) sum_j |q_j| C_j; the exact sum_l c_l[j] differs from x^_j by at most gamma_(L-1) C_j; qq and xx carry
    gamma_dim of sum q_j^2 and sum x^_j^2; qq + xx, and the final subtraction (2.0f * acc is exact) add one rounding each
    of quantities bounded by sum_j (|q_j| + C_j)^2.  Collected: |d - d64| <= gamma_m sum_j (|q_j| + C_j)^2 with
    m = dim + T + L + 4, gamma_m = m 2^-24 / (1 - m 2^-24)."""
    dim, S, K = 96, (8, 4, 12), (256, 16, 5)
    rng, cbs, codes, sq = quantizer(dim, S, K, 500, measure)
    Q = rng.standard_normal((9, dim)).astype(F)
    xh = m_decode(cbs, codes).astype(np.float64)
    q64 = Q.astype(np.float64)
    d64 = -(q64 @ xh.T) if measure == hip.DOT_PRODUCT else ((q64[:, None, :] - xh[None]) ** 2).sum(2)
    C, t = np.zeros((500, dim)), 0
    for cb in cbs:
        C, t = C + np.abs(picked(cb, codes[:, t:t + cb.shape[0]])), t + cb.shape[0]
    m = dim + sum(S) + len(S) + 4
    gamma = m * 2.0 ** -24 / (1 - m * 2.0 ** -24)
    bound = gamma * ((np.abs(q64)[:, None, :] + C[None]) ** 2).sum(2)
    assert (np.abs(sq.distances(Q).astype(np.float64) - d64) <= bound).all()


SEARCHES = {                                   # n, nq, k, allowed rows (None: no bitmap), every row the same codes
    "k1": (300, 3, 1, None, False), "k10_two_chunks": (9000, 9, 10, None, False), "k256": (700, 5, 256, None, False),
    "k_above_n": (5, 2, 10, None, False), "ties": (2500, 4, 10, None, True), "bitmap_short": (300, 9, 10, 130, False),
    "bitmap_zero": (300, 2, 10, 0, False), "empty": (0, 3, 4, None, False),
}


@pytest.mark.parametrize("measure", [hip.DOT_PRODUCT, hip.SQUARED_L2])
@pytest.mark.parametrize("case", sorted(SEARCHES))
def test_search_matches_sorted_model_distances(case, measure):
    n, nq, k, bits, ties = SEARCHES[case]
    rng, cbs, codes, sq = quantizer(24, (6, 3, 1), (256, 9, 2), n, measure, seed=5)
    if ties:
        codes[:] = codes[0]
        sq.set_codes(codes)
    Q = rng.standard_normal((nq, 24)).astype(F)
    allowed = np.ones(n, bool)
    words = None
    if bits is not None:                       # random bits, of which only the first `bits` count
        words = rng.integers(0, 2 ** 63, (n + 63) // 64, dtype=np.uint64) if bits else np.zeros((n + 63) // 64, np.uint64)
        allowed = ((words[np.arange(n) >> 6] >> (np.arange(n, dtype=np.uint64) & np.uint64(63))) & np.uint64(1)).astype(bool)
        allowed[bits:] = False
    idx, dist, cnt = sq.search_batched(Q, k, allow=words, allow_bits=bits)
    want = m_search(m_distances(cbs, codes, Q, measure), k, allowed)
    assert np.array_equal(idx, want[0]) and same_bits(dist, want[1]) and np.array_equal(cnt, want[2])
    if ties:
        assert (idx == np.arange(k)).all()


def _create(dim, S, K, measure=hip.DOT_PRODUCT):
    """the status of a scann_hip_stacked_create over zero codebooks of that shape"""
    S, K = np.array(S, np.uint32), np.array(K, np.uint32)
    return lambda sq: hip.load().scann_hip_stacked_create(hip.context(), dim, S.size, hip.ptr(S, hip.u32p), hip.ptr(K, hip.u32p),
                                                          hip.ptr(np.zeros(max(1, int(K.sum())) * dim, F), hip.f32p), measure,
                                                          hip.C.byref(hip.vp()))


REFUSALS = {
    "dim_not_multiple": (_create(16, (3,), (16,)), hip.INVALID_ARGUMENT),
    "one_code": (_create(16, (4,), (1,)), hip.INVALID_ARGUMENT),
    "k257_codes": (_create(16, (4,), (257,)), hip.INVALID_ARGUMENT),
    "nine_levels": (_create(16, (4,) * 9, (4,) * 9), hip.INVALID_ARGUMENT),
    "no_levels": (_create(16, (), ()), hip.INVALID_ARGUMENT),
    "t257": (_create(257, (257,), (2,)), hip.INVALID_ARGUMENT),
    "dim4096": (_create(4096, (1,), (2,)), hip.UNIMPLEMENTED),
    "cosine": (_create(16, (4,), (16,), hip.COSINE), hip.UNIMPLEMENTED),
    "code_out_of_range": (lambda sq: sq.set_codes(np.full((3, 8), 16, np.uint8)), hip.INVALID_ARGUMENT),
    "stride_below_dim": (lambda sq: hip.load().scann_hip_stacked_set_rows(sq.h, hip.ptr(np.zeros(64, F), hip.f32p), 2, 15), hip.INVALID_ARGUMENT),
    "n_2_32": (lambda sq: hip.load().scann_hip_stacked_set_codes(sq.h, hip.ptr(np.zeros(8, np.uint8), hip.u8p), 2 ** 32 - 1), hip.OUT_OF_RANGE),
    "k0": (lambda sq: sq.search_batched(np.zeros((1, 16), F), 0), hip.INVALID_ARGUMENT),
    "k257": (lambda sq: sq.search_batched(np.zeros((1, 16), F), 257), hip.INVALID_ARGUMENT),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_leave_the_handle_usable(case):
    cbs = books(16, (4, 4), (16, 16))
    sq = hip.StackedIndex(cbs, measure=hip.SQUARED_L2)
    Q = np.random.default_rng(6).standard_normal((2, 16)).astype(F)
    with pytest.raises(hip.ScannError) as e:   # a search before any rows
        sq.distances(Q)
    assert e.value.code == hip.FAILED_PRECONDITION
    codes = np.random.default_rng(7).integers(0, 16, (70, 8)).astype(np.uint8)
    sq.set_codes(codes)
    call, status = REFUSALS[case]
    try:
        got = call(sq)
    except hip.ScannError as err:
        got = err.code
    assert got == status
    assert case != "dim4096" or b"4095" in hip.load().scann_hip_last_error()   # the message names the limit
    assert sq.size() == 70 and same_bits(sq.distances(Q), m_distances(cbs, codes, Q, hip.SQUARED_L2))

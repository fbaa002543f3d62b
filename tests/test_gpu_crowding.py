"""Crowded searches (scann_hip_search_crowded / _device, include/scann_hip.h "crowding") on every handle kind.

Every case compares the crowded call with two references:
  (A) crowding_model over the GPU's own plain search_batched at k = depth: indices, distance bits, counts bitwise;
  (B) the same model over the oracle's row at k = depth.  (B) is only sound when the oracle's row has no equal
      neighbouring distances (a tie swap legitimately changes who is kept), so each case asserts that the oracle's
      depth + 1 distances are strictly increasing; the data and seeds below were chosen so that this holds for EVERY
      case (rows graded over 100 octaves of norm: neighbouring distances are never one ulp apart).  The tie family
      uses (A) only.
"""
import ctypes
import functools

import numpy as np
import pytest

import crowding_model as CM
import helpers as H
import quantized_checker as qc
from oracle import pyoracle as orc
from scann_rust_amd import hip, synth, trainer
from test_gpu_bf_filters import allow_of

pytestmark = pytest.mark.gpu

SENT = 0xFFFFFFFF
U64 = np.uint64(0xFFFFFFFFFFFFFFFF)
DIM = 32
DEPTHS = (1, 10, 63, 64, 65, 1000, 2048)
OCTAVES = 50
# seeds for which the oracle's 2049 nearest distances of all 64 queries are strictly increasing (checked on the CPU)
SEEDS = {(3001, hip.SQUARED_L2): 1, (3001, hip.DOT_PRODUCT): 1, (20013, hip.SQUARED_L2): 2, (20013, hip.DOT_PRODUCT): 3,
         (3001, hip.L1): 1, "int8": 1}
FAMILIES = ("same", "distinct", "mod7", "low32", "slots", "extremes", "short", "near-block")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def graded_rows(n, dim, seed):
    """U[-1, 1) rows, row i scaled by 2^U(-50, 50): the k nearest distances of a query spread over octaves"""
    rng = np.random.default_rng([seed, 1])
    x = rng.uniform(-1, 1, (n, dim)).astype(np.float32)
    return (x * np.exp2(rng.uniform(-OCTAVES, OCTAVES, (n, 1))).astype(np.float32)).astype(np.float32)


def graded_queries(nq, dim, seed):
    rng = np.random.default_rng([seed, 2])
    return (rng.uniform(-1, 1, (nq, dim)) * 2.0 ** (-OCTAVES)).astype(np.float32)


def int8_rows(n, dim, seed):
    rng = np.random.default_rng([seed, 3])
    mag = np.exp2(rng.uniform(0, 7, (n, 1)))
    return np.clip(np.rint(rng.uniform(-1, 1, (n, dim)) * mag), -127, 127).astype(np.int8)


INT8_INV = 0.03125


class Case:
    """one handle + its queries + the oracle's sorted rows (depth-independent: a brute-force row at depth d is the
    first d entries of the full sort when no two distances are equal)"""

    def __init__(self, make_index, q, oi, od, n):
        self.make_index, self.q, self.oi, self.od, self.n = make_index, q, oi, od, n
        self._index = None
        self._plain = {}

    @property
    def index(self):
        if self._index is None:
            self._index = self.make_index()
        return self._index

    def plain(self, nq, depth):
        """the GPU's own plain search at k = depth (computed once per batch size and depth)"""
        if (nq, depth) not in self._plain:
            self._plain[(nq, depth)] = self.index.search_batched(self.q[:nq], depth)
        return self._plain[(nq, depth)]

    def oracle(self, i, depth):
        """(idx, dist) of the oracle's row for query i at k = depth; asserts depth + 1 strictly increasing distances"""
        d = min(depth, self.n)
        assert np.all(np.diff(self.od[i, :min(depth + 1, self.n)]) > 0), "oracle row has tied neighbours"
        return self.oi[i, :d], self.od[i, :d]


@functools.lru_cache(maxsize=None)
def bf_case(n, measure):
    seed = SEEDS[(n, measure)]
    rows = graded_rows(n, DIM, seed)
    data, stride = orc.to_strided(rows)
    q = graded_queries(64, DIM, seed)
    oi, od, _ = orc.bf_search_batched(data, n, DIM, stride, measure, q, min(2049, n))
    return Case(lambda: hip.bf_create(data, n, DIM, stride, measure), q, oi, od, n)


@functools.lru_cache(maxsize=None)
def int8_case():
    n, seed = 3001, SEEDS["int8"]
    rows = int8_rows(n, DIM, seed)
    rng = np.random.default_rng([seed, 2])
    q = (rng.uniform(-1, 1, (3, DIM)) * 0.01).astype(np.float32)
    d = qc.distances(q, rows, DIM, qc.ROWS_INT8, hip.SQUARED_L2, INT8_INV)
    order = np.stack([np.lexsort((np.arange(n), d[i])) for i in range(3)])[:, :2049]
    od = np.take_along_axis(d, order, axis=1).astype(np.float32)
    return Case(lambda: hip.bf_create_quantized(rows, n, DIM, DIM, hip.ROWS_INT8, hip.SQUARED_L2, INT8_INV), q,
                order.astype(np.uint32), od, n)


def attrs_of(family, n, depth, near):
    """uint64 attribute array of a family.  near: the rows query 0 finds nearest (near-block)."""
    i = np.arange(n, dtype=np.uint64)
    if family == "same":
        return np.full(n, 5, np.uint64)
    if family == "distinct":
        return i + np.uint64(1000)
    if family == "mod7":
        return i % np.uint64(7)
    if family == "low32":      # equal low words, different high words
        return ((i % np.uint64(9)) << np.uint64(32)) | np.uint64(0xDEADBEEF)
    if family == "slots":      # multiples of the table's slot count (and of every smaller power-of-two table)
        return (i % np.uint64(11)) * np.uint64(hip.crowd_table_slots(depth)) * np.uint64(12288)
    if family == "extremes":
        return np.where(i % np.uint64(2) == 0, np.uint64(0), U64)
    if family == "short":      # half the index has no entry: attribute 0, as the real zeros of the first half
        return (i[:n // 2] % np.uint64(3))
    assert family == "near-block"
    a = i + np.uint64(1000)
    a[near[:depth]] = np.uint64(77)
    return a


def check_rows(got, rows, attrs, limit, k, nq, what):
    """got = (idx, dist, cnt) of a crowded call; rows(i) -> (idx, dist) of the reference row of query i"""
    gi, gd, gc = got
    assert gi.shape == (nq, k) and gd.shape == (nq, k)
    for i in range(nq):
        ri, rd = rows(i)
        wi, wd = CM.apply_fast(ri, rd, attrs, limit, k)
        c = int(gc[i])
        assert c == wi.size, (what, i, c, wi.size)
        assert np.array_equal(gi[i, :c], wi), (what, i)
        assert np.array_equal(bits(gd[i, :c]), bits(wd)), (what, i)
        assert np.all(gi[i, c:] == SENT) and np.all(np.isposinf(gd[i, c:])), (what, i)


def limits_of(depth):
    return sorted({0, 1, 2, depth, 2 ** 32 - 1})


def ks_of(depth):
    return sorted({1, min(10, depth), depth})


def sweep(case, nq, family, depths=DEPTHS):
    index = case.index
    near = case.oi[0]
    for depth in depths:
        attrs = attrs_of(family, case.n, depth, near)
        index.set_crowding_attributes(attrs)
        pi, pd, pc = case.plain(nq, depth)
        for k in ks_of(depth):
            for limit in limits_of(depth):
                what = (family, depth, k, limit)
                got = index.search_crowded(case.q[:nq], k, depth, limit)
                check_rows(got, lambda i: (pi[i, :pc[i]], pd[i, :pc[i]]), attrs, limit, k, nq, ("A",) + what)
                check_rows(got, lambda i: case.oracle(i, depth), attrs, limit, k, nq, ("B",) + what)
                if family == "near-block" and limit == 1 and depth <= case.n:
                    assert got[2][0] == 1          # query 0's whole row is one crowd: shorter than k
                if limit >= depth:                   # the first k of the row
                    assert np.array_equal(got[0], pi[:, :k]) and np.array_equal(bits(got[1]), bits(pd[:, :k]))
                if limit == 0:
                    assert not got[2].any()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("nq", [3, 64])
@pytest.mark.parametrize("measure", [hip.SQUARED_L2, hip.DOT_PRODUCT])
@pytest.mark.parametrize("n", [3001, 20013])
def test_bf_crowded(n, measure, nq, family):
    """the direct (n = 3001) and the sampled (n = 20013) plan of the brute-force search, every depth around the wave
    size and up to the largest k.  nq = 3: reference (A) comes from the few-query pipeline (k <= 64) while the
    crowded call's search is the batched one, so (A) also holds the two pipelines against each other."""
    sweep(bf_case(n, measure), nq, family)


@pytest.mark.parametrize("family", ["mod7", "short", "near-block"])
def test_bf_crowded_l1(family):
    sweep(bf_case(3001, hip.L1), 64, family, depths=(10, 65, 2048))


@pytest.mark.parametrize("family", ["mod7", "short", "near-block"])
def test_bf_crowded_int8_rows(family):
    sweep(int8_case(), 3, family, depths=(10, 65, 2048))


def test_reference_vector_through_a_handle():
    """crowding.rs:275-299 through a handle: rows (i + 1, 0, 0, 0), query 0, attributes [0,0,0,1,1,2], limit 2"""
    rows = np.zeros((6, 4), np.float32)
    rows[:, 0] = np.arange(1, 7)
    data, stride = orc.to_strided(rows)
    index = hip.bf_create(data, 6, 4, stride, hip.SQUARED_L2)
    index.set_crowding_attributes([0, 0, 0, 1, 1, 2])
    gi, gd, gc = index.search_crowded(np.zeros((1, 4), np.float32), 6, 6, 2)
    assert gc[0] == 5 and gi[0, :5].tolist() == [0, 1, 3, 4, 5] and gi[0, 5] == SENT
    assert gd[0, :5].tolist() == [1.0, 4.0, 16.0, 25.0, 36.0] and np.isposinf(gd[0, 5])
    # depth beyond the index: the row is walked to its count
    gi, gd, gc = index.search_crowded(np.zeros((1, 4), np.float32), 6, 50, 1)
    assert gc[0] == 3 and gi[0, :3].tolist() == [0, 3, 5]


@pytest.mark.parametrize("family", ["f50", "lt-k"])
@pytest.mark.parametrize("n,nq", [(3001, 3), (20013, 64)])
def test_bf_crowded_with_allow_bitmap(n, nq, family):
    """the crowded row is the model over the FILTERED plain row; a short filtered row never reads its sentinel
    slots: the attribute of index 0 (what a clamped or wrapped sentinel lookup would most plausibly hit) is unique,
    and row 0 is not allowed"""
    case = bf_case(n, hip.SQUARED_L2)
    index = case.index
    k, depth = 10, 64
    words, cap = allow_of(family, n, k)
    words = words.copy()
    words[0] &= ~np.uint64(1)                       # row 0 is never allowed
    attrs = np.arange(n, dtype=np.uint64) % np.uint64(4) + np.uint64(1)
    attrs[0] = np.uint64(0xABCDEF)
    index.set_crowding_attributes(attrs)
    pi, pd, pc = index.search_batched(case.q[:nq], depth, allow=words, allow_bits=cap)
    allowed = H.allowed_ids(words, cap, n)
    if family == "lt-k":
        assert np.all(pc == allowed.size) and allowed.size < k
    for limit in (1, 3, depth):
        got = index.search_crowded(case.q[:nq], k, depth, limit, allow=words, allow_bits=cap)
        check_rows(got, lambda i: (pi[i, :pc[i]], pd[i, :pc[i]]), attrs, limit, k, nq, (family, limit))
        # (B): the oracle's full sort restricted to the allowed rows
        mask = np.zeros(n, bool)
        mask[allowed] = True
        oi_full, od_full, _ = _full_sort(n)

        def orow(i):
            keep = mask[oi_full[i]]
            return oi_full[i][keep][:depth], od_full[i][keep][:depth]
        check_rows(got, orow, attrs, limit, k, nq, ("B", family, limit))
        assert not np.any(got[0] == 0)
        if family == "lt-k" and limit == depth:
            assert np.all(got[2] == allowed.size)


@functools.lru_cache(maxsize=None)
def _full_sort(n):
    """the oracle's full sort of every row for the SquaredL2 case (strictly increasing: asserted)"""
    seed = SEEDS[(n, hip.SQUARED_L2)]
    data, stride = orc.to_strided(graded_rows(n, DIM, seed))
    oi, od, oc = orc.bf_search_batched(data, n, DIM, stride, hip.SQUARED_L2, graded_queries(64, DIM, seed), n)
    return oi, od, oc


def test_bf_crowded_ties_follow_the_plain_row():
    """duplicated rows with different attributes: who is kept follows the plain search's tie order -- (A) only"""
    n, nq = 3001, 64
    rows = H.adversarial_rows("duplicates", n, DIM, 7)
    q = H.adversarial_queries("duplicates", nq, DIM, 7, rows)
    data, stride = orc.to_strided(rows)
    index = hip.bf_create(data, n, DIM, stride, hip.SQUARED_L2)
    attrs = np.arange(n, dtype=np.uint64) % np.uint64(3)     # copies of one row carry different attributes
    index.set_crowding_attributes(attrs)
    for nq_ in (3, nq):
        for depth, k in ((64, 10), (1000, 1000)):
            pi, pd, pc = index.search_batched(q[:nq_], depth)
            assert np.any(np.diff(pd[:, :depth], axis=1) == 0)    # the rows do hold ties
            for limit in (1, 2, 40):
                got = index.search_crowded(q[:nq_], k, depth, limit)
                check_rows(got, lambda i: (pi[i, :pc[i]], pd[i, :pc[i]]), attrs, limit, k, nq_, (depth, k, limit))


# ---- hashed handles ---------------------------------------------------------------------------------------------
# query seeds for which no oracle row of 101 entries holds equal neighbours (checked on the CPU)
QUERY_SEEDS = {'txh': 78, 'ah': 78, 'partitioned': 80}
def _opts(pre_reorder_k=0, exact_reorder=1, P=0):
    o = hip.default_opts()
    o.pre_reorder_k, o.exact_reorder, o.partitions_to_search = pre_reorder_k, exact_reorder, P
    return o


@functools.lru_cache(maxsize=None)
def txh_case():
    rows, data, stride, ix, oix, kw = H.make_txh_case(4096, 128, L=16, S=32, seed=31, P=4)
    q = synth.uniform_f32(64, 128, QUERY_SEEDS['txh'])

    def oracle(i, depth):   # m = 100 * 3.0 = 300 candidates, the depth + 1 best of them by exact distance
        r = orc.txh_search(oix, q[i], depth, stages=True)
        more = orc.reorder(data, stride, 128, q[i], r[4], depth + 1)
        return r[0], r[1], more[1]
    return kw, q, oracle, 4096


@functools.lru_cache(maxsize=None)
def ah_case():
    rows, data, stride, ix, kw = H.make_ah_case(2000, 64, S=16, seed=32)
    q = synth.uniform_f32(64, 64, QUERY_SEEDS['ah'])

    def oracle(i, depth):
        oi, od = orc.ah_search_with_reordering(ix["codebook"], ix["codes"], data, stride, q[i], depth, 300)
        more = orc.ah_search_with_reordering(ix["codebook"], ix["codes"], data, stride, q[i], depth + 1, 300)
        return oi, od, more[1]
    return kw, q, oracle, 2000


@functools.lru_cache(maxsize=None)
def partitioned_case():
    n, dim, L, P = 3000, 64, 20, 5
    rows = synth.uniform_f32(n, dim, 33)
    data, stride = orc.to_strided(rows)
    centers, assign = trainer.kmeans(rows, L, iters=3, seed=33)
    leaf_ids = np.argsort(assign, kind="stable").astype(np.uint32)
    leaf_off = np.zeros(centers.shape[0] + 1, np.uint32)
    leaf_off[1:] = np.cumsum(np.bincount(assign, minlength=centers.shape[0]))
    kw = dict(data=data, n_rows=n, dim=dim, stride=stride, centers=centers, leaf_offsets=leaf_off, leaf_ids=leaf_ids,
              codebook=None, codes=None, partitions_to_search=P, distance_measure=hip.SQUARED_L2)
    q = synth.uniform_f32(64, dim, QUERY_SEEDS['partitioned'])

    def oracle(i, depth):
        oi, od = orc.scann_search_partitioned(centers, leaf_off, leaf_ids, data, stride, hip.SQUARED_L2, q[i], P, depth)
        more = orc.scann_search_partitioned(centers, leaf_off, leaf_ids, data, stride, hip.SQUARED_L2, q[i], P,
                                            depth + 1)
        return oi, od, more[1]
    return kw, q, oracle, n


HASHED = {"txh": (txh_case, lambda: _opts(pre_reorder_k=300)), "ah": (ah_case, lambda: _opts(pre_reorder_k=300)),
          "partitioned": (partitioned_case, lambda: _opts())}


@pytest.mark.parametrize("nq", [3, 64])
@pytest.mark.parametrize("kind", sorted(HASHED))
def test_hashed_crowded(kind, nq):
    """Tree-X-Hybrid, flat hasher (pre_reorder_k = 300) and Partitioned mode; at nq = 3 the plain row of (A) comes
    from the small-batch pipeline, at nq = 64 from the batched one"""
    make, opts = HASHED[kind]
    kw, q, oracle, n = make()
    index = hip.txh_create(**kw)
    depth, k = 100, 10
    pi, pd, pc = index.search_batched(q[:nq], depth, opts=opts())
    orows = [oracle(i, depth) for i in range(nq)]
    for i in range(nq):
        assert np.all(np.diff(orows[i][2]) > 0), "oracle row has tied neighbours"
    for attrs in (np.arange(n, dtype=np.uint64) % np.uint64(7),
                  ((np.arange(n, dtype=np.uint64) % np.uint64(13)) << np.uint64(32)) | np.uint64(1)):
        index.set_crowding_attributes(attrs)
        for limit in (1, 3):
            got = index.search_crowded(q[:nq], k, depth, limit, opts=opts())
            check_rows(got, lambda i: (pi[i, :pc[i]], pd[i, :pc[i]]), attrs, limit, k, nq, ("A", kind, limit))
            check_rows(got, lambda i: orows[i][:2], attrs, limit, k, nq, ("B", kind, limit))


# ---- device entry point -------------------------------------------------------------------------------------------
def _device_crowded(index, qd, k, depth, limit, stream, outs, opts=None):
    import torch
    L = hip.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    nq, dim = qd.shape
    hip.check(L.scann_hip_search_crowded_device(index.h, p(qd), nq, dim, k, depth, limit,
                                                ctypes.byref(opts) if opts is not None else None, p(outs[0]),
                                                p(outs[1]), p(outs[2]), ctypes.c_void_p(stream.cuda_stream)))


@pytest.mark.parametrize("kind", ["bf", "txh"])
def test_device_entry_point_two_streams(kind):
    """after reserve, on two streams: rows equal the host entry's; a second call with another limit and no set in
    between sees no stale table state; no allocation (free device memory unchanged)"""
    import torch
    dev = torch.device("cuda:0")
    L = hip.load()
    if kind == "bf":
        case = bf_case(20013, hip.SQUARED_L2)
        index, q, n, opts = case.index, case.q, case.n, None
        k, depth = 10, 512
    else:
        kw, q, _, n = txh_case()
        index, opts = hip.txh_create(**kw), _opts(pre_reorder_k=300)
        k, depth = 10, 100
    nq = 64
    attrs = np.arange(n, dtype=np.uint64) % np.uint64(7)
    index.set_crowding_attributes(attrs)
    want = {limit: index.search_crowded(q[:nq], k, depth, limit, opts=opts) for limit in (1, 3)}
    qd = torch.from_numpy(np.ascontiguousarray(q[:nq])).to(dev)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    outs = [(torch.zeros((nq, k), dtype=torch.int32, device=dev), torch.zeros((nq, k), dtype=torch.float32, device=dev),
             torch.zeros(nq, dtype=torch.int32, device=dev)) for _ in streams]
    hip.check(L.scann_hip_index_reserve_crowded(index.h, nq, k, depth, ctypes.byref(opts) if opts is not None else None))
    for s, o in zip(streams, outs):      # each stream binds its workspace on its first call
        _device_crowded(index, qd, k, depth, 2, s, o, opts)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(dev)[0]
    for limit in (1, 3, 1):
        for s, o in zip(streams, outs):
            _device_crowded(index, qd, k, depth, limit, s, o, opts)
        for s, o in zip(streams, outs):
            assert L.scann_hip_index_last_device_status(index.h, ctypes.c_void_p(s.cuda_stream)) == hip.OK
            s.synchronize()
            gi, gd, gc = (t.cpu().numpy() for t in o)
            assert np.array_equal(gi.view(np.uint32), want[limit][0]), (kind, limit)
            assert np.array_equal(bits(gd), bits(want[limit][1]))
            assert np.array_equal(gc.view(np.uint32), want[limit][2])
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(dev)[0] == free0


# ---- errors ---------------------------------------------------------------------------------------------------------
def _code(fn):
    try:
        fn()
    except hip.ScannError as e:
        return e.code
    return hip.OK


def test_errors():
    case = bf_case(3001, hip.SQUARED_L2)
    q = case.q[:3]
    data, stride = orc.to_strided(graded_rows(300, DIM, 1))
    index = hip.bf_create(data, 300, DIM, stride, hip.SQUARED_L2)
    # no attributes attached
    assert _code(lambda: index.search_crowded(q, 5, 10, 1)) == hip.FAILED_PRECONDITION
    index.set_crowding_attributes(np.arange(300) % 3)
    assert _code(lambda: index.search_crowded(q, 5, 10, 1)) == hip.OK
    # depth < k
    assert _code(lambda: index.search_crowded(q, 11, 10, 1)) == hip.INVALID_ARGUMENT
    # depth = 0 means depth = k
    a = index.search_crowded(q, 7, 0, 1)
    b = index.search_crowded(q, 7, 7, 1)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and np.all(a[2] >= 1) and np.all(a[2] <= 3)
    # a depth the handle does not accept as k: the plain search's error
    big = case.index
    big.set_crowding_attributes(np.arange(case.n) % 3)
    plain = _code(lambda: big.search_batched(q, 2049))
    assert plain == hip.UNIMPLEMENTED and _code(lambda: big.search_crowded(q, 5, 2049, 1)) == plain
    # a depth beyond the index is legal on the host path: the row is walked to its count
    assert np.all(index.search_crowded(q, 5, 2049, 2 ** 32 - 1)[2] == 5)
    assert np.all(index.search_crowded(q, 300, 2049, 2 ** 32 - 1)[2] == 300)
    # wrong query dimensionality: the plain search's error
    assert _code(lambda: index.search_crowded(q[:, :8], 5, 10, 1)) == _code(lambda: index.search_batched(q[:, :8], 10))
    # detached again
    index.set_crowding_attributes(None)
    assert _code(lambda: index.search_crowded(q, 5, 10, 1)) == hip.FAILED_PRECONDITION
    # hashed handle: a candidate count above the handle's limit
    kw, hq, _, n = ah_case()
    ah = hip.txh_create(**kw)
    ah.set_crowding_attributes(np.arange(n) % 3)
    plain = _code(lambda: ah.search_batched(hq[:3], 9000, opts=_opts(exact_reorder=0)))
    assert plain == hip.UNIMPLEMENTED
    assert _code(lambda: ah.search_crowded(hq[:3], 5, 9000, 1, opts=_opts(exact_reorder=0))) == plain
    assert _code(lambda: ah.search_crowded(hq[:3], 5, 4, 1)) == hip.INVALID_ARGUMENT


def test_device_errors():
    import torch
    dev = torch.device("cuda:0")
    L = hip.load()
    data, stride = orc.to_strided(graded_rows(300, DIM, 1))
    index = hip.bf_create(data, 300, DIM, stride, hip.SQUARED_L2)
    qd = torch.zeros((4, DIM), dtype=torch.float32, device=dev)
    outs = (torch.zeros((4, 8), dtype=torch.int32, device=dev), torch.zeros((4, 8), dtype=torch.float32, device=dev),
            torch.zeros(4, dtype=torch.int32, device=dev))
    s = torch.cuda.current_stream(dev)
    assert _code(lambda: _device_crowded(index, qd, 8, 16, 1, s, outs)) == hip.FAILED_PRECONDITION
    index.set_crowding_attributes(np.arange(300) % 3)
    assert _code(lambda: _device_crowded(index, qd, 8, 4, 1, s, outs)) == hip.INVALID_ARGUMENT
    # a depth the handle does not accept as k on the device path (k > n; k > 2048): the plain device search's error
    big = (torch.zeros((4, 301), dtype=torch.int32, device=dev), torch.zeros((4, 301), dtype=torch.float32, device=dev),
           outs[2])
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    plain = lambda kk: _code(lambda: hip.check(L.scann_hip_search_batched_device(
        index.h, p(qd), 4, DIM, kk, None, p(big[0]), p(big[1]), p(big[2]), ctypes.c_void_p(s.cuda_stream))))
    assert plain(301) == hip.INVALID_ARGUMENT
    assert _code(lambda: _device_crowded(index, qd, 8, 301, 1, s, outs)) == hip.INVALID_ARGUMENT
    assert _code(lambda: _device_crowded(index, qd, 8, 9000, 1, s, outs)) == hip.UNIMPLEMENTED
    assert _code(lambda: hip.check(L.scann_hip_index_reserve_crowded(index.h, 4, 8, 4, None))) == hip.INVALID_ARGUMENT
    assert _code(lambda: _device_crowded(index, qd, 8, 16, 1, s, outs)) == hip.OK
    torch.cuda.synchronize()


# ---- exact crowded brute force ----------------------------------------------------------------------------------------
def test_search_crowded_exact():
    case = bf_case(3001, hip.SQUARED_L2)
    index, n = case.index, case.n
    oi, od, _ = _full_sort(n)
    # near block: the 40 nearest rows of query 0 share one attribute -> depth 10, 20, 40 hold one or two entries
    attrs = np.arange(n, dtype=np.uint64) + np.uint64(1000)
    attrs[oi[0, :40]] = np.uint64(77)
    index.set_crowding_attributes(attrs)
    assert index.search_crowded(case.q[:1], 10, 10, 1)[2][0] == 1
    (gi, gd), complete = index.search_crowded_exact(case.q[0], 10, 1)
    assert np.all(np.diff(od[0]) > 0)
    wi, wd = CM.apply(oi[0], od[0], attrs, 1, 10)
    assert complete and np.array_equal(gi, wi) and np.array_equal(bits(gd), bits(wd))
    assert gi[0] == oi[0, 0] and gi[1] == oi[0, 40]
    # all rows one crowd: the whole index is walked when it fits the largest k, otherwise the answer is incomplete
    index.set_crowding_attributes(np.full(n, 9, np.uint64))
    (gi, gd), complete = index.search_crowded_exact(case.q[0], 10, 1)
    assert gi.tolist() == [oi[0, 0]] and not complete
    rows = graded_rows(1500, DIM, 1)
    data, stride = orc.to_strided(rows)
    small = hip.bf_create(data, 1500, DIM, stride, hip.SQUARED_L2)
    small.set_crowding_attributes(np.full(1500, 9, np.uint64))
    (gi, gd), complete = small.search_crowded_exact(case.q[0], 10, 1)
    want = orc.bf_search(data, 1500, DIM, stride, hip.SQUARED_L2, case.q[0], 1)
    assert gi.tolist() == want[0].tolist() and complete


def test_host_cpp_crowding_through_handles():
    """scann.hpp: search_with_crowding and search_crowded_exact on the reference's vector"""
    import os
    import subprocess
    from scann_rust_amd import build
    exe = os.path.join(os.path.dirname(os.path.abspath(build.__file__)), "host", "crowding_test")
    if not os.path.exists(exe):
        build.build_host()
    r = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "crowding_test ok" in r.stdout

"""Mutable indexes on the device (include/scann_hip.h "mutable indexes"): every result compared with
tests/mutable_model.py -- the numpy state machine of MutableDataset plus the expected search built on the CPU oracle.

Brute-force bases are compared exactly (ids) and bitwise (distances) with the oracle's search over the live rows in
ascending id order; the data makes ties decide (rows duplicated across base and delta, a LOW id updated to a copy of a
higher row so that it sits in a late delta slot and must still win its tie at the top-k boundary).  Tree and flat-hasher
bases use continuous data (the oracle's rows have no equal adjacent distances: asserted) and the base part of the
expected answer is the oracle's filtered search under the live bitmap."""
import threading

import numpy as np
import pytest

import helpers as H
import mutable_model as mm
from oracle import pyoracle as orc
from scann_rust_amd import hip, synth

pytestmark = pytest.mark.gpu

T = hip.MUTABLE_DELTA_TILE
EMPTY = 0xFFFFFFFF
MEASURES = (hip.SQUARED_L2, hip.L2, hip.DOT_PRODUCT, hip.L1, hip.COSINE)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Pair:
    """the library's handle and the model, driven together: same calls, same answers, same errors"""

    def __init__(self, base, base_rows, capacity):
        self.mut = hip.Mutable(base, capacity)
        self.model = mm.MutableModel(base_rows, capacity)

    def _both(self, name, *args):
        err = None
        try:
            want = getattr(self.model, name)(*args)
        except mm.ModelError as e:
            err = e
        if err is not None:
            with pytest.raises(hip.ScannError) as e:
                getattr(self.mut, name)(*args)
            assert e.value.code == err.code, (name, e.value, err)
            raise err
        got = getattr(self.mut, name)(*args)
        if want is not None:
            assert np.array_equal(got, want), (name, got, want)
        self.same_counters()
        return got

    def add(self, rows):
        return self._both("add", rows)

    def remove(self, ids):
        return self._both("remove", ids)

    def update(self, ids, rows):
        return self._both("update", ids, rows)

    def same_counters(self):
        assert self.mut.size() == self.model.size() and self.mut.pending() == self.model.pending()

    def same_rows(self, ids):
        for id in ids:
            id = int(id)
            assert self.mut.exists(id) == self.model.exists(id), id
            if self.model.exists(id):
                assert np.array_equal(_bits(self.mut.get(id)), _bits(self.model.get(id))), id
            else:
                with pytest.raises(hip.ScannError) as e:
                    self.mut.get(id)
                assert e.value.code == hip.NOT_FOUND

    def close(self):
        self.mut.close()


def same_as(got, want, k, what):
    """got: (idx, dist, cnt) of the library; want: per query (ids, dists) of the model: exact ids, bitwise distances"""
    idx, dist, cnt = got
    assert idx.shape == (len(want), k) and dist.shape == (len(want), k)
    for i, (wi, wd) in enumerate(want):
        c = int(cnt[i])
        assert c == wi.size, "%s q%d: count %d, want %d" % (what, i, c, wi.size)
        assert np.array_equal(_bits(dist[i, :c]), _bits(wd)), "%s q%d: distances\n got %s\nwant %s" % (what, i, dist[i, :c], wd)
        assert np.array_equal(idx[i, :c], wi), "%s q%d: ids\n got %s\nwant %s\n%s" % (what, i, idx[i, :c], wi, wd)
        assert np.all(idx[i, c:] == EMPTY) and np.all(np.isposinf(dist[i, c:])), "%s q%d: unused slots" % (what, i)


def check_bf(p, measure, q, k, what, allow=None, allow_bits=None):
    got = p.mut.search_batched(q, k, allow=allow, allow_bits=allow_bits)
    same_as(got, p.model.search_bf(measure, q, k, allow, allow_bits), k, what)


def bf_base(n, dim, measure, seed):
    rows = synth.uniform_f32(n, dim, seed) - np.float32(0.5)
    rows[H.duplicate_protos(n)[1:]] = rows[0]          # duplicates inside the base
    data, stride = orc.to_strided(rows)
    return rows, hip.bf_create(data, n, dim, stride, measure)


def mutation_script(p, new_rows, check, tie_update=None, duplicates=True):
    """the issue's script, a search after each phase: add 70 rows; remove 40 base and 10 delta ids; update 15 base and
    5 delta ids (then tie_update(up) as a batch of its own: the last slot); update 3 removed ids; remove one id twice.
    new_rows: at least 100 fresh rows.  Returns the ids it touched."""
    base_ids, base_rows = p.model.base_ids.copy(), p.model.base_rows.copy()
    n = base_ids.size
    nr = iter(new_rows)
    add = np.stack([next(nr) for _ in range(70)])
    if duplicates:
        add[::9] = base_rows[:: max(1, n // 8)][:8]     # copies of base rows in the delta
        add[5] = add[3]                                   # and a duplicate inside the delta
    ids = p.add(add)
    assert ids.tolist() == list(range(p.model.next_index - 70, p.model.next_index))
    check("add")
    rm = np.concatenate([base_ids[(np.arange(40) * 13 + 2) % n], ids[::7]])
    assert rm.size == 50 and np.unique(rm).size == 50
    p.remove(rm)
    check("remove")
    up = np.concatenate([np.setdiff1d(base_ids, rm)[5::29][:15], ids[1::14]])
    assert up.size == 20 and not np.intersect1d(up, rm).size
    upr = np.stack([next(nr) for _ in range(20)])
    if duplicates:
        upr[0] = base_rows[n // 2]                        # an updated base id equal to a live base row
        upr[16] = base_rows[n // 3]                       # a delta row overwritten in place with a copy of a base row
    p.update(up, upr)
    if tie_update is not None:      # a batch of its own behind the others: the last slot
        tid, trow = tie_update(up)
        p.update(tid, trow)
        up = np.append(up, tid)
    check("update")
    rev = np.array([rm[0], rm[17], rm[45]])               # two removed base ids, one removed delta id
    p.update(rev, np.stack([next(nr) for _ in range(3)]))
    check("revive")
    p.remove(rm[3])
    p.remove(rm[3])
    p.remove([rm[44], rm[44]])
    check("remove twice")
    touched = np.concatenate([ids, rm, up, rev])
    p.same_rows(touched)
    return touched


# ---- 1. brute-force base: exact ids, bitwise distances, ties decided by (distance, external id) -------------------
@pytest.mark.parametrize("dim", [24, 19])
@pytest.mark.parametrize("measure", MEASURES)
def test_bf_script_is_exact(measure, dim):
    n, nq, k = 600, 9, 10
    rows, base = bf_base(n, dim, measure, 11 + dim)
    q = synth.uniform_f32(nq, dim, 12 + dim) - np.float32(0.5)
    q[1] = rows[0]
    p = Pair(base, rows, 128)
    cut = {}

    def tie_update(up):
        # a LOW live base id becomes a copy of the row at rank k - 1 of some query: it takes that rank (lower id) from a
        # late delta slot and pushes the original out of the top k
        for j in range(nq):
            wi, wd = p.model.search_bf(measure, q[j:j + 1], k + 6)[0]
            h = int(wi[k - 1])
            if wd[k - 2] == wd[k - 1] or wd[k - 1] == wd[k] or h < 50 or h in up.tolist():
                continue
            low = [i for i in range(40) if p.model.exists(i) and p.model.slot(i) is None and i not in wi.tolist()
                   and i not in up.tolist()]
            if low:
                cut.update(j=j, low=low[0], high=h)
                return low[0], p.model.get(h)
        raise AssertionError("no query whose k-th neighbour can be tied")

    def check(what):
        check_bf(p, measure, q, k, what)
        if what == "update":
            # the top-k boundary of the oracle falls inside the tie group: low id in, high id out, equal distance bits
            wi, wd = p.model.search_bf(measure, q[cut["j"]:cut["j"] + 1], k + 1)[0]
            assert wi[k - 1] == cut["low"] and wi[k] == cut["high"] and _bits(wd)[k - 1] == _bits(wd)[k]
            assert p.model.slot(cut["low"]) == len(p.model.delta_ids) - 1       # the last slot
            check_bf(p, measure, q, k + 1, "k + 1")

    mutation_script(p, synth.uniform_f32(100, dim, 13 + dim) - np.float32(0.5), check, tie_update)
    assert cut
    p.close()


# ---- 2. edges ------------------------------------------------------------------------------------------------------
def test_bf_edges():
    n, dim, measure = 600, 24, hip.SQUARED_L2
    rows, base = bf_base(n, dim, measure, 21)
    q = synth.uniform_f32(5, dim, 22) - np.float32(0.5)
    p = Pair(base, rows, 64)
    # no mutation at all: the plain search of the base, the same kernel
    for qq in (q, synth.uniform_f32(40, dim, 24) - np.float32(0.5)):   # the few-query pipeline and the batched one
        base.enable_timing(True)
        ref = base.search_batched(qq, 10)
        name_plain = base.last_kernel_ms()[1]
        base.enable_timing(True)
        got = p.mut.search_batched(qq, 10)
        assert base.last_kernel_ms()[1] == name_plain and (name_plain or qq.shape[0] <= 16)
        base.enable_timing(False)
        for a, b in zip(got, ref):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    check_bf(p, measure, q, 10, "no mutation")
    # k = 0; k larger than the live count
    idx, dist, cnt = p.mut.search_batched(q, 0)
    assert idx.shape == (5, 0) and not cnt.any()
    check_bf(p, measure, q, 700, "k > live, no mutation")
    # tombstones only, empty delta
    p.remove(np.arange(0, n, 3))
    check_bf(p, measure, q, 10, "tombstones only")
    check_bf(p, measure, q, 700, "k > live, tombstones")
    # delta and tombstones; k > live
    ids = p.add(synth.uniform_f32(30, dim, 23) - np.float32(0.5))
    check_bf(p, measure, q, 700, "k > live")
    # every base row removed: the delta alone
    p.remove(np.arange(n))
    assert p.mut.size() == 30
    check_bf(p, measure, q, 10, "delta only")
    check_bf(p, measure, q, 64, "delta only, k > live")
    # every row removed
    p.remove(ids)
    assert p.mut.size() == 0
    idx, dist, cnt = p.mut.search_batched(q, 10)
    assert not cnt.any() and np.all(idx == EMPTY) and np.all(np.isposinf(dist))
    p.close()


# ---- 3. delta tile edges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [1, T - 1, T, T + 1, 2 * T + 3])
def test_delta_tile_edges(size):
    n, dim, measure = 600, 24, hip.SQUARED_L2
    rows, base = bf_base(n, dim, measure, 31)
    p = Pair(base, rows, 2 * T + 16)
    new = synth.uniform_f32(size + 6, dim, 32 + size) - np.float32(0.5)
    new[7::50] = rows[7]                       # ties across tiles and with the base
    if size > T:
        new[T + 2] = new[3]
    ids = p.add(new)
    p.remove(ids[:6])                          # swap-removes: the last rows move to the first slots
    assert len(p.model.delta_ids) == size and (size < 7 or p.model.delta_ids[0] > p.model.delta_ids[6])
    q17 = synth.uniform_f32(17, dim, 33) - np.float32(0.5)
    q17[2] = rows[7]
    for nq in (1, 17):
        for k in (1, 10):
            check_bf(p, measure, q17[2:2 + nq] if nq == 1 else q17, k, "delta %d nq %d k %d" % (size, nq, k))
    if size == 2 * T + 3:
        check_bf(p, measure, q17[:3], min(hip.MUTABLE_MAX_K, p.mut.size()), "largest k")
        check_bf(p, measure, q17[:3], 700, "k 700")   # 600 + 3 * 700 keys: more than one round of the merge buffer
    p.close()


# ---- 4. tree and flat-hasher bases ---------------------------------------------------------------------------------
def _no_ties(want):
    for wi, wd in want:
        assert np.all(np.diff(wd) > 0), "the oracle's row has equal adjacent distances"


def check_lists(got, want, k, what):
    idx, dist, cnt = got
    _no_ties(want)
    for i, (wi, wd) in enumerate(want):
        c = int(cnt[i])
        assert c == wi.size, "%s q%d: count %d, want %d" % (what, i, c, wi.size)
        H.assert_topk_equal_up_to_ties(idx[i, :c], dist[i, :c], wi, wd, rel=0.0, what="%s q%d" % (what, i))
        assert np.all(idx[i, c:] == EMPTY) and np.all(np.isposinf(dist[i, c:]))


@pytest.fixture(scope="module")
def txh_case():
    rows, data, stride, ix, oix, kw = H.make_txh_case(2000, 64, 16, 16, seed=41, P=4, kmeans_iters=3, pq_iters=3)
    assert not np.array_equal(ix["leaf_ids"], np.arange(2000)), "leaf_ids must be a real permutation"
    return rows, oix, kw, hip.txh_create(**kw)


@pytest.fixture(scope="module")
def ah_case():
    rows, data, stride, ix, kw = H.make_ah_case(2000, 64, 16, seed=42, pq_iters=3)
    return rows, ix, kw, hip.txh_create(**kw)


def test_txh_base_script(txh_case):
    rows, oix, kw, base = txh_case
    q = synth.uniform_f32(9, 64, 43)
    k = 10
    p = Pair(base, rows, 128)

    def check(what):
        check_lists(p.mut.search_batched(q, k), p.model.search_txh(oix, q, k), k, "txh " + what)

    check("no mutation")
    mutation_script(p, synth.uniform_f32(100, 64, 44), check, duplicates=False)
    # pre_reorder_k = k: the base's candidates are its k best approximate rows; a delta row is returned regardless
    near = q[0] + np.float32(1e-3)
    nid = p.add(near)
    o = hip.default_opts()
    o.pre_reorder_k = k
    got = p.mut.search_batched(q, k, opts=o)
    want = p.model.search_txh(oix, q, k, pre_reorder_k=k)
    check_lists(got, want, k, "txh pre_reorder_k = k")
    assert got[0][0, 0] == nid
    p.close()


def test_ah_base_script(ah_case):
    rows, ix, kw, base = ah_case
    q = synth.uniform_f32(9, 64, 45)
    k, m = 10, 30
    p = Pair(base, rows, 128)
    o = hip.default_opts()
    o.pre_reorder_k = m

    def check(what):
        check_lists(p.mut.search_batched(q, k, opts=o), p.model.search_ah(ix["codebook"], ix["codes"], q, k, m), k,
                    "ah " + what)

    check("no mutation")
    mutation_script(p, synth.uniform_f32(100, 64, 46), check, duplicates=False)
    o.pre_reorder_k = k
    nid = p.add(q[3] + np.float32(1e-3))
    got = p.mut.search_batched(q, k, opts=o)
    check_lists(got, p.model.search_ah(ix["codebook"], ix["codes"], q, k, k), k, "ah pre_reorder_k = k")
    assert got[0][3, 0] == nid
    p.close()


# ---- 5. user filter combined with tombstones -----------------------------------------------------------------------
def _filters(p, n):
    """(name, words, capacity) over external ids: below the first delta id, in the middle of the delta ids, 0, only
    removed ids, and a mixed one"""
    nxt = p.model.next_index
    full = lambda cap: np.full(max(1, -(-cap // 64)), np.uint64(0xFFFFFFFFFFFFFFFF))
    removed = [i for i in range(nxt) if p.model.known(i) and not p.model.exists(i)]
    assert len(removed) >= 10
    mixed = np.flatnonzero(np.random.default_rng(5).random(nxt) < 0.3)
    return [("no delta id", full(n), n), ("mid delta", full(n + 35), n + 35), ("capacity 0", full(0), 0),
            ("only removed", H.words_of(removed, nxt)[0], nxt), ("mixed", H.words_of(mixed, nxt)[0], nxt),
            ("mixed, short capacity", H.words_of(mixed, nxt)[0], n + 11)]


def test_bf_filter_with_tombstones():
    n, dim, measure = 600, 24, hip.DOT_PRODUCT
    rows, base = bf_base(n, dim, measure, 51)
    q = synth.uniform_f32(9, dim, 52) - np.float32(0.5)
    p = Pair(base, rows, 128)
    mutation_script(p, synth.uniform_f32(100, dim, 53) - np.float32(0.5), lambda what: None)
    for name, words, cap in _filters(p, n):
        check_bf(p, measure, q, 10, "filter " + name, allow=words, allow_bits=cap)
        check_bf(p, measure, q, 10, "after " + name)       # a filter used in one call does not stick
        if name in ("capacity 0", "only removed"):
            assert not p.mut.search_batched(q, 10, allow=words, allow_bits=cap)[2].any()
    o = hip.default_opts()                                   # a caller's opts keep their own filter across a call with allow=
    own = H.words_of([3, 4, 601], 700)[0]
    o.allow_bitmap, o.allow_bitmap_bits = hip.ptr(own, hip.u64p), 700
    p.mut.search_batched(q, 10, opts=o, allow=np.zeros(1, np.uint64), allow_bits=64)
    assert o.allow_bitmap_bits == 700
    same_as(p.mut.search_batched(q, 10, opts=o), p.model.search_bf(measure, q, 10, own, 700), 10, "the opts' own filter")
    o = hip.default_opts()                                   # nor through a caller's opts
    p.mut.search_batched(q, 10, opts=o, allow=np.zeros(1, np.uint64), allow_bits=64)
    same_as(p.mut.search_batched(q, 10, opts=o), p.model.search_bf(measure, q, 10), 10, "same opts, no filter")
    p.close()


def test_txh_filter_with_tombstones(txh_case):
    rows, oix, kw, base = txh_case
    n, k = 2000, 10
    q = synth.uniform_f32(9, 64, 54)
    p = Pair(base, rows, 128)
    mutation_script(p, synth.uniform_f32(100, 64, 55), lambda what: None, duplicates=False)
    for name, words, cap in _filters(p, n):
        got = p.mut.search_batched(q, k, allow=words, allow_bits=cap)
        check_lists(got, p.model.search_txh(oix, q, k, allow=words, allow_bits=cap), k, "txh filter " + name)
        check_lists(p.mut.search_batched(q, k), p.model.search_txh(oix, q, k), k, "txh after " + name)
    p.close()


# ---- 6. export and rebase ------------------------------------------------------------------------------------------
def test_export_and_rebase():
    n, dim, measure = 600, 24, hip.SQUARED_L2
    rows, base = bf_base(n, dim, measure, 61)
    q = synth.uniform_f32(9, dim, 62) - np.float32(0.5)
    p = Pair(base, rows, 128)
    touched = mutation_script(p, synth.uniform_f32(100, dim, 63) - np.float32(0.5), lambda what: None)
    er, ei = p.mut.export_live()
    wr, wi = p.model.export_live()
    assert np.array_equal(ei, wi) and np.array_equal(_bits(er), _bits(wr))
    before = p.mut.search_batched(q, 10)
    data, stride = orc.to_strided(er)
    nb = hip.bf_create(data, ei.size, dim, stride, measure)
    with pytest.raises(hip.ScannError) as e:                  # not ascending
        p.mut.rebase(nb, ei[::-1].copy())
    assert e.value.code == hip.INVALID_ARGUMENT
    with pytest.raises(hip.ScannError) as e:                  # n differs from the base's size
        hip.check(hip.load().scann_hip_mutable_rebase(p.mut.h, nb.h, hip.ptr(ei, hip.u32p), ei.size - 1))
    assert e.value.code == hip.INVALID_ARGUMENT
    same_as(p.mut.search_batched(q, 10), p.model.search_bf(measure, q, 10), 10, "after refused rebases")
    p.mut.rebase(nb, ei)
    p.model.rebase(wr, wi)
    p.same_counters()
    assert p.mut.pending() == 0 and p.mut.size() == ei.size
    after = p.mut.search_batched(q, 10)
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    p.same_rows(touched)
    dropped = [int(i) for i in touched if not p.model.known(int(i))]
    assert dropped
    for call in (lambda i: p.mut.remove(i), lambda i: p.mut.update(i, rows[0]), lambda i: p.mut.get(i)):
        with pytest.raises(hip.ScannError) as e:
            call(dropped[0])
        assert e.value.code == hip.NOT_FOUND
    # the script again on the non-dense ids, under a user bitmap over external ids (the gather form of the bitmap kernel)
    assert not p.model.identity and not np.array_equal(p.model.base_ids, np.arange(p.model.base_ids.size))
    nxt = p.model.next_index + 80
    words = H.words_of(np.flatnonzero(np.random.default_rng(6).random(nxt) < 0.5), nxt)[0]

    def check(what):
        check_bf(p, measure, q, 10, "rebased " + what)
        check_bf(p, measure, q, 10, "rebased, filtered " + what, allow=words, allow_bits=nxt - 40)

    check("no mutation")
    mutation_script(p, synth.uniform_f32(100, dim, 64) - np.float32(0.5), check)
    er, ei = p.mut.export_live()
    wr, wi = p.model.export_live()
    assert np.array_equal(ei, wi) and np.array_equal(_bits(er), _bits(wr))
    p.close()


# ---- 7. errors and limits: host-side refusals ----------------------------------------------------------------------
def _refused(code, f):
    with pytest.raises(hip.ScannError) as e:
        f()
    assert e.value.code == code, e.value


def test_unsupported_bases_and_options(txh_case, ah_case):
    rows, oix, kw, txh = txh_case
    n, dim = rows.shape
    codes8, inv = hip.symmetric_int8(rows)
    quant = hip.bf_create_quantized(np.ascontiguousarray(codes8), n, dim, dim, hip.ROWS_INT8, hip.SQUARED_L2, inv)
    _refused(hip.UNIMPLEMENTED, lambda: hip.Mutable(quant, 16))
    part = hip.txh_create(**dict(kw, codebook=None, codes=None))
    _refused(hip.UNIMPLEMENTED, lambda: hip.Mutable(part, 16))
    lid = np.asarray(kw["leaf_ids"], np.int64)
    shard = hip.txh_create(**dict(kw, data=np.ascontiguousarray(kw["data"].reshape(n, -1)[lid]),
                                  leaf_sizes_global=np.diff(np.asarray(kw["leaf_offsets"], np.int64)).astype(np.uint32),
                                  data_is_csr_order=True))
    _refused(hip.UNIMPLEMENTED, lambda: hip.Mutable(shard, 16))
    csr = hip.txh_create(**dict(kw, data=np.ascontiguousarray(kw["data"].reshape(n, -1)[lid]), data_is_csr_order=True))
    _refused(hip.UNIMPLEMENTED, lambda: hip.Mutable(csr, 16))       # rows in CSR order, not a shard
    norows = hip.txh_create(**dict(ah_case[2], data=None))
    _refused(hip.UNIMPLEMENTED, lambda: hip.Mutable(norows, 16))
    _refused(hip.INVALID_ARGUMENT, lambda: hip.Mutable(txh, 0))
    _refused(hip.INVALID_ARGUMENT, lambda: hip.Mutable(txh, hip.MUTABLE_MAX_CAPACITY + 1))
    m = hip.Mutable(txh, 16)
    q = synth.uniform_f32(3, dim, 71)
    o = hip.default_opts()
    o.exact_reorder = 0
    _refused(hip.UNIMPLEMENTED, lambda: m.search_batched(q, 5, opts=o))
    m.add(q[0])
    _refused(hip.UNIMPLEMENTED, lambda: m.search_batched(q, 5, opts=o))
    _refused(hip.INVALID_ARGUMENT, lambda: m.search_batched(q[:, :32], 5))
    _refused(hip.INVALID_ARGUMENT, lambda: m.search_batched(q, hip.MUTABLE_MAX_K + 1))
    _refused(hip.UNIMPLEMENTED, lambda: m.rebase(quant))
    assert m.size() == n + 1 and m.search_batched(q, 5)[2].tolist() == [5, 5, 5]
    m.close()


def test_full_delta_and_bad_batches_change_nothing():
    n, dim, measure = 600, 24, hip.SQUARED_L2
    rows, base = bf_base(n, dim, measure, 72)
    q = synth.uniform_f32(4, dim, 73) - np.float32(0.5)
    p = Pair(base, rows, 4)
    new = synth.uniform_f32(8, dim, 74) - np.float32(0.5)
    with pytest.raises(mm.InvalidArgument):
        p.add(new[:, :20])
    with pytest.raises(mm.InvalidArgument):
        p.update(3, new[0, :20])
    ids = p.add(new[:4])
    p.remove(5)
    before = p.mut.search_batched(q, 10)
    for bad in (lambda: p.add(new[4]), lambda: p.add(new[4:6]), lambda: p.update(7, new[4]),
                lambda: p.update([int(ids[0]), 7], new[4:6]), lambda: p.update(5, new[4])):
        with pytest.raises(mm.ResourceExhausted):
            bad()
    # all or nothing: the third element is bad
    with pytest.raises(mm.NotFound):
        p.remove([1, 2, 9999])
    with pytest.raises(mm.NotFound):
        p.update([int(ids[0]), int(ids[1]), 9999], new[:3])
    p.same_counters()
    assert p.mut.pending() == 5 and p.mut.size() == n + 3
    after = p.mut.search_batched(q, 10)
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    check_bf(p, measure, q, 10, "after refusals")
    p.same_rows([1, 2, 5, 7] + ids.tolist())
    p.update(int(ids[2]), new[5])          # in place: needs no slot
    p.remove(ids[0])
    p.add(new[6])                          # the freed slot
    check_bf(p, measure, q, 10, "after reuse of a slot")
    p.close()


# ---- 8. fallback: the base's device entry reports Aborted / ResourceExhausted --------------------------------------
@pytest.fixture(scope="module")
def big_tree():
    from test_gpu_filters import Case
    return Case("txh", 16)


@pytest.mark.parametrize("fam,status", [("sampled", hip.ABORTED), ("unsampled", hip.RESOURCE_EXHAUSTED)])
def test_fallback_to_the_host_entry(big_tree, fam, status):
    c = big_tree
    from test_gpu_filters import K, M
    words, cap = c.family(fam)
    live = H.allowed_ids(words, cap, c.n)
    base = hip.txh_create(**c.kw)
    # the precondition: under this live set the base's enqueue-only search fails as documented
    st = H.device_search(base, c.q, K, c.opts(), allow=H.masked_words(words, cap, c.n), allow_bits=c.n)[0]
    assert st == status
    rows = c.data.reshape(c.n, c.stride)[:, :c.dim]
    p = Pair(base, rows, 64)
    p.remove(np.setdiff1d(np.arange(c.n), live))
    ids = p.add(c.q[:3] + np.float32(1e-3))
    got = p.mut.search_batched(c.q, K, opts=c.opts())
    qs = [0, 1, 2, 17, 63]
    c.oix.partitions_to_search = c.opts().partitions_to_search
    want = p.model.search_txh(c.oix, c.q[qs], K, pre_reorder_k=M)
    check_lists((got[0][qs], got[1][qs], got[2][qs]), want, K, "fallback " + fam)
    assert got[0][0, 0] == ids[0]
    assert np.all(got[2] == K)             # never partial rows
    p.close()


# ---- 9. threads ----------------------------------------------------------------------------------------------------
def test_mutations_beside_searches():
    n, dim, measure, k = 600, 24, hip.SQUARED_L2, 10
    rows, base = bf_base(n, dim, measure, 91)
    q = synth.uniform_f32(8, dim, 92) - np.float32(0.5)
    p = Pair(base, rows, 256)
    new = synth.uniform_f32(200, dim, 93) - np.float32(0.5)
    rng = np.random.default_rng(9)
    errors, done = [], threading.Event()

    def mutate():
        try:
            added = []
            for i in range(200):
                op = i % 4
                if op in (0, 1):
                    added.append(p.add(new[i]))
                elif op == 2:
                    p.remove(int(rng.integers(0, n)) if i % 8 == 2 else added[int(rng.integers(0, len(added)))])
                else:
                    p.update(int(rng.integers(0, n)) if i % 8 == 3 else added[-1], new[i])
        except Exception as e:       # noqa: BLE001
            errors.append(e)
        finally:
            done.set()

    def search():
        try:
            while True:
                last = done.is_set()
                idx, dist, cnt = p.mut.search_batched(q, k)
                assert np.all(cnt == k) and np.all(idx != EMPTY) and np.all(np.diff(dist, axis=1) >= 0)
                if last:
                    return
        except Exception as e:       # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=mutate)] + [threading.Thread(target=search) for _ in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert p.mut.pending() == 200
    er, ei = p.mut.export_live()
    wr, wi = p.model.export_live()
    assert np.array_equal(ei, wi) and np.array_equal(_bits(er), _bits(wr))
    check_bf(p, measure, q, k, "after the threads")
    p.close()

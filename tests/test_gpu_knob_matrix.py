"""The per-call knobs of the tree / flat-hasher search in pairs, on ONE handle, against the oracle.

csrc/knobs.h says of the SCANN_HIP_* switches read on every call: "None of them changes a result."  The rows of
tests/knob_matrix.py hold every pair of levels of the batch size, pre_reorder_k, the entry point / filter and the
seventeen knobs plan_txh_search reads.  Per index variant (flat hasher and tree, int8 and FP8 re-rank stores) every row
runs on one long-lived handle, in an order that starts at the smallest shapes (the workspace arena is rebuilt mid-
sequence, error and empty calls woven in), then on a second handle in a shuffled order that starts with the largest.

Every row: the kernel scann_hip_index_last_kernel_ms names is the one the mirror (knob_matrix.expected_kernel) derives;
counts and distance bits equal those of a default-knob call on a fresh handle, indices up to ties; the oracle's rows
for eight fixed queries; unused slots empty; the device entry Ok; pass 2 bit-identical to pass 1.  No tolerance.
On the flat hasher the form of the sparse prefilter's 64-pair items is read from the handle's workspace after every
row: it holds survivor bitmaps sized by the largest bitmap-form row so far (the mirror's sp_bitmap), and none on a
fresh handle that runs the same rows under SCANN_HIP_SP_BITMAP=0.

Indexes from explicit random 4-bit codes (no training), S = 16, dim 32, 131 072 rows: the smallest at which the sample
has more than 4096 points (the tail bound), the candidate list is longer than 4096 keys at m = 2000 (the select reads
it in place) and shorter at m = 600 (the select runs in LDS), the small pipeline is eligible at m = 600 and the wide
one is the default up to 4 queries: tests/test_knob_matrix.py asserts these on the plan mirror."""
import numpy as np
import pytest

import helpers as H
import knob_matrix as KM
from oracle import pyoracle as orc
from scann_rust_amd import hip, synth

pytestmark = pytest.mark.gpu

N, DIM, S, K = 131072, 32, KM.S, KM.K
TREE_L, TREE_P, TREE_CLUSTERS, TREE_SEED = 8, KM.TREE_P, 4, 2
NQ = KM.NQ_MAX
ORACLE_QUERIES = (0, 3, 15, 16, 39, 100, 200, 229)
MS = (600, 2000)
FILTERS = (None, "shared", "perq")
ENTRY_FILTER = {"host": None, "stages": None, "shared": "shared", "perq": "perq", "device": None,
                "device-shared": "shared"}
CREATION_KNOBS = ("SCANN_HIP_RERANK_I8", "SCANN_HIP_RERANK_STORE", "SCANN_HIP_RERANK_UNIFORM", "SCANN_HIP_SMFMAC")
VARIANTS = {
    "flat-int8-one-scale": ("ah", {"SCANN_HIP_RERANK_I8": "2", "SCANN_HIP_RERANK_UNIFORM": "2"}),
    "flat-int8-per-row": ("ah", {"SCANN_HIP_RERANK_I8": "2", "SCANN_HIP_RERANK_UNIFORM": "0"}),
    "flat-fp8": ("ah", {"SCANN_HIP_RERANK_I8": "2", "SCANN_HIP_RERANK_STORE": "fp8"}),
    "tree-int8-per-row": ("txh", {"SCANN_HIP_RERANK_I8": "2", "SCANN_HIP_RERANK_UNIFORM": "0"}),
    "tree-fp8": ("txh", {"SCANN_HIP_RERANK_I8": "2", "SCANN_HIP_RERANK_STORE": "fp8"}),
}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def tree_rows():
    """clustered rows whose 8 leaves (centres picked among the rows) are uneven: the three largest hold most of them"""
    return synth.clustered_f32(N, DIM, 2100 + TREE_SEED, n_clusters=TREE_CLUSTERS)[0]


class Kind:
    """one index kind: rows, explicit codes, queries, the two filters and the oracle's rows of ORACLE_QUERIES.
    shapes_only: stop at the leaf sizes and the stream (tests/test_knob_matrix.py reads no more)"""

    def __init__(self, kind, shapes_only=False):
        self.kind = kind
        rng = np.random.default_rng([31, kind == "txh"])
        rows = synth.uniform_f32(N, DIM, 2000) if kind == "ah" else tree_rows()
        # queries: rows of the index plus a little noise (sigma 0.03 per dimension)
        self.q = np.ascontiguousarray(rows[rng.choice(N, NQ, replace=False)] +
                                      np.float32(0.03) * rng.standard_normal((NQ, DIM)).astype(np.float32), np.float32)
        self.cb = np.ascontiguousarray(rows[rng.choice(N, 16, replace=False)].reshape(16, S, DIM // S)
                                       .transpose(1, 0, 2), np.float32)
        codes = rng.integers(0, 16, (N, S), dtype=np.uint8)
        if kind == "ah":
            self.kw = H.ah_kwargs_from_codes(rows, self.cb, codes)
            self.oix = None
            self.codes = self.kw["codes"]
            self.leaf_off, self.leaf_ids, self.P = np.array([0, N], np.int64), None, 1
        else:
            self.oix, self.kw = H.txh_from_codes(rows, self.cb, codes, TREE_L, TREE_P, MS[0] / K, seed=TREE_SEED)
            self.leaf_off, self.leaf_ids, self.P = self.kw["leaf_offsets"], self.kw["leaf_ids"], TREE_P
            assert not np.array_equal(self.leaf_ids, np.arange(N)), "leaf_ids must be a real permutation"
        self.data, self.stride = self.kw["data"], self.kw["stride"]
        self.leaves = np.diff(np.asarray(self.leaf_off, np.int64)).tolist()
        self.stream = H.max_stream(self.leaf_off, self.P)
        if shapes_only:
            return
        tok = np.zeros((1, 1), np.int64)   # (the f families read no tokens)
        st = H.sample_plan(self.stream, self.P)[0]
        fam = lambda seed: H.allow_family("f3", self.leaf_off, self.leaf_ids, tok, K, MS[0], st, seed)[0]
        self.shared = fam(1)
        self.perq = np.stack([fam(100 + i) for i in range(NQ)])
        self.oracle = {(m, f, i): self._oracle(m, f, i) for m in MS for f in FILTERS for i in ORACLE_QUERIES}
        self.staged = {(m, i): self._staged_oracle(m, i) for m in MS for i in ORACLE_QUERIES}

    def words(self, filt, i):
        return None if filt is None else self.shared if filt == "shared" else self.perq[i]

    def allow(self, filt, nq):
        return None if filt is None else self.shared if filt == "shared" else self.perq[:nq]

    def opts(self, m):
        o = hip.default_opts()
        o.pre_reorder_k = m
        if self.kind == "txh":
            o.partitions_to_search = TREE_P
        return o

    def _oracle(self, m, filt, i):
        """(idx, dist) of query i at pre_reorder_k = m under the filter: the tree oracle with the bitmap, the flat
        oracle on the allowed subset"""
        words = self.words(filt, i)
        if self.kind == "txh":
            self.oix.pre_reorder_multiplier = m / K
            self.oix.allow = None if words is None else H.masked_words(words, N, N)
            try:
                return orc.txh_search(self.oix, self.q[i], K)
            finally:
                self.oix.allow = None
        if words is None:
            return orc.ah_search_with_reordering(self.cb, self.codes, self.data, self.stride, self.q[i], K, m)
        allowed = H.allowed_ids(words, N, N)
        oi, od = orc.ah_search_with_reordering(self.cb, np.ascontiguousarray(self.codes[allowed]),
                                               np.ascontiguousarray(self.data.reshape(N, self.stride)[allowed]),
                                               self.stride, self.q[i], K, m)
        return allowed[oi].astype(np.uint32), od

    def _staged_oracle(self, m, i):
        """the `oracle` argument of H.check_txh_query / H.check_ah_query for the unfiltered query i"""
        if self.kind == "txh":
            self.oix.pre_reorder_multiplier = m / K
            return orc.txh_search(self.oix, self.q[i], K, stages=True)
        return orc.ah_search(self.cb, self.codes, self.q[i], m) + self.oracle[m, None, i]

    def check_stages(self, m, i, got, what):
        """the stage-aware oracle check of query i of an unfiltered call with stage outputs"""
        idx, dist, cnt, (tok, tokd, ci, cd, cc) = got
        if self.kind == "txh":
            self.oix.pre_reorder_multiplier = m / K
            H.check_txh_query(self.oix, self.q[i], K, idx[i, :cnt[i]], dist[i, :cnt[i]], tok[i], tokd[i],
                              ci[i, :cc[i]], cd[i, :cc[i]], what=what, oracle=self.staged[m, i])
        else:
            H.check_ah_query(self.cb, self.codes, self.data, self.stride, DIM, self.q[i], K, m, idx[i, :cnt[i]],
                             dist[i, :cnt[i]], ci[i, :cc[i]], cd[i, :cc[i]], what=what, oracle=self.staged[m, i])


@pytest.fixture(scope="module")
def kinds():
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = Kind(kind)
        return cache[kind]

    yield get
    cache.clear()


def _clear_knobs(monkeypatch):
    H.scan_env(monkeypatch, "default")
    for name in KM.KNOBS + CREATION_KNOBS:
        monkeypatch.delenv(name, raising=False)


def _create(kd, creation, monkeypatch):
    """a handle with the variant's creation-time knobs, which are removed again"""
    _clear_knobs(monkeypatch)
    for name, v in creation.items():
        monkeypatch.setenv(name, v)
    index = hip.txh_create(**kd.kw)
    for name in creation:
        monkeypatch.delenv(name)
    index.enable_timing(True)
    return index


def _call(index, kd, row):
    """(status, idx, dist, count, stage outputs or None) of the row's call, the environment already set"""
    nq, m, entry = row["nq"], row["m"], row["entry"]
    q, o = kd.q[:nq], kd.opts(m)
    allow = kd.allow(ENTRY_FILTER[entry], nq)
    if entry.startswith("device"):
        return H.device_search(index, q, K, o, allow=allow, allow_bits=None if allow is None else N) + (None,)
    if entry == "stages":
        idx, dist, cnt, extra = index.search_batched(q, K, o, stages=True)
        return hip.OK, idx, dist, cnt, extra
    idx, dist, cnt = index.search_batched(q, K, o, allow=allow, allow_bits=None if allow is None else N)
    return hip.OK, idx, dist, cnt, None


def _same_rows(got, ref, what):
    """counts and distance bits equal, indices up to ties, unused slots empty"""
    idx, dist, cnt = got
    assert np.array_equal(cnt, ref[2]), what + ": counts"
    assert np.array_equal(_bits(dist), _bits(ref[1])), what + ": distances"
    for i in range(idx.shape[0]):
        c = int(cnt[i])
        assert np.all(idx[i, c:] == 0xFFFFFFFF) and np.all(np.isposinf(dist[i, c:])), "%s q%d: unused slots" % (what, i)
        H.assert_topk_equal_up_to_ties(idx[i, :c], dist[i, :c], ref[0][i, :c], ref[1][i, :c], what="%s q%d" % (what, i))


def _defaults(kd, creation, monkeypatch):
    """{(m, filter): rows of all 230 queries} of a fresh handle with every per-call knob unset.  Per nq level that
    handle also makes one host and one device call: the prefix of the 230 rows, the device entry Ok."""
    index = _create(kd, creation, monkeypatch)
    ref = {}
    for m in MS:
        for filt in FILTERS:
            o = kd.opts(m)
            ref[m, filt] = index.search_batched(kd.q, K, o, allow=kd.allow(filt, NQ), allow_bits=None if filt is None else N)
            for nq in KM.FACTORS[0][1]:
                what = "default m%d %s nq%d" % (m, filt, nq)
                allow = kd.allow(filt, nq)
                sub = tuple(x[:nq] for x in ref[m, filt])
                _same_rows(index.search_batched(kd.q[:nq], K, o, allow=allow, allow_bits=None if filt is None else N), sub,
                           what + " host")
                if filt != "perq":
                    status, di, dd, dc = H.device_search(index, kd.q[:nq], K, o, allow=allow,
                                                         allow_bits=None if filt is None else N)
                    assert status == hip.OK, "%s device: status %d" % (what, status)
                    _same_rows((di, dd, dc), sub, what + " device")
            for i in ORACLE_QUERIES:
                oi, od = kd.oracle[m, filt, i]
                idx, dist, cnt = ref[m, filt]
                assert cnt[i] == oi.size, "default m%d %s q%d: count" % (m, filt, i)
                H.assert_topk_equal_up_to_ties(idx[i, :cnt[i]], dist[i, :cnt[i]], oi, od,
                                               what="default m%d %s q%d against the oracle" % (m, filt, i))
    index.close()
    return ref


def _disturb(index, kd, d):
    """one call of knob_matrix.DISTURBANCES, checked by its status (and count)"""
    o = kd.opts(d["m"])
    if d["partitions_to_search"] is not None:
        o.partitions_to_search = d["partitions_to_search"]
    try:
        idx, dist, cnt = index.search_batched(kd.q[:d["nq"]], d["k"], o,
                                              q_dim=None if d["q_dim"] is None else DIM + d["q_dim"])
        status = hip.OK
    except hip.ScannError as e:
        status, cnt = e.code, None
    assert status == getattr(hip, d["status"]), "%s: status %d" % (d["name"], status)
    if d["count"] is not None:
        # (k = 0: fill_empty's rows have no columns to hold 0xFFFFFFFF / +inf -- the counts and the shape are all there is)
        assert idx.shape == dist.shape == (d["nq"], d["k"]) and cnt.shape == (d["nq"],), d["name"]
        assert np.all(cnt == d["count"]), "%s: counts %s" % (d["name"], cnt)


def _stream():
    import torch
    return torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream


def _bitmap_bytes(index):
    """bytes of survivor bitmaps in the workspace the rows run on.  The device entry's calls are enqueued on torch's
    current stream, whose workspace is the primary one the host entry uses (the first device slot): the two reads are
    of one workspace, and both are made so that a second one would show."""
    host, dev = index.debug_survivor_bitmap_bytes(), index.debug_survivor_bitmap_bytes(_stream())
    assert host == dev, "the host and the device entry ran on two workspaces: %d / %d bytes" % (host, dev)
    return host


def _run_row(index, kd, row, ref, monkeypatch, seen=None):
    """the row's call on `index` under its knobs, with every check that needs no other pass; returns its outputs.
    seen: {"bytes": the largest survivor bitmaps a bitmap-form row of this handle has asked for so far} -- updated by
    the mirror's plan and compared with the handle's"""
    what = KM.row_id(row)
    for name in KM.KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, v in KM.row_env(row).items():
        monkeypatch.setenv(name, v)
    status, idx, dist, cnt, extra = _call(index, kd, row)
    kernel = index.last_kernel_ms()[1]
    for name in KM.KNOBS:
        monkeypatch.delenv(name, raising=False)
    want = KM.expected_kernel(row, kd.kind, kd.stream, kd.leaves)
    assert kernel == want, "%s: ran %s, the plan mirror says %s" % (what, kernel, want)
    assert status == hip.OK, "%s: status %d" % (what, status)
    if seen is not None:
        plan = KM.expected_plan(row, kd.kind, kd.stream, kd.leaves)
        assert plan["sp_bitmap"] == (kd.kind == "ah" and plan["sp_pairs64"] and row["SCANN_HIP_SP_BITMAP"] is None), what
        seen["bytes"] = max(seen["bytes"], plan["sp_bitmap_bytes"])
        assert _bitmap_bytes(index) == seen["bytes"], "%s: %d bytes of survivor bitmaps, the plan mirror says %d" % (
            what, _bitmap_bytes(index), seen["bytes"])
    nq, m, filt = row["nq"], row["m"], ENTRY_FILTER[row["entry"]]
    _same_rows((idx, dist, cnt), tuple(x[:nq] for x in ref[m, filt]), what)
    for i in ORACLE_QUERIES:
        if i >= nq:
            continue
        if extra is not None:
            kd.check_stages(m, i, (idx, dist, cnt, extra), "%s q%d" % (what, i))
        oi, od = kd.oracle[m, filt, i]
        assert cnt[i] == oi.size, "%s q%d: count %d, the oracle's %d" % (what, i, cnt[i], oi.size)
        H.assert_topk_equal_up_to_ties(idx[i, :cnt[i]], dist[i, :cnt[i]], oi, od, what="%s q%d against the oracle" % (what, i))
    out = [idx.copy(), dist.copy(), cnt.copy()]
    if extra is not None:
        tok, tokd, ci, cd, cc = extra
        P = kd.P
        valid = np.arange(ci.shape[1])[None, :] < cc[:, None]
        out += [tok[:, :P].copy(), tokd[:, :P].copy(), np.where(valid, ci, 0), np.where(valid, cd, 0), cc.copy()]
    return out


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_knob_matrix(kinds, variant, monkeypatch):
    kind, creation = VARIANTS[variant]
    kd = kinds(kind)
    rows = KM.matrix_rows()
    ref = _defaults(kd, creation, monkeypatch)

    # pass 1: from the smallest shapes up, a disturbance after every eighth row
    order = KM.pass1_order(rows)
    # (scann_hip_index_device_bytes leaves the search workspaces out, by its contract, and nothing else reports the
    # arena: its rebuilds are DERIVED from the sequence, not observed -- a call with more queries than any before it
    # asks ensure_txh_workspace for longer per-query buffers, and TxhWorkspace::commit rebuilds the arena for it.  This
    # assertion holds the row order to that; none here would fail if the library never rebuilt the arena)
    assert KM.growth_steps(rows, order) >= 2
    index = _create(kd, creation, monkeypatch)
    held = index.device_bytes()
    first = {}
    seen = {"bytes": 0}
    assert _bitmap_bytes(index) == 0
    for n_done, r in enumerate(order, 1):
        first[r] = _run_row(index, kd, rows[r], ref, monkeypatch, seen)
        if n_done % 8 == 0:
            _disturb(index, kd, KM.DISTURBANCES[(n_done // 8 - 1) % len(KM.DISTURBANCES)])
    assert len(first) == len(rows)
    assert (seen["bytes"] > 0) == (kind == "ah"), "the bitmap form ran on the flat hasher, and only there"
    assert index.device_bytes() == held, "the handle's persistent allocations changed during the searches"
    index.close()

    # pass 2: a new handle, the largest row first, then a seeded shuffle
    order = KM.pass2_order(rows)
    assert KM.growth_steps(rows, order) == 0
    index = _create(kd, creation, monkeypatch)
    seen = {"bytes": 0}
    for r in order:
        again = _run_row(index, kd, rows[r], ref, monkeypatch, seen)
        for a, b in zip(again, first[r]):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), \
                "%s: pass 2 differs from pass 1" % KM.row_id(rows[r])
    index.close()

    # the list form on a fresh handle: every row that runs 64-pair items, under SCANN_HIP_SP_BITMAP=0 -- the same kernel
    # name, the rows of the default-knob handle and of the oracle, and no survivor bitmaps in the workspace
    if kind == "ah":
        index = _create(kd, creation, monkeypatch)
        seen = {"bytes": 0}
        pairs64 = [r for r in range(len(rows)) if KM.expected_plan(rows[r], kind, kd.stream, kd.leaves)["sp_pairs64"]]
        assert len(pairs64) >= 2
        for r in pairs64:
            _run_row(index, kd, dict(rows[r], SCANN_HIP_SP_BITMAP="0"), ref, monkeypatch, seen)
        assert seen["bytes"] == 0 and _bitmap_bytes(index) == 0
        index.close()

"""scann_hip_fold_mutable on the device (include/scann_hip.h "fold") against tests/fold_model.py: the arrays of the new
base, read back through scann_hip_index_write_file and scann_rust_amd/index_file.py, must equal the model's exactly
(rows and codes bitwise; offsets, ids and base_ids equal), and searches of the new base must match the CPU oracle run on
the model's arrays, stage outputs included.

The tree has L = 7 hand-placed centres over dim 32: leaf 0 is longer than 2 * FOLD_CHUNK + 1 positions, leaf 3 is
small and is emptied by the script, leaf 5 starts empty and receives delta rows, centre 6 is a copy of centre 2 (a row
equidistant to both must go to leaf 2).  The script adds rows (high ids), updates low ids in between (delta rows that
must merge into the middle of leaves) and removes ids across 64-bit bitmap word boundaries: a delta of about 1500."""
import numpy as np
import pytest

import fold_model as fm
import helpers as H
from oracle import pyoracle as orc
from scann_rust_amd import hip, index_file, synth
from test_gpu_mutable import Pair

pytestmark = pytest.mark.gpu

DIM, L, K_TOP = 32, 7, 10
COUNTS = (2100, 400, 300, 40, 160, 0, 0)      # rows generated around each centre; n = 3000
assert COUNTS[0] > 2 * hip.FOLD_CHUNK + 1 and sum(COUNTS) == 3000


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def centres():
    c = synth.uniform_f32(L, DIM, 7) * np.float32(4.0)
    c[6] = c[2]
    return np.ascontiguousarray(c)


def near(centre_ids, seed):
    """one row per entry of centre_ids: that centre plus noise in [0, 0.3)"""
    centre_ids = np.asarray(centre_ids)
    return np.ascontiguousarray(centres()[centre_ids] + synth.uniform_f32(centre_ids.size, DIM, seed) * np.float32(0.3))


_cache = {}


def tree_case(S, K, use_residuals):
    """(rows, index dict of fold_model with partitions_to_search / multiplier): codes by the oracle's encoder"""
    key = (S, K, use_residuals)
    if key not in _cache:
        owner = np.repeat(np.arange(L), COUNTS)
        owner = owner[np.random.default_rng(1).permutation(owner.size)]
        rows = near(owner, 11)
        rng = np.random.default_rng(S * 1000 + K)
        codebook = rng.random((S, K, DIM // S), dtype=np.float32) * np.float32(0.3 if use_residuals else 4.3)
        ix = dict(kind="txh", centers=centres(), codebook=codebook, use_residuals=use_residuals, P=3, mult=5.0)
        off, lid, codes = fm.frozen_build(ix, rows)
        assert np.diff(off).tolist() == list(COUNTS) and not np.array_equal(lid, np.arange(lid.size))
        ix.update(leaf_off=off, leaf_ids=lid, codes=codes)
        _cache[key] = (rows, ix)
    rows, ix = _cache[key]
    return rows, dict(ix)


def create(ix, rows):
    data, stride = orc.to_strided(rows)
    n = rows.shape[0]
    if ix["kind"] == "bf":
        return hip.bf_create(data, n, DIM, stride, ix["measure"])
    if ix["kind"] == "ah":
        return hip.txh_create(**H.ah_kwargs_from_codes(rows, ix["codebook"], ix["codes"]))
    return hip.txh_create(data=data, n_rows=n, dim=DIM, stride=stride, centers=ix["centers"], leaf_offsets=ix["leaf_off"],
                          leaf_ids=ix["leaf_ids"], codebook=ix["codebook"], codes=ix["codes"], codes_packed4=False,
                          use_residuals=ix["use_residuals"], partitions_to_search=ix["P"], pre_reorder_multiplier=ix["mult"])


def script(p, seed, empty_leaf=None):
    """adds (high ids), updates of low ids in between, removes over word boundaries and of one whole leaf"""
    n = p.model.base_ids.size
    base_ids = p.model.base_ids.copy()
    targets = np.array([0, 1, 2, 4, 5])                      # never leaf 3 (emptied); 2 is also equidistant to 6
    pick = lambda count, s: targets[np.random.default_rng(s).integers(0, targets.size, count)]
    p.add(near(pick(350, seed), seed + 1))
    low = base_ids[np.arange(800) * 3 + 1]                   # low ids, every third
    p.update(low[:400], near(pick(400, seed + 2), seed + 3))
    p.add(near(pick(350, seed + 4), seed + 5))
    p.update(low[400:], near(pick(400, seed + 6), seed + 7))
    rm = np.concatenate([base_ids[60:70], base_ids[124:131], base_ids[n - 70:n - 58]])   # words 0|1, 1|2, and late ones
    if empty_leaf is not None:
        rm = np.union1d(rm, base_ids[empty_leaf])
    p.remove(rm)
    assert 1400 <= len(p.model.delta_ids) <= 1600


def file_arrays(index, tmp_path, name="folded.scannidx"):
    path = str(tmp_path / name)
    hip.index_write_file(index, path)
    return index_file.arrays(path), path


def same_arrays(arr, base_ids, f):
    """the written file of the new base against the model's fold `f`"""
    n = f["base_ids"].size
    assert np.array_equal(base_ids, f["base_ids"])
    assert arr["n_rows"] == n and arr["n_local"] == n and arr["dim"] == DIM and arr["stride"] == hip.compute_stride(DIM)
    assert np.array_equal(_bits(arr["data"][:, :DIM]), _bits(f["rows"])), "rows are not bit-copies"
    assert not np.asarray(arr["data"][:, DIM:]).view(np.uint32).any(), "padding is not zero"
    if f["kind"] == "bf":
        assert arr["kind"] == 0 and arr["distance_measure"] == f["measure"]
        return
    S, Kc = f["codebook"].shape[:2]
    assert arr["kind"] == 1 and arr["num_subspaces"] == S and arr["num_codes"] == Kc
    assert np.array_equal(_bits(arr["codebook"]), _bits(f["codebook"]))
    codes = np.asarray(arr["codes"])
    assert bool(arr["codes_packed4"]) == (Kc <= 16)
    if arr["codes_packed4"]:
        codes = orc.unpack4(np.ascontiguousarray(codes), S)
    assert np.array_equal(codes, f["codes"]), "codes differ"
    if f["kind"] == "ah":
        assert arr["num_partitions"] == 0
        return
    assert arr["num_partitions"] == L and bool(arr["use_residuals"]) == f["use_residuals"]
    assert arr["partitions_to_search"] == f["P"] and arr["pre_reorder_multiplier"] == np.float32(f["mult"])
    assert np.array_equal(_bits(arr["centers"]), _bits(f["centers"]))
    assert np.array_equal(arr["leaf_offsets"], f["leaf_off"]), (arr["leaf_offsets"], f["leaf_off"])
    assert np.array_equal(arr["leaf_ids"], f["leaf_ids"]), "leaf_ids differ"


def queries(seed, nq=8):
    return near(np.arange(nq) % 6, seed)


def oracle_index(f):
    data, stride = orc.to_strided(f["rows"])
    return orc.TxhIndex(data, stride, DIM, f["centers"], f["leaf_off"], f["leaf_ids"], f["codebook"], f["codes"],
                        use_residuals=f["use_residuals"], partitions_to_search=f["P"], pre_reorder_multiplier=f["mult"])


def same_searches(index, f, q, k=K_TOP, opts=None, exact_candidates=False, what=""):
    """searches of the new base against the oracle on the model's arrays, stage outputs included"""
    n = f["base_ids"].size
    data, stride = orc.to_strided(f["rows"])
    if f["kind"] == "bf":
        idx, dist, cnt = index.search_batched(q, k)
        for i in range(q.shape[0]):
            oi, od = orc.bf_search(data, n, DIM, stride, f["measure"], q[i], k)
            assert cnt[i] == oi.size
            H.assert_topk_equal_up_to_ties(idx[i, :cnt[i]], dist[i, :cnt[i]], oi, od, what="%s bf q%d" % (what, i))
        return
    o = opts if opts is not None else hip.default_opts()
    if f["kind"] == "ah" and not o.pre_reorder_k:
        o.pre_reorder_k = 40
    if f["kind"] == "txh":      # the index's own defaults, spelled out: the stage outputs are pitched by them
        o.partitions_to_search = o.partitions_to_search or f["P"]
        o.pre_reorder_k = o.pre_reorder_k or orc.pre_reorder_k(k, f["mult"])
    idx, dist, cnt, (tok, tokd, ci, cd, cc) = index.search_batched(q, k, o, stages=True)
    if f["kind"] == "ah":
        for i in range(q.shape[0]):
            H.check_ah_query(f["codebook"], f["codes"], data, stride, DIM, q[i], k, o.pre_reorder_k, idx[i, :cnt[i]],
                             dist[i, :cnt[i]], ci[i, :cc[i]], cd[i, :cc[i]], what="%s ah q%d" % (what, i))
        return
    oix = oracle_index(f)
    if o.partitions_to_search:
        oix.partitions_to_search = o.partitions_to_search
    if o.pre_reorder_k:
        oix.pre_reorder_multiplier = float(o.pre_reorder_k) / float(k)
        assert orc.pre_reorder_k(k, oix.pre_reorder_multiplier) == o.pre_reorder_k
    assert (tok.shape[1], ci.shape[1]) == (o.partitions_to_search, o.pre_reorder_k)   # the pitch of the stage outputs
    for i in range(q.shape[0]):
        H.check_txh_query(oix, q[i], k, idx[i, :cnt[i]], dist[i, :cnt[i]], tok[i], tokd[i], ci[i, :cc[i]], cd[i, :cc[i]],
                          what="%s txh q%d" % (what, i))
        if exact_candidates:
            oci = np.asarray(orc.txh_search(oix, q[i], k, stages=True)[4])
            # the oracle's list, position for position, except inside a run of bit-equal approximate distances.
            # (Which rows of such a run the list keeps depends on the order inside the leaf and is checked: the members
            # of every run must be the oracle's.  The order in which a run is LISTED is the oracle's final sort by
            # distance alone, which the device does not reproduce: it lists ties by index.  Measured on this case:
            # device [38 1368], oracle [1368 38], equal distances.)
            got, gd = ci[i, :cc[i]], _bits(cd[i, :cc[i]])
            assert got.size == oci.size, "%s q%d: %d candidates, want %d" % (what, i, got.size, oci.size)
            s = 0
            while s < got.size:
                e = s + 1
                while e < got.size and gd[e] == gd[s]:
                    e += 1
                assert sorted(got[s:e].tolist()) == sorted(oci[s:e].tolist()), \
                    "%s q%d candidates [%d, %d)\n got %s\nwant %s" % (what, i, s, e, got, oci)
                s = e


def fold_and_compare(p, ix, tmp_path, q, what, **kw):
    """fold the handle and the model; arrays, handle state and searches.  Returns (new base, fold of the model)."""
    f = fm.fold(p.model, ix)
    ids_before = [i for i in range(p.model.next_index) if p.model.exists(i)][::37]
    rows_before = [p.model.get(i) for i in ids_before]
    nxt = p.model.next_index
    new_base, base_ids = p.mut.fold()
    arr, _ = file_arrays(new_base, tmp_path)
    same_arrays(arr, base_ids, f)
    fm.apply(p.model, f)
    p.same_counters()
    assert p.mut.pending() == 0 and p.model.next_index == nxt and new_base.size() == base_ids.size
    for i, r in zip(ids_before, rows_before):
        assert np.array_equal(_bits(p.mut.get(i)), _bits(r)), i
    same_searches(new_base, f, q, what=what, **kw)
    return new_base, f


# ---- 1. the script on every kind of base ---------------------------------------------------------------------------
@pytest.mark.parametrize("S,K,use_residuals", [(8, 16, True), (8, 16, False), (4, 256, True)])
def test_tree_script(S, K, use_residuals, tmp_path):
    rows, ix = tree_case(S, K, use_residuals)
    base = create(ix, rows)
    p = Pair(base, rows, 2048)
    leaf3 = ix["leaf_ids"][ix["leaf_off"][3]:ix["leaf_off"][4]]
    script(p, 100 + S, empty_leaf=leaf3)
    delta_ids = np.asarray(p.model.delta_ids)
    new_base, f = fold_and_compare(p, ix, tmp_path, queries(21), "tree S%d K%d" % (S, K))
    sizes = np.diff(f["leaf_off"])
    assert sizes[3] == 0 and sizes[5] > 0 and sizes[6] == 0      # emptied, filled, shadowed by its twin centre
    # delta rows were merged into the middle of leaves, not appended: in some leaf a base row follows a delta row
    from_delta = np.isin(f["base_ids"][f["leaf_ids"]], delta_ids).astype(int)
    assert any(np.any(np.diff(from_delta[a:b]) < 0) for a, b in zip(f["leaf_off"][:-1], f["leaf_off"][1:]))
    assert np.any(fm.assign_encode(ix, near([2, 2, 2], 5))[0] == 2)    # equidistant to centres 2 and 6: the lower one
    p.close()


def test_flat_hasher_script(tmp_path):
    n, S = 5000, 8
    assert n > 4 * hip.FOLD_CHUNK
    rows = near(np.arange(n) % 5, 31)
    codebook = np.random.default_rng(32).random((S, 16, DIM // S), dtype=np.float32) * np.float32(4.3)
    ix = dict(kind="ah", codebook=codebook, codes=orc.encode_many(codebook, rows))
    p = Pair(create(ix, rows), rows, 2048)
    script(p, 130)
    fold_and_compare(p, ix, tmp_path, queries(33), "flat hasher")
    p.close()


@pytest.mark.parametrize("measure", [hip.DOT_PRODUCT, hip.SQUARED_L2])
def test_brute_force_script(measure, tmp_path):
    rows = near(np.arange(3000) % 5, 41)
    ix = dict(kind="bf", measure=measure)
    p = Pair(create(ix, rows), rows, 2048)
    script(p, 140)
    fold_and_compare(p, ix, tmp_path, queries(43), "bf %d" % measure)
    p.close()


# ---- 2. order inside a leaf decides: duplicates --------------------------------------------------------------------
def test_duplicates_keep_the_oracle_order(tmp_path):
    rows, ix = tree_case(8, 16, True)
    p = Pair(create(ix, rows), rows, 64)
    leaf1 = ix["leaf_ids"][ix["leaf_off"][1]:ix["leaf_off"][2]]
    r = int(leaf1[len(leaf1) // 2])                           # a live base row in the middle of leaf 1
    low = int(leaf1[3])                                        # a low id of the same leaf becomes a copy of it
    p.update(low, rows[r])
    p.add(np.stack([rows[r], rows[r]]))                        # and two identical delta rows with high ids
    o = hip.default_opts()
    o.partitions_to_search, o.pre_reorder_k = 1, 2             # the boundary of the candidate list falls inside the tie
    q = np.stack([rows[r], rows[int(leaf1[5])]])
    new_base, f = fold_and_compare(p, ix, tmp_path, q, "duplicates", k=2, opts=o, exact_candidates=True)
    members = f["leaf_ids"][f["leaf_off"][1]:f["leaf_off"][2]]
    same = [int(j) for j in members if np.array_equal(_bits(f["rows"][j]), _bits(rows[r]))]
    assert len(same) == 4 and same == sorted(same) and f["base_ids"][same[0]] == low
    # strict '<', first in scan order: of the four equal rows the list of two keeps the first two OF THE LEAF
    stage = new_base.search_batched(q[:1], 2, o, stages=True)[3]
    assert sorted(stage[2][0, :stage[4][0]].tolist()) == same[:2], (stage[2][0], same)
    p.close()


# ---- 3. edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["txh", "ah", "bf"])
def test_nothing_mutated(kind, tmp_path):
    rows, ix = tree_case(8, 16, True)
    if kind == "ah":
        ix = dict(kind="ah", codebook=ix["codebook"], codes=orc.encode_many(ix["codebook"], rows))
    elif kind == "bf":
        ix = dict(kind="bf", measure=hip.SQUARED_L2)
    base = create(ix, rows)
    before, _ = file_arrays(base, tmp_path, "before.scannidx")
    p = Pair(base, rows, 16)
    new_base, f = fold_and_compare(p, ix, tmp_path, queries(51), "nothing mutated " + kind)
    after, _ = file_arrays(new_base, tmp_path, "after.scannidx")
    assert sorted(k for k in before if isinstance(before[k], np.ndarray)) == sorted(k for k in after if isinstance(after[k], np.ndarray))
    for name, a in before.items():
        if name == "file_bytes":
            continue
        assert np.array_equal(np.asarray(a), np.asarray(after[name])), name
    assert p.model.identity
    p.close()


def test_every_base_row_removed_then_no_live_row(tmp_path):
    rows, ix = tree_case(8, 16, True)
    p = Pair(create(ix, rows), rows, 256)
    ids = p.add(near(np.arange(150) % 6, 61))
    p.remove(np.arange(3000))
    assert p.mut.size() == 150
    q = queries(62)
    new_base, f = fold_and_compare(p, ix, tmp_path, q, "delta alone")
    assert np.array_equal(f["base_ids"], ids) and not p.model.identity
    # no live row left: refused, and the handle answers as before the call
    p.remove(ids)
    before = p.mut.search_batched(q, K_TOP)
    with pytest.raises(hip.ScannError) as e:
        p.mut.fold()
    assert e.value.code == hip.INVALID_ARGUMENT and "empty dataset" in str(e.value)
    p.same_counters()
    for a, b in zip(before, p.mut.search_batched(q, K_TOP)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    nid = p.add(rows[5])                                       # the id sequence goes on
    assert nid == 3150 and p.mut.search_batched(rows[5:6], 1)[0][0, 0] == nid
    p.close()


def test_nan_delta_row_goes_to_centre_zero(tmp_path):
    rows, ix = tree_case(8, 16, True)
    p = Pair(create(ix, rows), rows, 16)
    bad = near([4], 71)
    bad[0, 9] = np.nan
    nid = int(p.add(bad)[0])
    p.add(near([4, 5], 72))
    o = hip.default_opts()
    o.partitions_to_search = 1                                 # queries around centre 1: leaf 0 is not scanned
    new_base, f = fold_and_compare(p, ix, tmp_path, near([1, 1, 1], 73), "nan row", opts=o)
    j = int(np.flatnonzero(f["base_ids"] == nid)[0])
    in_leaf0 = f["leaf_ids"][f["leaf_off"][0]:f["leaf_off"][1]]
    assert j in in_leaf0.tolist() and in_leaf0[-1] == j        # centre 0, the highest index of the leaf
    p.close()


# ---- 4. life after a fold ------------------------------------------------------------------------------------------
def test_life_after_a_fold(tmp_path):
    rows, ix = tree_case(8, 16, True)
    p = Pair(create(ix, rows), rows, 2048)
    script(p, 200)
    q = queries(81)
    new_base, f = fold_and_compare(p, ix, tmp_path, q, "first fold")
    assert not p.model.identity                                 # rows were removed: base_ids is a real list
    oix = oracle_index(f)

    def check(what, **kw):
        from test_gpu_mutable import check_lists
        got = p.mut.search_batched(q, K_TOP, **kw)
        check_lists(got, p.model.search_txh(oix, q, K_TOP, **kw), K_TOP, what)
        return got

    got = check("through the handle")                           # external ids
    assert np.all(np.isin(got[0][got[0] != 0xFFFFFFFF], f["base_ids"]))
    nxt = p.model.next_index
    ids = p.add(near([0, 1, 5], 82))
    assert ids.tolist() == [nxt, nxt + 1, nxt + 2]
    live = f["base_ids"]
    p.update(live[[3, 700, 2500]], near([1, 0, 2], 83))
    p.remove(live[1000:1070])
    check("after further mutations")
    cap = p.model.next_index
    words = H.words_of(np.flatnonzero(np.random.default_rng(8).random(cap) < 0.5), cap)[0]
    check("user bitmap over external ids", allow=words, allow_bits=cap - 2)   # the gather form of the bitmap kernel
    # a second fold, from non-identity base_ids
    fold_and_compare(p, f, tmp_path, q, "second fold")
    p.close()


# ---- 5. the finish half ran on the new arrays ----------------------------------------------------------------------
def test_rerank_copy_is_rebuilt(tmp_path, monkeypatch):
    H.scan_env(monkeypatch, "default")
    monkeypatch.setenv("SCANN_HIP_RERANK_I8", "2")
    monkeypatch.setenv("SCANN_HIP_RERANK_I8_MIN", "1")
    rows, ix = tree_case(8, 16, True)
    p = Pair(create(ix, rows), rows, 2048)
    script(p, 300)
    o = hip.default_opts()
    o.partitions_to_search, o.pre_reorder_k = 3, 4 * K_TOP + 24   # pre_reorder_k > 4 k: the filter's domain
    fold_and_compare(p, ix, tmp_path, queries(91, 40), "int8 re-rank rows", opts=o)
    p.close()


@pytest.mark.parametrize("scan", ["dense32", "sp-words"])
def test_scan_operands_are_rebuilt(scan, tmp_path, monkeypatch):
    H.scan_env(monkeypatch, scan)
    rows, ix = tree_case(8, 16, True)
    p = Pair(create(ix, rows), rows, 2048)
    script(p, 310)
    new_base, f = fold_and_compare(p, ix, tmp_path, queries(92, 40), "scan " + scan)
    new_base.enable_timing(True)
    new_base.search_batched(queries(92, 40), K_TOP)
    assert new_base.last_kernel_ms()[1] == H.scan_kernel_name(scan, 8)
    p.close()


# ---- 6. preconditions and capacity ---------------------------------------------------------------------------------
def test_descending_leaf_is_refused(tmp_path):
    rows, ix = tree_case(8, 16, True)
    a, b = int(ix["leaf_off"][1]), int(ix["leaf_off"][2])
    ix["leaf_ids"] = ix["leaf_ids"].copy()
    ix["codes"] = ix["codes"].copy()
    ix["leaf_ids"][a:b] = ix["leaf_ids"][a:b][::-1]
    ix["codes"][a:b] = ix["codes"][a:b][::-1]
    base = create(ix, rows)
    p = Pair(base, rows, 16)
    p.add(near([1, 2], 95))
    q = queries(96)
    before = p.mut.search_batched(q, K_TOP)
    with pytest.raises(hip.ScannError) as e:
        p.mut.fold()
    assert e.value.code == hip.FAILED_PRECONDITION and "ascending" in str(e.value)
    p.same_counters()
    assert p.mut.base is base
    for x, y in zip(before, p.mut.search_batched(q, K_TOP)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    # a short id array: ResourceExhausted with the count reported and nothing changed
    import ctypes as C
    ids, got, h = np.zeros(8, np.uint32), C.c_uint64(0), hip.vp()
    st = hip.load().scann_hip_fold_mutable(p.mut.h, C.byref(h), hip.ptr(ids, hip.u32p), 8, C.byref(got))
    assert st == hip.RESOURCE_EXHAUSTED and got.value == 3002 and not h.value
    p.close()


# ---- 7. write / load -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["txh", "bf"])
def test_written_file_loads_to_the_same_searches(kind, tmp_path):
    rows, ix = tree_case(8, 16, True)
    if kind == "bf":
        ix = dict(kind="bf", measure=hip.DOT_PRODUCT)
    p = Pair(create(ix, rows), rows, 2048)
    script(p, 400)
    new_base, base_ids = p.mut.fold()
    _, path = file_arrays(new_base, tmp_path)
    loaded = hip.load_file(path)
    q = queries(97, 20)
    for a, b in zip(new_base.search_batched(q, K_TOP), loaded.search_batched(q, K_TOP)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    info = hip.index_file_info(path)
    assert info["n_rows"] == base_ids.size and info["has_data"] == 1
    p.close()


@pytest.mark.parametrize("kind", ["partitioned", "rowless"])
def test_other_handles_write_and_load(kind, tmp_path):
    """scann_hip_index_write_file on handles no fold produces: a Partitioned one (no codes) and one created without rows"""
    rows, ix = tree_case(8, 16, True)
    data, stride = orc.to_strided(rows)
    kw = dict(data=data, n_rows=rows.shape[0], dim=DIM, stride=stride, centers=ix["centers"], leaf_offsets=ix["leaf_off"],
              leaf_ids=ix["leaf_ids"], codebook=ix["codebook"], codes=ix["codes"], codes_packed4=False,
              use_residuals=True, partitions_to_search=3, pre_reorder_multiplier=5.0)
    o = hip.default_opts()
    if kind == "partitioned":
        kw.update(codebook=None, codes=None)
    else:
        kw.update(data=None)
        o.exact_reorder = 0
    index = hip.txh_create(**kw)
    arr, path = file_arrays(index, tmp_path, kind + ".scannidx")
    info = hip.index_file_info(path)
    assert info["n_rows"] == rows.shape[0] and info["num_partitions"] == L
    assert info["has_data"] == (1 if kind == "partitioned" else 0)
    assert info["num_subspaces"] == (0 if kind == "partitioned" else 8)
    assert np.array_equal(arr["leaf_offsets"], ix["leaf_off"]) and np.array_equal(arr["leaf_ids"], ix["leaf_ids"])
    assert np.array_equal(_bits(arr["centers"]), _bits(ix["centers"]))
    if kind == "rowless":
        assert np.array_equal(orc.unpack4(np.ascontiguousarray(arr["codes"]), 8), ix["codes"])
    loaded = hip.load_file(path)
    q = queries(98, 20)
    for a, b in zip(index.search_batched(q, K_TOP, o), loaded.search_batched(q, K_TOP, o)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))

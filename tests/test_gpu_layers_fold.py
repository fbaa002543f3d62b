"""scann_hip_fold_mutable into the integer-MFMA prefilters: the operand planes a fold leaves behind, searched.

tests/test_gpu_fold.py checks the planes after a fold on an 8-leaf tree of 3000 rows under dense32 / sp-words.  A folded
FLAT hasher's planes feed the bitmap form (adc_smfmac_bits_kernel64 + adc_refine_bits_kernel): the delta rows' codes
are encoded on the device and the 1024-point ranges are re-cut by the new row count.  Here a flat hasher is folded
twice, so that the new bases have
  n' = 5121   five full ranges and a last range of ONE point
  n' = 5120   whole ranges only
and each new base is compared with tests/fold_model.py (fold_and_compare: index files section by section, then all 65
queries against the oracle over the folded arrays, staged outputs included) under the bitmap form, searched again
under SCANN_HIP_SP_BITMAP=0 (same candidate sets), and searched through the rebased mutable handle after further
mutations.  One tree of 20000 rows (the 7 hand-placed centres of tests/test_gpu_fold.py) is folded under sp-words.

Every search asserts its scan: scann_hip_index_last_kernel_ms on the new base, and for the flat forms the survivor
bitmaps in its workspace (debug_survivor_bitmap_bytes: the call's size under the bitmap form, 0 on a handle that only
ran lists)."""
import numpy as np
import pytest

import fold_model as fm
from oracle import pyoracle as orc
from scann_rust_amd import hip, synth
from test_gpu_fold import DIM, L, create, fold_and_compare, file_arrays, near, queries, same_searches, script
from test_gpu_mutable import Pair, check_lists
from test_gpu_sp_bitmap import _bitmap_bytes, _knob, _same_staged

pytestmark = pytest.mark.gpu

K, M, NQ = 10, 250, 65
NAME = "adc_smfmac_kernel"
FLAT_N, FLAT_S = 4133, 16
TREE_COUNTS = (14000, 2700, 2000, 250, 1050, 0, 0)
assert sum(TREE_COUNTS) == 20000 and len(TREE_COUNTS) == L


def _opts():
    o = hip.default_opts()
    o.pre_reorder_k = M
    return o


def spread(count, seed):
    """rows spread over the flat codebook's range: their code vectors are all different, so that approximate distances
    do not tie at the candidate cut (the rows of tests/test_gpu_fold.py sit around five centres and share a handful of
    code vectors: final rows then depend on which members of a tie the candidate list keeps, which only a staged
    comparison can follow -- a search through the mutable handle has no stage outputs)"""
    return np.ascontiguousarray(synth.uniform_f32(count, DIM, seed) * np.float32(4.3))


def flat_case():
    rows = spread(FLAT_N, 531)
    codebook = np.random.default_rng(532).random((FLAT_S, 16, DIM // FLAT_S), dtype=np.float32) * np.float32(4.3)
    return rows, dict(kind="ah", codebook=codebook, codes=orc.encode_many(codebook, rows))


def flat_round(p, round_no):
    """round 1: 4133 rows -> 5121 (12 removed over the word edge 63 | 64 and the range edge 1023 | 1024, 150 updated,
    1000 added); round 2 -> 5120 (100 removed, 50 updated, and as many added as it takes)."""
    ids = p.model.base_ids.copy()
    n = ids.size
    if round_no == 1:
        p.remove(ids[[60, 61, 62, 63, 64, 65, 1022, 1023, 1024, 1025, n - 2, n - 1]])
        p.update(ids[200:2000:12], spread(150, 543))
        want = 5121
    else:
        p.remove(ids[7:4107:41])
        p.update(ids[300:2300:40], spread(50, 553))
        want = 5120
    add = want - p.model.size()
    assert 90 <= add <= 1000, add
    p.add(spread(add, 545 + 10 * round_no))   # (seeds no other call uses: no copies)
    assert p.model.size() == want
    return want


def _scan_ran(index, n, bitmap):
    assert index.last_kernel_ms()[1] == NAME, index.last_kernel_ms()[1]
    assert index.debug_survivor_bitmap_bytes() == (_bitmap_bytes(n, NQ) if bitmap else 0)


def test_flat_hasher_folds_into_the_bitmap_form(tmp_path, monkeypatch):
    _knob(monkeypatch, None)               # the bitmap form; the planes are built under it, by create and by the fold
    rows, ix = flat_case()
    p = Pair(create(ix, rows), rows, 2048)
    q = spread(NQ, 561)
    for round_no in (1, 2):
        n2 = flat_round(p, round_no)
        what = "flat fold %d" % round_no
        _knob(monkeypatch, None)
        new_base, f = fold_and_compare(p, ix, tmp_path, q, what, opts=_opts())   # every query against the oracle
        assert new_base.size() == n2 == f["base_ids"].size and n2 % 1024 == (1 if round_no == 1 else 0)
        assert not p.model.identity
        new_base.enable_timing(True)
        staged = {}
        staged["1"] = new_base.search_batched(q, K, _opts(), stages=True)
        _scan_ran(new_base, n2, True)
        # the list form over the same planes, on a handle of its own (loaded from the folded base's file): no bitmaps
        _, path = file_arrays(new_base, tmp_path, "folded%d.scannidx" % round_no)
        _knob(monkeypatch, "0")
        lists = hip.load_file(path)
        lists.enable_timing(True)
        same_searches(lists, f, q, opts=_opts(), what=what + " lists")
        staged["0"] = lists.search_batched(q, K, _opts(), stages=True)
        _scan_ran(lists, n2, False)
        staged["0 folded"] = new_base.search_batched(q, K, _opts(), stages=True)   # and on the folded handle itself
        assert new_base.last_kernel_ms()[1] == NAME
        _same_staged(staged["1"], staged["0"], NQ, what + " bitmap / lists")
        _same_staged(staged["1"], staged["0 folded"], NQ, what + " bitmap / lists on the folded handle")
        lists.close()
        # through the rebased mutable handle, after further mutations: base row j answers under base_ids[j]
        _knob(monkeypatch, None)
        live = f["base_ids"]
        gone = live[[0, 63, 64, 1023, 1024, n2 - 1]]
        p.remove(gone)
        near_q = slice(3 * round_no, 3 * round_no + 3)       # (other queries each round: the rows must stay distinct)
        ids = p.add(q[near_q] + np.float32(1e-3))
        got = p.mut.search_batched(q, K, opts=_opts())
        _scan_ran(new_base, n2, True)
        check_lists(got, p.model.search_ah(f["codebook"], f["codes"], q, K, M), K, what + " through the handle")
        assert np.array_equal(got[0][near_q, 0], ids) and not np.isin(got[0], gone).any()
        ix = f
    p.close()


def tree_case():
    owner = np.repeat(np.arange(L), TREE_COUNTS)
    owner = owner[np.random.default_rng(571).permutation(owner.size)]
    rows = near(owner, 572)
    S = 8
    from test_gpu_fold import centres
    codebook = np.random.default_rng(573).random((S, 16, DIM // S), dtype=np.float32) * np.float32(0.3)
    ix = dict(kind="txh", centers=centres(), codebook=codebook, use_residuals=True, P=3, mult=float(M) / K)
    off, lid, codes = fm.frozen_build(ix, rows)
    assert np.diff(off).tolist() == list(TREE_COUNTS)
    ix.update(leaf_off=off, leaf_ids=lid, codes=codes)
    return rows, ix


def test_tree_folds_under_sp_words(tmp_path, monkeypatch):
    """20000 rows in 7 leaves, P = 3, m = 250, 65 queries: the sparse prefilter's word-parallel flush over the folded
    planes (leaf 3 emptied, leaf 5 filled, a delta of about 1500 rows merged into the middle of the leaves)"""
    _knob(monkeypatch, None, pairs=None, scan="sp-words")
    rows, ix = tree_case()
    p = Pair(create(ix, rows), rows, 2048)
    leaf3 = ix["leaf_ids"][ix["leaf_off"][3]:ix["leaf_off"][4]]
    script(p, 580, empty_leaf=leaf3)
    q = queries(581, NQ)
    new_base, f = fold_and_compare(p, ix, tmp_path, q, "tree fold")
    sizes = np.diff(f["leaf_off"])
    assert sizes[3] == 0 and sizes[5] > 0
    new_base.enable_timing(True)
    o = hip.default_opts()
    o.partitions_to_search, o.pre_reorder_k = 3, M
    new_base.search_batched(q, K, o)
    assert new_base.last_kernel_ms()[1] == NAME, new_base.last_kernel_ms()[1]
    p.close()

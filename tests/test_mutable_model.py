"""The reference's own unit tests of MutableDataset / IncrementalUpdater (mutator/mod.rs:600-646, 750-782), transcribed
against tests/mutable_model.py -- the model the GPU tests compare the library with -- plus the quirks the library
restates: double remove, revival, a full delta, ids never reused, rebase dropping ids, swap-remove at every position."""
import numpy as np
import pytest

import mutable_model as mm


def _empty(dim, capacity=64):
    return mm.MutableModel(np.zeros((0, dim), np.float32), capacity)


def test_mutable_dataset():
    """mod.rs:600-615"""
    d = _empty(3)
    idx0 = d.add([1.0, 2.0, 3.0])
    idx1 = d.add([4.0, 5.0, 6.0])
    assert d.size() == 2
    assert d.get(idx0).tolist() == [1.0, 2.0, 3.0]
    assert d.get(idx1).tolist() == [4.0, 5.0, 6.0]
    d.remove(idx0)
    assert d.size() == 1
    with pytest.raises(mm.NotFound):
        d.get(idx0)
    assert d.get(idx1).tolist() == [4.0, 5.0, 6.0]


def test_mutable_dataset_update():
    """mod.rs:617-626"""
    d = _empty(2)
    idx = d.add([1.0, 2.0])
    assert d.get(idx).tolist() == [1.0, 2.0]
    d.update(idx, [10.0, 20.0])
    assert d.get(idx).tolist() == [10.0, 20.0]


def test_mutable_dataset_compact():
    """mod.rs:628-646, compact() as export_live + rebase"""
    d = _empty(2)
    idx0, idx1, idx2 = d.add([1.0, 2.0]), d.add([3.0, 4.0]), d.add([5.0, 6.0])
    d.remove(idx1)
    assert d.size() == 2
    rows, ids = d.export_live()
    assert ids.tolist() == [idx0, idx2] and rows.tolist() == [[1.0, 2.0], [5.0, 6.0]]
    d.rebase(rows, ids)
    assert d.size() == 2
    assert d.exists(idx0) and not d.exists(idx1) and d.exists(idx2)
    assert d.get(idx2).tolist() == [5.0, 6.0]
    with pytest.raises(mm.NotFound):   # forgotten, not merely removed
        d.remove(idx1)
    assert d.add([7.0, 8.0]) == 3      # next_index is kept


def test_incremental_updater():
    """mod.rs:750-782: 50 mutations are not due at threshold 100, 100 are, the counter resets with the new index"""
    d = _empty(1, capacity=128)
    for i in range(50):
        d.add([float(i)])
    assert not d.needs_rebuild(100)
    for i in range(50, 100):
        d.add([float(i)])
    assert d.needs_rebuild(100) and d.pending() == 100
    rows, ids = d.export_live()
    assert ids.size == 100
    d.rebase(rows, ids)
    assert not d.needs_rebuild(100) and d.pending() == 0 and d.size() == 100


def _based(n=10, dim=2, capacity=8):
    rows = np.arange(n * dim, dtype=np.float32).reshape(n, dim)
    return mm.MutableModel(rows, capacity), rows


def test_double_remove_succeeds_and_counts():
    d, _ = _based()
    d.remove(3)
    d.remove(3)
    assert d.pending() == 2 and d.size() == 9 and not d.exists(3)
    a = d.add([1.0, 1.0])
    d.remove(a)
    d.remove(a)
    assert d.pending() == 5 and d.size() == 9
    with pytest.raises(mm.NotFound):
        d.remove(10_000)
    assert d.pending() == 5


def test_update_revives_removed_ids():
    d, rows = _based()
    d.remove(4)
    d.update(4, [9.0, 9.0])               # a removed base row
    assert d.exists(4) and d.get(4).tolist() == [9.0, 9.0] and d.size() == 10
    a = d.add([1.0, 2.0])
    d.remove(a)
    assert not d.exists(a)
    d.update(a, [3.0, 4.0])               # a removed former delta row
    assert d.exists(a) and d.get(a).tolist() == [3.0, 4.0]
    d.update(5, [7.0, 7.0])               # a live base row moves to the delta under its id
    assert d.get(5).tolist() == [7.0, 7.0] and not d.live[5] and d.slot(5) is not None
    d.update(5, [8.0, 8.0])               # a live delta row is overwritten in place
    assert d.get(5).tolist() == [8.0, 8.0] and len(d.delta_ids) == 3
    with pytest.raises(mm.NotFound):
        d.update(99, [0.0, 0.0])
    with pytest.raises(mm.InvalidArgument):
        d.update(5, [0.0, 0.0, 0.0])


def test_full_delta_changes_nothing():
    d, _ = _based(capacity=3)
    ids = d.add(np.ones((3, 2), np.float32))
    before = (d.size(), d.pending(), d.next_index, list(d.delta_ids))
    with pytest.raises(mm.ResourceExhausted):
        d.add([2.0, 2.0])
    with pytest.raises(mm.ResourceExhausted):
        d.update(0, [2.0, 2.0])           # a base row needs a new slot
    with pytest.raises(mm.ResourceExhausted):
        d.update([int(ids[0]), 1], np.zeros((2, 2), np.float32))   # all or nothing: the first element alone would fit
    assert before == (d.size(), d.pending(), d.next_index, list(d.delta_ids))
    assert d.get(int(ids[0])).tolist() == [1.0, 1.0] and d.live[0] and d.live[1]
    d.update(int(ids[1]), [5.0, 5.0])     # in place: no slot needed
    assert d.get(int(ids[1])).tolist() == [5.0, 5.0]


def test_batches_are_all_or_nothing():
    d, _ = _based()
    with pytest.raises(mm.NotFound):
        d.remove([1, 2, 77])
    assert d.size() == 10 and d.pending() == 0 and d.exists(1) and d.exists(2)
    with pytest.raises(mm.NotFound):
        d.update([1, 2, 77], np.zeros((3, 2), np.float32))
    assert d.pending() == 0 and d.live[1] and not d.delta_ids
    with pytest.raises(mm.InvalidArgument):
        d.add(np.zeros((2, 3), np.float32))
    assert d.next_index == 10


def test_ids_are_never_reused():
    d, _ = _based()
    a = d.add([1.0, 1.0])
    d.remove(a)
    b = d.add([2.0, 2.0])
    assert (a, b) == (10, 11)
    rows, ids = d.export_live()
    d.rebase(rows, ids)
    assert d.add([3.0, 3.0]) == 12


def test_rebase_drops_ids_and_rejects_unsorted():
    d, rows = _based()
    d.remove([2, 3])
    a = d.add([1.0, 1.0])
    r, ids = d.export_live()
    assert ids.tolist() == [0, 1, 4, 5, 6, 7, 8, 9, a]
    d.rebase(r, ids)
    assert not d.identity and d.size() == 9 and d.pending() == 0
    for gone in (2, 3):
        assert not d.exists(gone)
        with pytest.raises(mm.NotFound):
            d.update(gone, [0.0, 0.0])
        with pytest.raises(mm.NotFound):
            d.get(gone)
    assert d.get(a).tolist() == [1.0, 1.0] and d.get(4).tolist() == rows[4].tolist()
    with pytest.raises(mm.InvalidArgument):
        d.rebase(r, ids[::-1])
    with pytest.raises(mm.InvalidArgument):
        d.rebase(r[:2], [5, 5])


@pytest.mark.parametrize("where", ["first", "middle", "last", "only"])
def test_swap_remove_keeps_every_other_row(where):
    d, _ = _based(capacity=8)
    n = 1 if where == "only" else 5
    rows = np.arange(n * 2, dtype=np.float32).reshape(n, 2) + 100
    ids = np.atleast_1d(d.add(rows)).tolist()
    victim = {"first": 0, "middle": 2, "last": n - 1, "only": 0}[where]
    d.remove(ids[victim])
    assert len(d.delta_ids) == n - 1 and not d.exists(ids[victim])
    for i, id in enumerate(ids):
        if i != victim:
            assert d.get(id).tolist() == rows[i].tolist()
            assert d.delta_ids[d.slot(id)] == id
    if where == "first":   # the last row moved into the hole: slots are not id order
        assert d.delta_ids[0] == ids[-1]
    r, out = d.export_live()
    assert np.all(np.diff(out.astype(np.int64)) > 0) and out.size == d.size()


def test_allowed_mask_capacity_rule():
    words = np.array([0xFFFFFFFFFFFFFFFF, 0x1], np.uint64)
    ids = np.array([0, 63, 64, 65, 127, 128, 5000])
    assert mm.MutableModel.allowed(ids, words, None).tolist() == [True, True, True, False, False, False, False]
    assert mm.MutableModel.allowed(ids, words, 64).tolist() == [True, True, False, False, False, False, False]
    assert mm.MutableModel.allowed(ids, words, 0).tolist() == [False] * 7
    assert mm.MutableModel.allowed(ids, None, None).all()

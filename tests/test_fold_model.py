"""tests/fold_model.py against a from-scratch build with the model frozen (CPU only): the fold of base + tombstones +
delta must give, array for array, what assigning and encoding EVERY live row and filling the leaves in ascending
datapoint order gives -- provided the base's own codes came from the same encoder, which these cases arrange."""
import numpy as np
import pytest

import fold_model as fm
import mutable_model as mm
from oracle import pyoracle as orc
from scann_rust_amd import synth

N, DIM, L, S, K = 500, 16, 6, 4, 16


def tree_case(use_residuals, seed=3):
    rows = synth.uniform_f32(N, DIM, seed)
    rng = np.random.default_rng(seed)
    centers = np.ascontiguousarray(rows[np.sort(rng.choice(N, L, replace=False))])
    centers[4] = centers[1]                                   # two identical centres: the lower index takes the rows
    codebook = (rng.random((S, K, DIM // S), dtype=np.float32) - np.float32(0.5 if use_residuals else 0.0))
    ix = dict(kind="txh", centers=centers, codebook=codebook, use_residuals=use_residuals)
    off, lid, codes = fm.frozen_build(ix, rows)
    ix.update(leaf_off=off, leaf_ids=lid, codes=codes)
    assert off[5] - off[4] == 0                               # an empty leaf
    return rows, ix


def script(model, rows, seed):
    """adds (high ids), updates of low ids interleaved, removes over a bitmap word boundary; returns the updated ids"""
    new = synth.uniform_f32(90, DIM, seed)
    model.add(new[:30])
    up = np.array([1, 7, 63, 64, 65, 130, 257])
    model.update(up, new[30:37])
    model.add(new[37:60])
    model.remove(np.arange(60, 70))                           # straddles word 0 / word 1 (63 .. 65 are in the delta)
    model.remove([N - 1, N + 3])
    model.update([N + 5, 2], new[60:62])
    return np.append(up, 2)


def same_index(a, b_off, b_lid, b_codes):
    assert np.array_equal(a["leaf_off"], b_off)
    assert np.array_equal(a["leaf_ids"], b_lid)
    assert np.array_equal(a["codes"], b_codes)


@pytest.mark.parametrize("use_residuals", [True, False])
def test_fold_without_mutation_is_the_identity(use_residuals):
    rows, ix = tree_case(use_residuals)
    f = fm.fold(mm.MutableModel(rows, 128), ix)
    same_index(f, ix["leaf_off"], ix["leaf_ids"], ix["codes"])
    assert np.array_equal(f["rows"].view(np.uint32), rows.view(np.uint32))
    assert np.array_equal(f["base_ids"], np.arange(N))


@pytest.mark.parametrize("use_residuals", [True, False])
def test_fold_equals_a_frozen_build_over_the_live_rows(use_residuals):
    rows, ix = tree_case(use_residuals)
    model = mm.MutableModel(rows, 128)
    script(model, rows, 5)
    f = fm.fold(model, ix)
    live_rows, live_ids = model.export_live()
    assert np.array_equal(f["base_ids"], live_ids) and np.array_equal(f["rows"].view(np.uint32), live_rows.view(np.uint32))
    same_index(f, *fm.frozen_build(ix, live_rows))
    # a second fold, from non-identity ids
    fm.apply(model, f)
    assert not model.identity
    script2 = synth.uniform_f32(20, DIM, 6)
    model.add(script2[:10])
    model.update(live_ids[[0, 100, 300]], script2[10:13])
    model.remove(live_ids[200:210])
    f2 = fm.fold(model, f)
    live_rows, live_ids2 = model.export_live()
    assert np.array_equal(f2["base_ids"], live_ids2)
    same_index(f2, *fm.frozen_build(ix, live_rows))


def test_an_updated_low_id_lands_inside_its_leaf():
    rows, ix = tree_case(True)
    model = mm.MutableModel(rows, 16)
    off, lid = ix["leaf_off"], ix["leaf_ids"]
    leaf = int(np.argmax(np.diff(off)))
    members = lid[off[leaf]:off[leaf + 1]]
    victim = int(members[1])                                   # the leaf's second row: low rank, neighbours either side
    model.update(victim, rows[victim] + np.float32(1e-4))      # stays in its leaf
    assert fm.assign_encode(ix, model.get(victim)[None])[0][0] == leaf
    model.add(rows[int(members[2])])                           # and a high id in the same leaf: goes to the end
    f = fm.fold(model, ix)
    assert np.array_equal(f["base_ids"][:N], np.arange(N))     # nothing removed: new index == id
    got = f["leaf_ids"][f["leaf_off"][leaf]:f["leaf_off"][leaf + 1]]
    assert got.tolist() == members.tolist() + [N]
    assert got[1] == victim and got[-1] == N


def test_ids_counters_and_rows_survive_the_fold():
    rows, ix = tree_case(True)
    model = mm.MutableModel(rows, 128)
    script(model, rows, 7)
    ids = list(range(model.next_index))
    before = {i: model.get(i) for i in ids if model.exists(i)}
    size, nxt = model.size(), model.next_index
    fm.apply(model, fm.fold(model, ix))
    assert model.size() == size and model.next_index == nxt and model.pending() == 0 and not model.delta_ids
    assert all(model.exists(i) == (i in before) for i in ids)
    for i, r in before.items():
        assert np.array_equal(model.get(i).view(np.uint32), r.view(np.uint32))
    assert model.add(rows[0]) == nxt


def test_flat_hasher_and_brute_force():
    rows = synth.uniform_f32(N, DIM, 9)
    codebook = np.random.default_rng(9).random((S, K, DIM // S), dtype=np.float32)
    ix = dict(kind="ah", codebook=codebook, codes=orc.encode_many(codebook, rows))
    model = mm.MutableModel(rows, 128)
    f = fm.fold(model, ix)
    assert np.array_equal(f["codes"], ix["codes"])
    script(model, rows, 10)
    f = fm.fold(model, ix)
    live_rows, live_ids = model.export_live()
    assert np.array_equal(f["codes"], orc.encode_many(codebook, live_rows))
    b = fm.fold(model, dict(kind="bf"))
    assert np.array_equal(b["base_ids"], live_ids) and np.array_equal(b["rows"].view(np.uint32), live_rows.view(np.uint32))
    model.remove(live_ids)
    with pytest.raises(ValueError):
        fm.fold(model, ix)

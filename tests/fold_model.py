"""Pure numpy restatement of scann_hip_fold_mutable (include/scann_hip.h "fold") over the state of
tests/mutable_model.py: the arrays of the new base, with the trained model frozen.  Test infrastructure: the product
never imports it.

An index is a dict:
  kind "bf":  nothing more (the rows are the model's)
  kind "ah":  codebook [S][K][dsub], codes [n][S] (u8, by datapoint index)
  kind "txh": centers [L][dim], leaf_off [L + 1], leaf_ids [n], codebook, codes [n][S] in CSR order, use_residuals

fold(model, ix) -> (new index dict with "rows" [n'][dim] and "base_ids" [n'], same kind); the model is not changed.
apply(model, folded): the handle state after the call (the effects of rebase).

Base rows keep their leaf and their code bytes; delta rows are assigned with the oracle's partition(x, 1) and encoded
with its Codebook::encode (against the residual when use_residuals); leaf l holds its members in ascending new index."""
import numpy as np

from oracle import pyoracle as orc


def assign_encode(ix, rows):
    """(token, code [S]) of each row under the frozen model of a tree index"""
    centers, cb = ix["centers"], ix["codebook"]
    tok = np.array([int(orc.partition(centers, x, 1)[0][0]) for x in rows], np.int64).reshape(len(rows))
    tgt = rows - centers[tok] if ix["use_residuals"] and len(rows) else rows   # (f32 subtraction, as the encoder's)
    return tok, orc.encode_many(cb, np.ascontiguousarray(tgt, np.float32)).reshape(len(rows), cb.shape[0])


def fold(model, ix):
    rows, ids = model.export_live()
    if ids.size == 0:
        raise ValueError("InvalidArgument: Cannot build from empty dataset")
    out = dict(ix, rows=rows, base_ids=ids)
    if ix["kind"] == "bf":
        return out
    base_j = np.searchsorted(ids, model.base_ids)                 # new index of a LIVE base row
    d_ids = np.asarray(model.delta_ids, np.int64)
    d_rows = np.asarray(model.delta_rows, np.float32).reshape(d_ids.size, model.dim)
    d_j = np.searchsorted(ids, d_ids)
    S = ix["codebook"].shape[0]
    if ix["kind"] == "ah":
        codes = np.zeros((ids.size, S), np.uint8)
        codes[base_j[model.live]] = np.asarray(ix["codes"])[model.live]
        if d_ids.size:
            codes[d_j] = orc.encode_many(ix["codebook"], d_rows)
        out["codes"] = codes
        return out
    off, lid = np.asarray(ix["leaf_off"], np.int64), np.asarray(ix["leaf_ids"], np.int64)
    L = off.size - 1
    leaf_of_pos = np.repeat(np.arange(L), np.diff(off))
    keep = model.live[lid]                                          # surviving CSR positions
    d_tok, d_codes = assign_encode(ix, d_rows)
    leaf = np.concatenate([leaf_of_pos[keep], d_tok])
    j = np.concatenate([base_j[lid[keep]], d_j])
    codes = np.concatenate([np.asarray(ix["codes"], np.uint8)[keep], d_codes.astype(np.uint8)])
    assert j.size == ids.size and np.array_equal(np.sort(j), np.arange(ids.size)), "every live row in exactly one leaf"
    order = np.lexsort((j, leaf))                                   # by leaf, ascending new index inside a leaf
    new_off = np.zeros(L + 1, np.uint32)
    new_off[1:] = np.cumsum(np.bincount(leaf, minlength=L))
    out.update(leaf_off=new_off, leaf_ids=j[order].astype(np.uint32), codes=np.ascontiguousarray(codes[order]))
    return out


def frozen_build(ix, rows):
    """TreeXHybridSearcher::build over `rows` with the centres and the codebook given: assign + encode EVERY row, fill
    the leaves in ascending datapoint order (a stable argsort by leaf)"""
    tok, codes = assign_encode(ix, rows)
    order = np.argsort(tok, kind="stable")
    L = ix["centers"].shape[0]
    off = np.zeros(L + 1, np.uint32)
    off[1:] = np.cumsum(np.bincount(tok, minlength=L))
    return off, order.astype(np.uint32), np.ascontiguousarray(codes[order])


def apply(model, folded):
    """the handle after the fold: rebased onto the new rows under base_ids (identity when they are 0 .. n' - 1)"""
    ids = folded["base_ids"]
    identity = int(ids[-1]) == ids.size - 1
    model.rebase(folded["rows"], None if identity else ids)

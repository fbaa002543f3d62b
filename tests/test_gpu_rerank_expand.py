"""The bracket kernel of the 8-bit row filter (txh_rows.hip rerank_i8_kernel) with SCANN_HIP_RERANK_EXPAND = 1 (one
epilogue per wave; the one-scale int8 store by the expanded square) and 0 (per dimension, per round), on every row
family of tests/rerank_expand_model.py:

  rows      the filtered index returns the rows of an index built without the row store, bit for bit;
  brackets  read back with scann_hip_index_debug_rerank_brackets, every candidate's [L, U] contains the oracle's exact
            f32 distance of its row (float64 comparison; an infinite distance needs U = +inf, a NaN one is exempt);
  status    the device status is Ok.

Shapes: 3000 rows, 9 queries (SCANN_HIP_SMALL=0 keeps so few queries on the batched pipeline, where the filter runs).
dim 16 leaves one lane of eight with a slice of the row, 128 is one full pass with the query slice in registers, 144
and 272 end in a partial pass (272 also takes the LDS form), m = 64 leaves a block whose last six rounds are empty and
m = 1025 a fifth block with one candidate.  The NaN query of `nonfinite` stays out: its tables pass every point and the
device entry has no host retry (tests/test_gpu_rerank_rows.py)."""
import contextlib
import os

import numpy as np
import pytest

from oracle import pyoracle as orc
from scann_rust_amd import hip
from tests import helpers as H
from tests import rerank_expand_model as XM
from tests import rerank_filter_model as RM

pytestmark = pytest.mark.gpu

N, NQ = 3000, 9
DIMS = (16, 128, 144, 272)
KM = ((1, 64), (10, 1025))
STORES = {"i8-row": {"SCANN_HIP_RERANK_UNIFORM": "0"}, "i8-one": {"SCANN_HIP_RERANK_UNIFORM": "2"},
          "fp8": {"SCANN_HIP_RERANK_STORE": "fp8"}}
DONE = 0x80000000   # cand_count of a query whose rows rerank_short_kernel wrote itself
CREATE_KNOBS = ("SCANN_HIP_RERANK_I8", "SCANN_HIP_RERANK_STORE", "SCANN_HIP_RERANK_UNIFORM")


@contextlib.contextmanager
def _create_knobs(**kv):
    old = {k: os.environ.get(k) for k in CREATE_KNOBS}
    for k in CREATE_KNOBS:
        os.environ.pop(k, None)
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _stream():
    import torch
    return torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream


def _opts(m):
    o = hip.default_opts()
    o.pre_reorder_k = m
    return o


class Case:
    """one (family, dim): the rows, the oracle's exact distances of every (query, row), the index without a row store
    and its rows per (k, m) -- computed once, shared by the three stores"""

    def __init__(self, family, dim):
        d = XM.expand_rows(family, N, dim, NQ, seed=5)
        self.q = d["queries"][1:] if family == "nonfinite" else d["queries"]
        self.rows = d["rows"]
        data, stride = orc.to_strided(d["rows"])
        self.exact = np.stack([orc.one_to_many(q, data, stride, N, 0) for q in self.q])
        self.kw = H.ah_kwargs_from_codes(d["rows"], d["codebook"], d["codes"])
        with _create_knobs(SCANN_HIP_RERANK_I8="0"):
            self.plain = hip.txh_create(**self.kw)
        self.want = {}

    def filtered(self, store):
        with _create_knobs(SCANN_HIP_RERANK_I8="2", **STORES[store]):
            return hip.txh_create(**self.kw)

    def plain_rows(self, k, m):
        """(idx, dist, count) of the device entry and the candidates per query (the staged outputs of the host entry)"""
        if (k, m) not in self.want:
            status, di, dd, dc = H.device_search(self.plain, self.q, k, _opts(m))
            assert status == hip.OK
            cc = self.plain.search_batched(self.q, k, _opts(m), stages=True)[3][4]
            self.want[k, m] = (di, dd, dc, np.asarray(cc, np.uint32))
        return self.want[k, m]


@pytest.fixture(scope="module")
def case():
    cache = {}

    def get(family, dim):
        if (family, dim) not in cache:
            cache.clear()   # (the parameters come family by family, dim by dim: one case alive at a time)
            cache[family, dim] = Case(family, dim)
        return cache[family, dim]

    yield get
    cache.clear()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("store", list(STORES))
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("family", XM.FAMILIES)
def test_rows_brackets_and_status(case, family, dim, store, monkeypatch):
    c = case(family, dim)
    monkeypatch.setenv("SCANN_HIP_SMALL", "0")
    monkeypatch.setenv("SCANN_HIP_RERANK_I8_MIN", "1")
    filt = c.filtered(store)
    nq = c.q.shape[0]
    seen = {}
    for k, m in KM:
        wi, wd, wc, ncand = c.plain_rows(k, m)
        for knob in ("1", "0"):
            what = "%s dim %d %s k=%d m=%d expand=%s" % (family, dim, store, k, m, knob)
            monkeypatch.setenv("SCANN_HIP_RERANK_EXPAND", knob)
            status, di, dd, dc = H.device_search(filt, c.q, k, _opts(m))
            assert status == hip.OK, what
            assert np.array_equal(dc, wc), what + ": counts"
            assert np.array_equal(_bits(dd), _bits(wd)), what + ": distances"
            assert np.array_equal(di, wi), what + ": indices"
            lb, ub, rows, counts = filt.debug_rerank_brackets(nq, m, _stream())
            L, U = XM.from_ordered(lb), XM.from_ordered(ub)
            for i in range(nq):
                # (rerank_short_kernel replaces the count of a query it finished itself by DONE)
                cnt = int(ncand[i])
                assert counts[i] in (cnt, DONE) and 0 < cnt <= m and rows[i, :cnt].max() < N, what
                bad = RM.bracket_holds(L[i, :cnt], U[i, :cnt], c.exact[i][rows[i, :cnt]])
                assert not bad.any(), "%s q%d: %d of %d candidates outside their bracket, first at %d" % (
                    what, i, int(bad.sum()), cnt, int(np.flatnonzero(bad)[0]))
            seen[m, knob] = (lb, ub, counts)
            if knob == "1" and store == "i8-one" and family in ("duplicates", "permuted"):
                # the brackets are no wider than the model's by more than the summation order can explain (a bracket
                # of [-inf, +inf], or an inflated B, would pass everything above): within 2 x either way
                st = RM.make_store(store, c.rows)
                for i in range(nq):
                    r = rows[i, :int(ncand[i])]
                    acc, B = XM.expanded(st, c.q[i], r)
                    Lm, Um = XM.bracket(acc, st.E[r], B, dim)
                    got = U[i, :r.size].astype(np.float64) - L[i, :r.size].astype(np.float64)
                    want = Um.astype(np.float64) - Lm.astype(np.float64)
                    assert np.isfinite(want).all() and want.min() > 0.0, what
                    assert (got <= 2.0 * want).all() and (got >= 0.5 * want).all(), "%s q%d: bracket widths" % (what, i)
    if family == "duplicates" and store == "i8-one":
        # the knob reaches the kernel: B > 0 widens the expanded bracket (one-scale store) of every finite candidate
        (l1, u1, n1), (l0, u0, n0) = seen[1025, "1"], seen[1025, "0"]
        live = np.arange(1025)[None, :] < c.plain_rows(10, 1025)[3][:, None]
        assert ((l1 != l0) | (u1 != u0))[live].mean() > 0.9

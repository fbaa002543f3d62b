"""Shared builders/checkers for the parity tests (test infrastructure)."""
import numpy as np

from oracle import pyoracle as orc
from scann_rust_amd import synth, trainer


def make_txh_case(n, dim, L, S, seed, K=16, use_residuals=True, P=4, mult=3.0, clustered=False,
                  kmeans_iters=5, pq_iters=5):
    """Build one trained index + the oracle view and the kwargs of hip.txh_create."""
    if clustered:
        rows, _ = synth.clustered_f32(n, dim, seed, n_clusters=max(4, L))
    else:
        rows = synth.uniform_f32(n, dim, seed)
    data, stride = orc.to_strided(rows)
    ix = trainer.build_txh_index(rows, L, S, K=K, use_residuals=use_residuals, seed=seed,
                                 kmeans_iters=kmeans_iters, pq_iters=pq_iters)
    oix = orc.TxhIndex(data, stride, dim, ix["centers"], ix["leaf_off"], ix["leaf_ids"],
                       ix["codebook"], ix["codes"], use_residuals=use_residuals,
                       partitions_to_search=P, pre_reorder_multiplier=mult)
    kwargs = dict(data=data, n_rows=n, dim=dim, stride=stride, centers=ix["centers"],
                  leaf_offsets=ix["leaf_off"], leaf_ids=ix["leaf_ids"], codebook=ix["codebook"],
                  codes=ix["codes"], codes_packed4=False, use_residuals=use_residuals,
                  partitions_to_search=P, pre_reorder_multiplier=mult)
    return rows, data, stride, ix, oix, kwargs


def make_ah_case(n, dim, S, seed, K=16, pq_iters=5):
    rows = synth.uniform_f32(n, dim, seed)
    data, stride = orc.to_strided(rows)
    ix = trainer.build_ah_index(rows, S, K=K, seed=seed, pq_iters=pq_iters)
    kwargs = dict(data=data, n_rows=n, dim=dim, stride=stride, centers=None, leaf_offsets=None,
                  leaf_ids=None, codebook=ix["codebook"], codes=ix["codes"], codes_packed4=False,
                  use_residuals=False, partitions_to_search=1, pre_reorder_multiplier=1.0)
    return rows, data, stride, ix, kwargs


def assert_topk_equal_up_to_ties(got_idx, got_dist, want_idx, want_dist, rel=0.0, what=""):
    """SURVEY.md 8c parity rule: same index multiset up to groups whose distances tie
    (bit-equal when rel == 0, else within rel); distances equal position by position."""
    got_idx = np.asarray(got_idx); want_idx = np.asarray(want_idx)
    got_dist = np.asarray(got_dist, np.float32); want_dist = np.asarray(want_dist, np.float32)
    assert got_idx.shape == want_idx.shape, "%s: length %s vs %s" % (what, got_idx.shape, want_idx.shape)
    if rel == 0.0:
        assert np.array_equal(got_dist.view(np.uint32), want_dist.view(np.uint32)), \
            "%s: distances differ bitwise\n got %s\nwant %s" % (what, got_dist, want_dist)
    else:
        assert np.allclose(got_dist, want_dist, rtol=rel, atol=0.0), \
            "%s: distances differ\n got %s\nwant %s" % (what, got_dist, want_dist)
    if np.array_equal(got_idx, want_idx):
        return
    # differing positions must sit inside tie groups; the last group may be cut by k,
    # so only compare groups fully inside the result.
    n = got_idx.size
    i = 0
    while i < n:
        j = i
        while j + 1 < n and (want_dist[j + 1] == want_dist[i] if rel == 0.0 else
                             abs(want_dist[j + 1] - want_dist[i]) <= rel * abs(want_dist[i])):
            j += 1
        if j == n - 1 and j > i or (j == n - 1 and got_idx[i] != want_idx[i]):
            # tail group: membership may legitimately differ (tie cut by k / m)
            if i == j:
                # a single differing last element is a tie only if distances are equal,
                # which the distance check above already established.
                pass
        elif sorted(got_idx[i:j + 1].tolist()) != sorted(want_idx[i:j + 1].tolist()):
            raise AssertionError("%s: indices differ outside ties at [%d,%d]\n got %s\nwant %s"
                                 % (what, i, j, got_idx, want_idx))
        i = j + 1


def recall_at_k(retrieved, gt, k):
    """bin/ann_benchmark.rs:452-471."""
    tot = 0.0
    for r, g in zip(retrieved, gt):
        tot += len(set(r[:k].tolist()) & set(g[:k].tolist())) / float(k)
    return tot / len(retrieved)


def check_txh_query(oix, query, k, got_idx, got_dist, got_tok, got_tokd, got_ci, got_cd, what=""):
    """Stage-aware parity check of one Tree-X-Hybrid query against the oracle.

    tokens / centre distances: bit-exact.  Candidates: the sorted approximate distances
    must be bitwise identical; memberships may differ only inside ties of the approximate
    distance (FastTopNeighbors' slot-order tie behaviour is not reproduced: SURVEY 8c "up
    to distance ties").  Final rows: equal to the oracle's if the candidate sets agree,
    otherwise equal to the oracle's exact re-rank OF THE GPU's candidate list."""
    oi, od, otok, otokd, oci, ocd = orc.txh_search(oix, query, k, stages=True)
    P = otok.size
    assert np.array_equal(got_tok[:P], otok), "%s tokens" % what
    assert np.array_equal(np.asarray(got_tokd[:P], np.float32).view(np.uint32), otokd.view(np.uint32))
    assert got_ci.size == oci.size, "%s candidate count %d vs %d" % (what, got_ci.size, oci.size)
    assert np.array_equal(np.asarray(got_cd, np.float32).view(np.uint32), ocd.view(np.uint32)), \
        "%s approximate distances differ" % what
    assert_topk_equal_up_to_ties(got_ci, got_cd, oci, ocd, what=what + " cand")
    if sorted(got_ci.tolist()) == sorted(oci.tolist()):
        assert got_idx.size == oi.size
        assert_topk_equal_up_to_ties(got_idx, got_dist, oi, od, what=what + " final")
    else:
        ri, rd = orc.reorder(oix.data, oix.stride, oix.dim, query, got_ci, k)
        assert got_idx.size == ri.size
        assert_topk_equal_up_to_ties(got_idx, got_dist, ri, rd, what=what + " final(gpu cands)")


# ---- adversarial data for the brute-force kernels (tests/test_gpu_bf_adversarial.py) -------------------------
# Sample stride of every brute-force filter bound (bf.hip make_plan: rs = n / kBfSampleRows for n > 8192).
BF_SAMPLE_ROWS = 8192

ADVERSARIAL_FAMILIES = ("signed", "scaled-70", "scaled-20", "scaled+20", "scaled+56", "spread", "integers",
                        "duplicates", "zero", "overflow", "sample-adversarial")


def _scale_exp(family):
    """'scaled-70' -> -70: rows are U[-1, 1) x 2^s (exact: a power of two)."""
    return int(family[len("scaled"):])


def _signed(rng, shape):
    return rng.uniform(-1.0, 1.0, shape).astype(np.float32)


def adversarial_rows(family, n, dim, seed):
    """[n, dim] f32 rows of one family, deterministic from the seed.

    signed      U[-1, 1): dot distances take both signs, SquaredL2 cancels
    scaled<s>   signed x 2^s (s = -70: products are subnormal; s = +56: SquaredL2 stays finite)
    spread      each row x exp(U(-20, 20)), and every 8th dimension 2^30 larger than the rest
    integers    values in {-2, ..., 2}: exact arithmetic, massive exact ties, exactly orthogonal pairs
    duplicates  30 % of the rows are copies of 5 rows
    zero        signed, with three zero rows
    overflow    signed, with four rows of elements near 1e20 (SquaredL2 distance +inf, row norm overflows)
    sample-adversarial  rows at the filter-bound sample positions (i % rs == 0) lie far from every query
                (U[-1, -0.5)), all others near (U[0.5, 1)): every non-sampled row passes the bound
    """
    rng = np.random.default_rng([seed, 1])
    if family == "signed":
        return _signed(rng, (n, dim))
    if family.startswith("scaled"):
        return _signed(rng, (n, dim)) * np.float32(2.0 ** _scale_exp(family))
    if family == "spread":
        x = _signed(rng, (n, dim)) * np.exp(rng.uniform(-20.0, 20.0, (n, 1))).astype(np.float32)
        x[:, 3::8] *= np.float32(2.0 ** 30)
        return x.astype(np.float32)
    if family == "integers":
        return rng.integers(-2, 3, (n, dim)).astype(np.float32)
    if family == "duplicates":
        x = _signed(rng, (n, dim))
        protos = duplicate_protos(n)
        others = np.setdiff1d(np.arange(n), protos)
        copies = rng.choice(others, size=min(others.size, (3 * n) // 10), replace=False)
        x[copies] = x[rng.choice(protos, size=copies.size)]
        return x
    if family == "zero":
        x = _signed(rng, (n, dim))
        x[zero_rows(n)] = 0.0
        return x
    if family == "overflow":
        x = _signed(rng, (n, dim))
        big = overflow_rows(n)
        x[big] = (np.sign(_signed(rng, (big.size, dim))) * rng.uniform(0.5, 1.0, (big.size, dim)) *
                  1e20).astype(np.float32)
        return x
    if family == "sample-adversarial":
        rs = max(1, n // BF_SAMPLE_ROWS)
        x = rng.uniform(0.5, 1.0, (n, dim)).astype(np.float32)
        x[::rs] = -x[::rs]
        return x
    raise ValueError(family)


def duplicate_protos(n):
    """rows the duplicates family copies"""
    return np.arange(min(n, 5)) * max(1, n // 7)


def zero_rows(n):
    return np.unique(np.array([0, n // 3, n - 1]) % max(n, 1))


def overflow_rows(n):
    return np.unique(np.array([1, n // 4, n // 2, n - 2]) % max(n, 1))


def adversarial_queries(family, nq, dim, seed, rows):
    """[nq, dim] f32 queries matching adversarial_rows(family, ...) = `rows`, deterministic from the seed.
    integers: every 4th query is a row (distance 0); duplicates: every 3rd query is a copied row; zero: query 0
    is zero; sample-adversarial: U[0.5, 1), near every non-sampled row.  Others: the rows' distribution."""
    rng = np.random.default_rng([seed, 2])
    n = rows.shape[0]
    if family == "spread":
        q = _signed(rng, (nq, dim)) * np.exp(rng.uniform(-5.0, 5.0, (nq, 1))).astype(np.float32)
        q[:, 3::8] *= np.float32(2.0 ** 30)
        return q.astype(np.float32)
    if family == "integers":
        q = rng.integers(-2, 3, (nq, dim)).astype(np.float32)
        q[::4] = rows[rng.integers(0, n, q[::4].shape[0])]
        return q
    if family == "duplicates":
        q = _signed(rng, (nq, dim))
        q[::3] = rows[rng.choice(duplicate_protos(n), q[::3].shape[0])]
        return q
    if family == "sample-adversarial":
        return rng.uniform(0.5, 1.0, (nq, dim)).astype(np.float32)
    if family.startswith("scaled"):
        return _signed(rng, (nq, dim)) * np.float32(2.0 ** _scale_exp(family))
    q = _signed(rng, (nq, dim))
    if family == "zero":
        q[0] = 0.0
    return q


def bf16_split_ties(n, dim, seed):
    """(rows [n, dim], queries [4, dim]) on which the split-bf16 shortlist scores misorder exact DotProduct ties
    by far more than the bf16 pass's own rounding, but well inside its error bound (bf.hip shortlist_dot_err).

    Every query element is (1 + 2^-9) 2^e: split into hi = 2^e and lo = 2^(e-9).  Half of the row elements are
    1 + 2^-9 or 1 + 2^-8 (hi = 1, lo > 0), the other half 1 or 1 + 2^-7 (lo = 0).  The pass drops ql.xl, so a
    row's bf16 score is its exact DotProduct distance + 2^-9 sum(lo parts) 2^e.  1200 rows share the largest exact
    dot product in five levels that trade lo parts (B) for hi parts (C): the shortlist holds only the smallest-B
    level, at the highest indices, while the smallest indices of the tie lie in the largest-B level.  With dim 32
    every product and partial sum is exact in f32, so the ties are exact in every summation order."""
    assert dim == 32 and n >= 2000
    rng = np.random.default_rng([seed, 3])
    half = dim // 2
    x = np.ones((n, dim), np.float32)
    levels = [(half - 5, 16), (half - 4, 12), (half - 3, 8), (half - 2, 4), (half - 1, 0)]   # 4C + B = 4 half - 4
    cb = np.empty((n, 2), np.int64)
    per = 240
    for i, (c, b) in enumerate(levels):
        cb[i * per:(i + 1) * per] = (c, b)
    rest = np.arange(len(levels) * per, n)
    cb[rest, 0] = rng.integers(0, half - 6, rest.size)
    cb[rest, 1] = rng.integers(0, 9, rest.size)
    for r in range(n):
        c, b = cb[r]
        hi_dims = rng.permutation(half)[:c]
        lo_dims = half + rng.permutation(half)[:b]
        x[r, hi_dims] = np.float32(1.0 + 2.0 ** -7)
        x[r, half:] = np.float32(1.0 + 2.0 ** -9)
        x[r, lo_dims] = np.float32(1.0 + 2.0 ** -8)
    q = np.full((4, dim), 1.0 + 2.0 ** -9, np.float32) * np.array([1, 2, 4, 0.5], np.float32)[:, None]
    return x, q

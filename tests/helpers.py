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


def check_txh_query(oix, query, k, got_idx, got_dist, got_tok, got_tokd, got_ci, got_cd, what="", oracle=None):
    """Stage-aware parity check of one Tree-X-Hybrid query against the oracle.

    tokens / centre distances: bit-exact.  Candidates: the sorted approximate distances
    must be bitwise identical; memberships may differ only inside ties of the approximate
    distance (FastTopNeighbors' slot-order tie behaviour is not reproduced: SURVEY 8c "up
    to distance ties").  Final rows: equal to the oracle's if the candidate sets agree,
    otherwise equal to the oracle's exact re-rank OF THE GPU's candidate list.  `oracle`: the staged oracle outputs of
    this query (orc.txh_search(oix, query, k, stages=True)), where the caller keeps them.  They are trusted: the caller
    must have computed them for this very query, k, oix.allow and oix.pre_reorder_multiplier -- a stale tuple is
    compared against without any error."""
    oi, od, otok, otokd, oci, ocd = oracle if oracle is not None else orc.txh_search(oix, query, k, stages=True)
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


# ---- explicit-codebook indexes for the tree / flat hasher scans (tests/test_gpu_txh_subspaces.py) -------------------
# Codebooks and codes are written down, not trained: numpy k-means never sees the pathological tables, and the codes
# need not be anyone's nearest codeword (the reference's ADC scan only reads them).
PQ_FAMILIES = ("one-code", "flat", "flat-one", "dominant", "loose", "integers", "tiny", "huge", "nonfinite")
PQ_HUGE_EXP = 62


def pq_tables(codebook, q):
    """[S, K] f32 LUT of query q, with the reference's arithmetic (oracle lut_from_query)"""
    return orc.lut_from_query(codebook, q).reshape(codebook.shape[0], codebook.shape[1])


def adversarial_pq(family, n, dim, S, nq, seed):
    """(codebook [S, 16, dim / S] f32, codes [n, S] u8, rows [n, dim] f32, queries [nq, dim] f32) of one family.

    one-code  every row has code row A, every 1000th row code row B: all approximate distances tie in two groups,
              and the survivors of any bound overflow the candidate lists of a stream of >= ~30k points
    flat      every subspace's 16 codewords are equal: tables without a range (scale 0, every point passes)
    flat-one  subspace 1 alone is flat
    dominant  subspace 0's codewords (and the data / queries there) spread 2^20 wider than the rest: the int8 step is
              set by one subspace, every other one quantises to a few steps (a coarse, loose filter)
    loose     codeword 0 of every subspace lies far from every query and most rows use it in all but two subspaces: the
              bound sits beyond half of the int8 sum range (the sparse prefilter's coarser-scale branch)
    integers  codewords, rows and queries in {-2, ..., 2}: exact tables, massive exact ties at the bound
    tiny      everything x 2^-70: table entries are subnormal or zero
    huge      everything x 2^62: every table entry is finite, sums of S entries overflow to +inf (asserted)
    nonfinite codeword 5 of subspace 2 is +-1e20: that table entry is +inf (the pair is not quantised: all pass)
    """
    assert dim % S == 0
    dsub = dim // S
    rng = np.random.default_rng([seed, 7, S])
    cb = rng.uniform(-1.0, 1.0, (S, 16, dsub)).astype(np.float32)
    codes = rng.integers(0, 16, (n, S)).astype(np.uint8)
    q = rng.uniform(-1.0, 1.0, (nq, dim)).astype(np.float32)
    noise = 0.1
    if family == "one-code":
        rows_ab = rng.integers(0, 16, (2, S)).astype(np.uint8)
        codes[:] = rows_ab[0]
        codes[::1000] = rows_ab[1]
    elif family == "flat":
        cb[:] = cb[:, :1]
    elif family == "flat-one":
        cb[1] = cb[1, :1]
    elif family == "dominant":
        cb[0] *= np.float32(2.0 ** 20)
        q[:, :dsub] *= np.float32(2.0 ** 20)
    elif family == "loose":
        cb[:, 0] = 5.0
        far = rng.random((n, S)) < 0.999
        far[np.arange(n), rng.integers(0, S, n)] = False
        far[np.arange(n), rng.integers(0, S, n)] = False
        codes[far] = 0
        codes[~far] = rng.integers(1, 16, int((~far).sum())).astype(np.uint8)
    elif family == "integers":
        cb = rng.integers(-2, 3, (S, 16, dsub)).astype(np.float32)
        q = rng.integers(-2, 3, (nq, dim)).astype(np.float32)
    elif family == "nonfinite":
        cb[2, 5] = np.where(rng.random(dsub) < 0.5, -1e20, 1e20).astype(np.float32)
    elif family not in ("tiny", "huge"):
        raise ValueError(family)
    rows = cb[np.arange(S)[None, :], codes].reshape(n, dim)
    if family == "integers":
        rows = np.clip(rows + rng.integers(-1, 2, (n, dim)), -2, 2).astype(np.float32)
    elif family == "nonfinite":
        rows = np.clip(rows, -1.0, 1.0) + np.float32(noise) * rng.uniform(-1.0, 1.0, (n, dim)).astype(np.float32)
    else:
        rows = rows + np.float32(noise) * rng.uniform(-1.0, 1.0, (n, dim)).astype(np.float32)
    if family in ("tiny", "huge"):
        f = np.float32(2.0 ** (-70 if family == "tiny" else PQ_HUGE_EXP))
        cb, rows, q = cb * f, rows * f, q * f
    rows = np.ascontiguousarray(rows, np.float32)
    if family == "huge":
        for qi in q:
            t = pq_tables(cb, qi)
            assert np.all(np.isfinite(t)), "huge: a single table entry overflowed"
            with np.errstate(over="ignore"):
                assert np.isinf(t.max(1).sum(dtype=np.float32)), "huge: a sum of S entries stays finite"
    if family == "nonfinite":
        assert all(np.isinf(pq_tables(cb, qi)[2, 5]) for qi in q)
    return cb, codes, rows, np.ascontiguousarray(q, np.float32)


def pq_loose_bound_reached(codebook, codes, q, m):
    """True when the m-th smallest approximate distance of q puts the sparse prefilter's bound past half of the int8
    sum range (txh_prefilter.hip lut8_build_kernel: qmax > 128 S - 1 takes the coarser scale; the sampled bound is >= it)."""
    t = pq_tables(codebook, q).astype(np.float64)
    S = t.shape[0]
    _, od = orc.ah_search(codebook, codes, q, m)
    T = float(od[-1])
    sc = float((t.max(1) - t.min(1)).max()) / 255.0
    tq = T * (1.0 + S * 2.0 ** -23) - float(t.min(1).sum())
    return sc > 0 and np.floor(tq / sc + 0.5 * S + 1.0) > 128.0 * S - 1.0


def ah_kwargs_from_codes(rows, codebook, codes):
    """hip.txh_create kwargs of a flat hasher over explicit codes (the AsymmetricHasher view)."""
    n, dim = rows.shape
    data, stride = orc.to_strided(rows)
    return dict(data=data, n_rows=n, dim=dim, stride=stride, centers=None, leaf_offsets=None, leaf_ids=None,
                codebook=codebook, codes=np.ascontiguousarray(codes, np.uint8), codes_packed4=False,
                use_residuals=False, partitions_to_search=1, pre_reorder_multiplier=1.0)


def txh_from_codes(rows, codebook, codes, L, P, mult, seed, use_residuals=True, tree_rows=None):
    """(oracle TxhIndex, hip.txh_create kwargs) of a tree index over explicit codes: L centres picked among the rows,
    every row in its nearest centre's leaf (f64 distances, the lowest centre on ties), leaves in ascending row order,
    the codes in that CSR order (read against the residual to the leaf centre when use_residuals).  `tree_rows`: the
    rows the centres and the assignment are taken from, when they are not the indexed rows."""
    n, dim = rows.shape
    tr = rows if tree_rows is None else tree_rows
    rng = np.random.default_rng([seed, 9])
    centers = np.ascontiguousarray(tr[np.sort(rng.choice(n, L, replace=False))], np.float32)
    c64 = centers.astype(np.float64)
    assign = np.empty(n, np.int64)
    for r0 in range(0, n, 8192):
        x = tr[r0:r0 + 8192].astype(np.float64)
        assign[r0:r0 + 8192] = ((x[:, None, :] - c64[None]) ** 2).sum(2).argmin(1)
    order = np.argsort(assign, kind="stable").astype(np.uint32)
    leaf_off = np.zeros(L + 1, np.uint32)
    leaf_off[1:] = np.cumsum(np.bincount(assign, minlength=L))
    csr_codes = np.ascontiguousarray(codes[order], np.uint8)
    data, stride = orc.to_strided(rows)
    oix = orc.TxhIndex(data, stride, dim, centers, leaf_off, order, codebook, csr_codes, use_residuals=use_residuals,
                       partitions_to_search=P, pre_reorder_multiplier=mult)
    kw = dict(data=data, n_rows=n, dim=dim, stride=stride, centers=centers, leaf_offsets=leaf_off, leaf_ids=order,
              codebook=codebook, codes=csr_codes, codes_packed4=False, use_residuals=use_residuals,
              partitions_to_search=P, pre_reorder_multiplier=mult)
    return oix, kw


def check_ah_query(codebook, codes, data, stride, dim, query, k, m, got_idx, got_dist, got_ci, got_cd, what="",
                   oracle=None):
    """Stage-aware parity check of one AsymmetricHasher::search_with_reordering query (as check_txh_query): the sorted
    approximate candidate distances bitwise equal to the oracle's, memberships equal up to their ties; final rows
    equal to the oracle's if the candidate sets agree, else to the oracle's re-rank of the GPU's candidate list.
    `oracle`: (candidate idx, candidate dist, final idx, final dist) of this query from orc.ah_search and
    orc.ah_search_with_reordering, where the caller keeps them.  They are trusted: the caller must have computed them
    for this very codebook, codes, data, query, k and m -- a stale tuple is compared against without any error."""
    oci, ocd = oracle[:2] if oracle is not None else orc.ah_search(codebook, codes, query, m)
    assert got_ci.size == oci.size, "%s candidate count %d vs %d" % (what, got_ci.size, oci.size)
    assert np.array_equal(np.asarray(got_cd, np.float32).view(np.uint32), ocd.view(np.uint32)), \
        "%s approximate distances differ" % what
    assert_topk_equal_up_to_ties(got_ci, got_cd, oci, ocd, what=what + " cand")
    if sorted(got_ci.tolist()) == sorted(oci.tolist()):
        oi, od = oracle[2:] if oracle is not None else \
            orc.ah_search_with_reordering(codebook, codes, data, stride, query, k, m)
    else:
        oi, od = orc.reorder(data, stride, dim, query, got_ci, k)
    assert got_idx.size == oi.size, "%s final count %d vs %d" % (what, got_idx.size, oi.size)
    assert_topk_equal_up_to_ties(got_idx, got_dist, oi, od, what=what + " final")


# ---- rows for the re-rank row filter (tests/test_gpu_rerank_rows.py, tests/rerank_filter_model.py) -------------------
# The codebook and codes only choose the candidates: they are written down (codes = the nearest codeword of each row's
# unit-scale `base`), and the rows the re-rank reads are the family's.  The overflow families keep the codebook and the
# queries at unit scale, so that the scan's approximate distances stay finite while the exact ones overflow.
RERANK_FAMILIES = ("offset", "overflow-all", "overflow-most", "near-overflow", "tiny", "magnitudes", "spike", "permuted",
                   "duplicates", "nonfinite")
RERANK_OVERFLOW_EXP = 62
RERANK_FINITE_STRIDE = 1000   # overflow-most: rows i % 1000 == 7 stay finite (at most 9 of them below 10 000 rows)
FLT_MAX = float(np.finfo(np.float32).max)


def rerank_subspaces(dim):
    return 16 if dim % 16 == 0 else 8


def encode_codes(codebook, base):
    """[n, S] u8: the nearest codeword of every subspace of the unit-scale rows (float64)"""
    S, K, dsub = codebook.shape
    x = np.asarray(base, np.float64).reshape(base.shape[0], S, dsub)
    cb = codebook.astype(np.float64)
    codes = np.empty((base.shape[0], S), np.uint8)
    for s in range(S):
        codes[:, s] = ((x[:, s, None, :] - cb[None, s]) ** 2).sum(2).argmin(1)
    return codes


def overflow_finite_rows(n):
    return np.arange(7, n, RERANK_FINITE_STRIDE)


def _exact_all(rows, q):
    """[nq, n] oracle f32 SquaredL2 distances of every row"""
    data, stride = orc.to_strided(rows)
    return np.stack([orc.one_to_many(qi, data, stride, rows.shape[0], 0) for qi in q])


def rerank_rows(family, n, dim, nq, seed):
    """dict(codebook [S, 16, dim / S], codes [n, S] u8, rows [n, dim] f32, base [n, dim] f32 (unit scale: the tree's
    centres and assignment), queries [nq, dim] f32) of one family; each family asserts its premise.

    offset        rows and queries + 1000 (the codebook too): brackets wider than the candidates' spread
    overflow-all  rows x 2^62 (elements 0.6-1 in magnitude): every exact distance is +inf
    overflow-most overflow-all, except rows i % 1000 == 7, small and near every query: fewer than 10 finite distances
    near-overflow rows of squared norm 2^128 (1 +- 2^-9): distances straddle FLT_MAX
    tiny          everything x 2^-70: e^2 and d~ underflow, the 1e-30 floor carries the bracket
    magnitudes    rows x 2^+-20, half of the queries x 2^-20: under one scale the small rows quantise to 0
    spike         one coordinate per row (and query) 1000 x the rest: every other coordinate quantises to 0
    permuted      coordinate permutations of one int8-grid vector (scale 2^-4: x~ = x, E = 0); queries c (1, ..., 1):
                  the distances tie in real arithmetic and differ only by f32 summation order
    duplicates    rows 4i + 1 copy rows 4i, rows 4i + 2 differ from them by one ulp in one coordinate; every 3rd query
                  is a row
    nonfinite     rows with a NaN, +inf or -inf element, a zero row; query 0 holds a NaN, query 1 is a row, query 2 is
                  zero (the zero row: d~ = 0)
    """
    from tests import rerank_filter_model as RM
    assert dim % 16 == 0 or family in ("duplicates", "offset", "spike")
    S = rerank_subspaces(dim)
    rng = np.random.default_rng([seed, 11, dim])
    cb = rng.uniform(-1.0, 1.0, (S, 16, dim // S)).astype(np.float32)
    base = rng.uniform(-1.0, 1.0, (n, dim)).astype(np.float32)
    q = rng.uniform(-1.0, 1.0, (nq, dim)).astype(np.float32)
    f32 = np.float32
    if family == "offset":
        rows, q, cbr = base + f32(1000.0), q + f32(1000.0), cb + f32(1000.0)
    elif family in ("overflow-all", "overflow-most"):
        base = (np.sign(base) * rng.uniform(0.6, 1.0, (n, dim))).astype(np.float32)
        rows, cbr = base * f32(2.0 ** RERANK_OVERFLOW_EXP), cb
        if family == "overflow-most":
            fin = overflow_finite_rows(n)
            base[fin] = rng.uniform(-0.05, 0.05, (fin.size, dim)).astype(np.float32)
            rows[fin] = base[fin]
    elif family == "near-overflow":
        b64 = base.astype(np.float64)
        b64 /= np.linalg.norm(b64, axis=1, keepdims=True)
        rows = (b64 * 2.0 ** 64 * np.sqrt(1.0 + rng.uniform(-2.0 ** -9, 2.0 ** -9, (n, 1)))).astype(np.float32)
        cbr = cb
    elif family == "tiny":
        f = f32(2.0 ** -70)
        rows, q, cbr = base * f, q * f, cb * f
    elif family == "magnitudes":
        rows = base * np.where(rng.random((n, 1)) < 0.5, f32(2.0 ** -20), f32(2.0 ** 20))
        q = q * np.where(np.arange(nq)[:, None] % 2 == 0, f32(2.0 ** -20), f32(1.0))   # (2^20 queries: scan ties)
        cbr = cb
    elif family == "spike":
        for a in (base, q):
            j = rng.integers(0, dim, a.shape[0])
            a[np.arange(a.shape[0]), j] = np.where(rng.random(a.shape[0]) < 0.5, -1.0, 1.0) * \
                rng.uniform(500.0, 1000.0, a.shape[0])
        rows, cbr = base, cb
        base = np.clip(base, -1.0, 1.0)
    elif family == "permuted":
        v = rng.integers(-127, 128, dim).astype(np.float32)
        v[0] = 127.0
        rows = np.stack([v[rng.permutation(dim)] for _ in range(n)]) * f32(2.0 ** -4)
        base, cbr = rows / f32(8.0), cb
        q = np.repeat((f32(0.3) + f32(0.0137) * np.arange(nq, dtype=np.float32))[:, None], dim, axis=1)
    elif family == "duplicates":
        rows, cbr = base.copy(), cb
        m4 = (n // 4) * 4
        rows[1:m4:4] = rows[0:m4:4]
        rows[2:m4:4] = rows[0:m4:4]
        rows[2:m4:4, 5] = np.nextafter(rows[2:m4:4, 5], np.float32(np.inf))
        q[::3] = rows[rng.integers(0, n // 4, q[::3].shape[0]) * 4]
        base = rows
    elif family == "nonfinite":
        rows, cbr = base.copy(), cb
        bad = rng.choice(n, 60, replace=False)
        vals = np.array([np.nan, np.inf, -np.inf], np.float32)
        rows[bad, rng.integers(0, dim, bad.size)] = vals[np.arange(bad.size) % 3]
        rows[nonfinite_zero_row(n)] = 0.0
        base = np.where(np.isfinite(rows), rows, 0.0).astype(np.float32)
        q[0, 3] = np.nan
        q[1] = rows[np.setdiff1d(np.arange(n), bad)[17]]
        q[2] = 0.0
    else:
        raise ValueError(family)
    rows = np.ascontiguousarray(rows, np.float32)
    q = np.ascontiguousarray(q, np.float32)
    codes = encode_codes(cb, base if family != "offset" else rows - f32(1000.0))
    out = dict(codebook=np.ascontiguousarray(cbr, np.float32), codes=codes, rows=rows, base=base, queries=q)
    # ---- premises
    if family in ("overflow-all", "overflow-most", "near-overflow"):
        ex = _exact_all(rows, q)
        fin = np.isfinite(ex)
        if family == "overflow-all":
            assert not fin.any(), "overflow-all: an exact distance is finite"
        elif family == "overflow-most":
            assert (fin.sum(1) < 10).all() and (fin.sum(1) > 0).all(), fin.sum(1)
            d8 = RM.approx_distances(RM.i8_store(rows), q[0])
            assert (np.isinf(d8).sum() > n // 2), "overflow-most: d~ does not overflow"
        else:
            near = fin & (ex >= FLT_MAX * (1.0 - 2.0 ** -10))
            assert near.sum() > nq and (~fin).sum() > nq, (int(near.sum()), int((~fin).sum()))
    if family == "tiny":
        st = RM.i8_store(rows)
        assert np.mean(st.E == np.float32(1e-30)) > 0.9, "tiny: e^2 does not underflow"
        assert RM.approx_distances(st, q[0]).max() < np.finfo(np.float32).tiny
    if family == "magnitudes":
        st = RM.i8_store(rows, uni_scale=RM.i8_store(rows).deq.max())
        small = np.abs(rows).max(1) < 2.0 ** -19
        assert small.sum() > n // 4 and not st.codes[small].any(), "magnitudes: small rows keep a code under one scale"
    if family == "spike":
        st = RM.i8_store(rows)
        assert ((st.codes != 0).sum(1) == 1).all(), "spike: a coordinate besides the spike keeps a code"
    if family == "permuted":
        st = RM.i8_store(rows)
        assert (st.E == np.float32(1e-30)).all(), "permuted: x~ != x"
        ex = _exact_all(rows[:2000], q[:1])[0]
        assert np.unique(ex).size >= 3, "permuted: the f32 distances do not differ"
    if family == "duplicates":
        st = RM.i8_store(rows)
        m4 = (n // 4) * 4
        assert np.mean((st.codes[2:m4:4] == st.codes[0:m4:4]).all(1)) > 0.9, "duplicates: near-pairs differ in int8"
        ex = _exact_all(rows[:m4], q[:4])
        assert (ex[:, 2::4] != ex[:, 0::4]).any() and (ex[:, 1::4] == ex[:, 0::4]).all()
    if family == "nonfinite":
        st = RM.i8_store(rows)
        assert np.isinf(st.E[~np.isfinite(rows).all(1)]).all()
        assert RM.approx_distances(st, q[2], [nonfinite_zero_row(n)])[0] == 0.0
    if family == "offset":
        st = RM.i8_store(rows)
        for qi in q[:4]:
            Lb, Ub = RM.bracket(RM.approx_distances(st, qi), st.E, dim)
            assert Lb.max() < Ub.min(), "offset: a bracket is narrower than the rows' spread"
    return out


def nonfinite_zero_row(n):
    return n // 2 + 1


# ---- allow-list filters (tests/test_gpu_filters.py) -----------------------------------------------------------------
# Python mirror of the sample plan of csrc/txh.h (sample_stride / sample_plan / sample_rank) and of the candidate
# capacities plan_txh_search derives from it (api_search.hip), so that a test can name the points the threshold sample reads
# and the sizes at which a bound is statistical.
SAMPLE_TARGET, SAMPLE_MIN = 32768, 4096
WIDE_GROUPS = 16384


def sample_stride(total):
    ns = min(max(total // 16, SAMPLE_MIN), SAMPLE_TARGET)
    return max(1, -(-total // ns))


def sample_plan(max_stream, P):
    """(st, scap): stride and per-query sample capacity for a batch whose longest stream is max_stream points"""
    ms = min(int(max_stream), 0xFFFFFFFF)
    st = sample_stride(ms)
    while True:
        scap = ((-(-ms // st) + P) + 3) & ~3
        if scap <= SAMPLE_TARGET or P >= SAMPLE_TARGET - 4:
            return st, max(scap, 4)
        st += 1 + st // 8


def sample_rank(m, st):
    """J: the rank of the sampled bound (f32 arithmetic as in txh.h); 0 = no bound"""
    if m == 0:
        return 0
    r = np.float32(m) / np.float32(st)
    s = np.float32(0.5) * (np.float32(6.0) + np.sqrt(np.float32(36.0) + np.float32(4.0) * r, dtype=np.float32))
    jp = s * s + np.float32(2.0)
    j = m if jp >= np.float32(m) else int(jp)
    return max(1, min(j, m))


def plan_caps(max_stream, P, m):
    """(st, J, cap, cap32) of the batched pipeline's first attempt: cap = the candidate list of the f32 bound, cap32 =
    the integer prefilter's survivor list (plan_txh_search)"""
    ms = min(int(max_stream), 0xFFFFFFFF)
    st, _ = sample_plan(ms, P)
    j = sample_rank(m, st)
    cap = int(j + 8.0 * np.sqrt(j) + 16.0) * st + 256
    cap = min(max(cap, m), ms)
    return st, j, cap, min(ms, 4 * cap + 16384)


def wide_group(cnt, m):
    """stream positions per group minimum of the wide pipeline (txh.hip wide_group)"""
    g = 1
    while g < 64 and -(-cnt // g) > WIDE_GROUPS:
        g <<= 1
    while g > 1 and cnt // g < (m * 3) // 2:
        g >>= 1
    return g


def max_stream(leaf_off, P):
    """the longest stream of P leaves: the sum of the P largest"""
    return int(np.sort(np.diff(np.asarray(leaf_off, np.int64)))[::-1][:P].sum())


def words_of(ids, cap):
    """(words, cap): the bitmap of datapoint indices `ids` (all < cap) over ceil(cap / 64) words, at least one"""
    words = np.zeros(max(1, -(-cap // 64)), np.uint64)
    ids = np.asarray(ids, np.uint64)
    np.bitwise_or.at(words, (ids >> np.uint64(6)).astype(np.int64), np.uint64(1) << (ids & np.uint64(63)))
    return words, int(cap)


def allowed_ids(words, cap, n):
    """datapoint indices below n the bitmap (words, capacity cap) allows: bit i set and i < cap"""
    i = np.arange(min(n, cap, words.size * 64), dtype=np.uint64)
    return i[((words[(i >> np.uint64(6)).astype(np.int64)] >> (i & np.uint64(63))) & np.uint64(1)) == 1] \
        .astype(np.int64)


def masked_words(words, cap, n):
    """the bitmap as the reference reads it, over ceil(n / 64) words: bits at or past the capacity cleared"""
    return words_of(allowed_ids(words, cap, n), n)[0]


def sampled_rows(leaf_off, st):
    """CSR rows the threshold sample reads: positions j * st of every leaf (adc_sample_kernel)"""
    leaf_off = np.asarray(leaf_off, np.int64)
    return np.concatenate([np.arange(a, b, st) for a, b in zip(leaf_off[:-1], leaf_off[1:])])


FILTER_FAMILIES = ("empty", "one", "k-1", "m-1", "m", "m+1", "one-leaf", "unprobed", "f50", "f10", "f3", "f1", "f0.1",
                   "not-topk", "not-topm", "sampled", "unsampled", "wide-one-per-group", "wide-one-group",
                   "cap0", "cap1", "cap63", "cap64", "cap65", "cap-n-1", "cap-n", "cap-over", "prefix")


def allow_family(family, leaf_off, leaf_ids, tokens, k, m, st, seed, topk=None, topm=None):
    """(words, capacity) of the allow-set `family` over an index of CSR offsets leaf_off and row ids leaf_ids (None =
    identity).  tokens: [nq][P] the queries' probed leaves (query 0's decide the m-sized families); st: the sample
    stride of the batch; topk / topm: per query, the oracle's exact top-k / approximate top-m indices (the not-top
    families).  Deterministic for a given seed."""
    leaf_off = np.asarray(leaf_off, np.int64)
    n = int(leaf_off[-1])
    ids = np.arange(n, dtype=np.int64) if leaf_ids is None else np.asarray(leaf_ids, np.int64)
    rng = np.random.default_rng([seed, FILTER_FAMILIES.index(family)])
    tokens = np.asarray(tokens, np.int64)

    def rows_of(leaves):
        return np.concatenate([np.arange(leaf_off[l], leaf_off[l + 1]) for l in leaves] + [np.zeros(0, np.int64)])

    probed0 = ids[rows_of(tokens[0])]

    def spread(cnt):   # cnt of query 0's probed points, evenly spaced over its stream
        cnt = min(cnt, probed0.size)
        return probed0[np.linspace(0, probed0.size - 1, cnt).astype(np.int64)] if cnt else probed0[:0]

    if family == "empty":
        return words_of([], n)
    if family in ("one", "k-1", "m-1", "m", "m+1"):
        cnt = {"one": 1, "k-1": k - 1, "m-1": m - 1, "m": m, "m+1": m + 1}[family]
        return words_of(spread(cnt), n)
    if family == "one-leaf":
        return words_of(ids[rows_of([tokens[0][0]])], n)
    if family == "unprobed":
        return words_of(ids[rows_of(np.setdiff1d(np.arange(leaf_off.size - 1), tokens.ravel()))], n)
    if family[0] == "f":
        return words_of(np.flatnonzero(rng.random(n) < float(family[1:]) / 100.0), n)
    if family in ("not-topk", "not-topm"):
        drop = np.unique(np.concatenate([np.asarray(x, np.int64) for x in (topk if family == "not-topk" else topm)]))
        return words_of(np.setdiff1d(np.arange(n), drop), n)
    if family in ("sampled", "unsampled"):
        s = np.zeros(n, bool)
        s[ids[sampled_rows(leaf_off, st)]] = True
        return words_of(np.flatnonzero(s if family == "sampled" else ~s), n)
    if family in ("wide-one-per-group", "wide-one-group"):
        # stream positions of query 0 = its probed leaves in token order; groups of g positions
        g = wide_group(probed0.size, m)
        if family == "wide-one-per-group":
            return words_of(probed0[g // 2::g], n)
        grp = int(rng.integers(0, max(1, probed0.size // g)))
        return words_of(probed0[grp * g:(grp + 1) * g], n)
    # word and capacity edges: every bit of every word set, the stray bits past the capacity included
    cap = {"cap0": 0, "cap1": 1, "cap63": 63, "cap64": 64, "cap65": 65, "cap-n-1": n - 1, "cap-n": n,
           "cap-over": n + 100, "prefix": n // 2 + 7}[family]
    words = np.full(max(1, -(-cap // 64)), np.uint64(0xFFFFFFFFFFFFFFFF))
    if family == "prefix":   # a bitmap of a prefix of the index (ceil(cap / 64) words), every other row allowed
        words[:] = np.uint64(0x5555555555555555)
    return words, cap


# ---- forced scans and the device entry (tests/test_gpu_txh_subspaces.py, tests/test_gpu_filters.py) -----------------
SCAN_KNOBS = ("SCANN_HIP_MFMA", "SCANN_HIP_SMFMAC", "SCANN_HIP_RESIDENT", "SCANN_HIP_SP_WORDS", "SCANN_HIP_SMALL",
              "SCANN_HIP_WIDE", "SCANN_HIP_FUSED", "SCANN_HIP_RERANK_I8", "SCANN_HIP_RERANK_I8_MIN",
              "SCANN_HIP_RERANK_STORE", "SCANN_HIP_RERANK_UNIFORM", "SCANN_HIP_THR_TIES", "SCANN_HIP_THR_TAIL",
              "SCANN_HIP_SELECT_DIRECT", "SCANN_HIP_LOCAL_PRUNE")
SCANS = {
    "gather": {"SCANN_HIP_MFMA": "0", "SCANN_HIP_RESIDENT": "0"},
    "resident": {"SCANN_HIP_MFMA": "0", "SCANN_HIP_RESIDENT": "2"},
    "dense32": {"SCANN_HIP_SMFMAC": "0", "SCANN_HIP_MFMA": "2"},
    "mfma16": {"SCANN_HIP_MFMA": "3"},
    "sp-lanes": {"SCANN_HIP_SMFMAC": "1", "SCANN_HIP_MFMA": "2", "SCANN_HIP_SP_WORDS": "0"},
    "sp-words": {"SCANN_HIP_SMFMAC": "1", "SCANN_HIP_MFMA": "2", "SCANN_HIP_SP_WORDS": "1"},
    "default": {},
}


def scan_env(monkeypatch, scan):
    """Set the knobs of `scan` (before the index is created: SMFMAC=0 then builds no operand planes)."""
    for name in SCAN_KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, val in SCANS[scan].items():
        monkeypatch.setenv(name, val)


def sparse_kernel_name(S):
    return "adc_smfmac_kernel" if S <= 32 else "adc_smfmac_wide_kernel"


def scan_kernel_name(scan, S):
    """the kernel scann_hip_index_last_kernel_ms names for a batched search under `scan` (4-bit codes)"""
    if scan == "gather" or (scan == "resident" and S > 32):
        return "adc_scan_kernel"     # (the resident layout holds S <= 32)
    return {"resident": "adc_scan_res_kernel", "dense32": "adc_mfma_kernel", "mfma16": "adc_mfma16_kernel"}.get(
        scan, sparse_kernel_name(S))


def device_search(index, q, k, o, allow=None, allow_bits=None):
    """scann_hip_search_batched_device on torch's current stream: (status, idx, dist, count) after the call.  `allow`:
    a host bitmap, copied to the device for the call (capacity allow_bits, default every word)."""
    import ctypes
    import torch
    from scann_rust_amd import hip
    dev = torch.device("cuda:0")
    L = hip.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    nq, dim = q.shape
    qd = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(dev)
    oi = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
    od = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    oc = torch.full((nq,), 7, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    da = None
    if allow is not None:
        words = np.ascontiguousarray(allow, np.uint64)
        da = torch.from_numpy(words.view(np.int64).copy()).to(dev)
        o.allow_bitmap = ctypes.cast(ctypes.c_void_p(da.data_ptr()), ctypes.POINTER(ctypes.c_uint64))
        o.allow_bitmap_bits = words.size * 64 if allow_bits is None else int(allow_bits)
    torch.cuda.synchronize()
    try:
        hip.check(L.scann_hip_search_batched_device(index.h, p(qd), nq, dim, k, ctypes.byref(o), p(oi), p(od), p(oc),
                                                    st))
        status = L.scann_hip_index_last_device_status(index.h, st)
        torch.cuda.synchronize()
    finally:
        if da is not None:
            o.allow_bitmap, o.allow_bitmap_bits = None, 0
    return status, oi.cpu().numpy().view(np.uint32), od.cpu().numpy(), oc.cpu().numpy().view(np.uint32)


# ---- rows and centres for the index-build kernels (tests/test_gpu_build.py, tests/build_model.py) -------------------
# The brute-force families above, plus the three the build side needs: NaN rows, an all-equal set, and centre sets
# drawn from the rows themselves.
BUILD_FAMILIES = ("signed", "scaled-70", "scaled+56", "spread", "integers", "duplicates", "zero", "overflow", "nan",
                  "all-equal")


def nan_element_rows(n):
    """rows of the nan family with ONE NaN element"""
    return np.unique(np.array([2, n // 5, n // 2 + 3]) % max(n, 1))


def nan_whole_row(n):
    """the row of the nan family whose every element is NaN"""
    return (2 * n) // 3


def build_rows(family, n, dim, seed):
    """[n, dim] f32 rows of one BUILD_FAMILIES member.
    nan        signed, with a NaN in one element of three rows (the column moves with the row) and one whole-NaN row
               (when n >= 8; smaller sets keep one NaN element in row n - 1)
    all-equal  one signed row, n times
    others     adversarial_rows"""
    if family == "nan":
        x = _signed(np.random.default_rng([seed, 13]), (n, dim))
        if n < 8:
            x[n - 1, (dim - 1) // 2] = np.nan
            return x
        for r in nan_element_rows(n):
            x[r, int(r) % dim] = np.nan
        x[nan_whole_row(n)] = np.nan
        return x
    if family == "all-equal":
        return np.repeat(_signed(np.random.default_rng([seed, 14]), (1, dim)), n, axis=0)
    return adversarial_rows(family, n, dim, seed)


def centers_from_rows(rows, k, seed):
    """[k, dim] f32 centres drawn from the rows (so that rows hit a centre exactly: distance 0), every third one a copy
    of an earlier centre (ties between duplicated centres must go to the lowest index)"""
    rng = np.random.default_rng([seed, 15])
    c = np.ascontiguousarray(rows[rng.integers(0, rows.shape[0], k)], np.float32)
    for j in range(2, k, 3):
        c[j] = c[rng.integers(0, j)]
    return c


ENCODE_FAMILIES = ("dup", "equal", "nan-sub", "nan-code", "overflow", "tiny", "integers")


def encode_inputs(family, S, K, dsub, n, seed):
    """(codebook [S, K, dsub] f32, rows [n, S dsub] f32) on which an argmin and Codebook::encode's strict '<' against
    a running minimum of +inf can part ways.
    dup       two codewords of every subspace copy two others, every third row is made of such codewords (distance 0
              to both copies): the lowest index
    equal     every codeword of a subspace is the same: code 0
    nan-sub   40 rows with one NaN element, one whole-NaN row: every distance of that subspace is NaN -> code 0
    nan-code  NaN codewords are never chosen: codeword 0 of every subspace, all but the last codeword of subspace
              S - 2 (the last one wins), every codeword of subspace S - 1 (code 0)
    overflow  every 4th row x 1e20: distances overflow to +inf, which is not < +inf -> code 0; an infinite codeword
              (inf - inf = NaN against nothing, +inf against everything)
    tiny      everything x 2^-70: every squared difference is subnormal
    integers  codewords and rows in {-2, ..., 2}: exact arithmetic, massive exact ties"""
    rng = np.random.default_rng([seed, ENCODE_FAMILIES.index(family), S, K, dsub])
    cb = rng.uniform(-1, 1, (S, K, dsub)).astype(np.float32)
    x = rng.uniform(-1, 1, (n, S * dsub)).astype(np.float32)
    if family == "dup":
        pairs = [(K - 1 - i, i) for i in range(min(2, K // 2))]          # (copy, original), copy > original
        for hi, lo in pairs:
            cb[:, hi] = cb[:, lo]
        if pairs:
            pick = np.array([p[j] for p in pairs for j in (0, 1)])
            x[::3] = cb[np.arange(S), rng.choice(pick, (x[::3].shape[0], S))].reshape(-1, S * dsub)
    elif family == "equal":
        cb[:] = cb[:, :1]
    elif family == "nan-sub":
        x[rng.integers(0, n, min(n, 40)), rng.integers(0, S * dsub, min(n, 40))] = np.nan
        x[min(7, n - 1)] = np.nan
    elif family == "nan-code":
        cb[:, 0, dsub // 2] = np.nan
        cb[S - 2, :K - 1] = np.nan
        cb[S - 1] = np.nan
    elif family == "overflow":
        x[::4] *= np.float32(1e20)
        cb[min(1, S - 1), K // 2] = np.float32(3e38)
        cb[S - 1, 0] = np.inf
    elif family == "tiny":
        cb, x = cb * np.float32(2.0 ** -70), x * np.float32(2.0 ** -70)
    elif family == "integers":
        cb = rng.integers(-2, 3, (S, K, dsub)).astype(np.float32)
        x = rng.integers(-2, 3, (n, S * dsub)).astype(np.float32)
    else:
        raise ValueError(family)
    return np.ascontiguousarray(cb, np.float32), np.ascontiguousarray(x, np.float32)

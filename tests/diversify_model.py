"""CrowdingMultidimensional::apply (restricts/crowding.rs:166-200) and MmrDiversifier::apply (:217-267) restated: the
rules the multi-attribute crowded and the MMR searches are checked against.  All arithmetic in np.float32."""
import numpy as np

from oracle import pyoracle as orc

F32_MIN = np.float32(-3.4028234663852886e38)    # f32::MIN


def md_apply(idx, dist, attrs2d, limits, k):
    """(kept indices, kept distances) of one result row (already cut to its count).  attrs2d: [n_dims][n_attrs]
    uint64, an index at or past n_attrs has attribute 0 in every dimension; limits: one per dimension.  The literal
    walk, except that k = 0 keeps nothing (the reference tests the length after the push)."""
    idx, dist = np.asarray(idx), np.asarray(dist)
    attrs2d = np.asarray(attrs2d, np.uint64)
    n_dims, n_attrs = attrs2d.shape
    limits = [int(x) for x in limits]
    assert len(limits) == n_dims, "the reference panics on limits[dim]"
    have = idx < n_attrs
    a = np.zeros((n_dims, idx.size), np.uint64)
    a[:, have] = attrs2d[:, idx[have].astype(np.int64)]
    cols = [a[j].tolist() for j in range(n_dims)]
    counts = [dict() for _ in range(n_dims)]
    keep = []
    dims = range(n_dims)
    for pos in range(idx.size):
        if len(keep) >= k:
            break
        allowed = True
        for j in dims:
            if counts[j].get(cols[j][pos], 0) >= limits[j]:
                allowed = False
                break
        if allowed:
            for j in dims:
                c = counts[j]
                c[cols[j][pos]] = c.get(cols[j][pos], 0) + 1
            keep.append(pos)
    keep = np.asarray(keep, np.int64)
    return idx[keep].copy(), dist[keep].copy()


def mmr_apply(idx, dist, k, lam, sim):
    """The literal walk with a similarity callable sim(a, b) -> float.  Returns (indices, distances, fallbacks):
    entries in selection order; fallbacks = rounds in which no score exceeded f32::MIN (best_idx stayed 0)."""
    idx, dist = np.asarray(idx), np.asarray(dist, np.float32)
    lam = np.float32(min(max(np.float32(lam), np.float32(0)), np.float32(1)))
    oml = np.float32(1) - lam
    if idx.size == 0 or k == 0:
        return idx[:0].copy(), dist[:0].copy(), 0
    remaining = list(range(idx.size))
    selected = [remaining.pop(0)]
    fallbacks = 0
    with np.errstate(all="ignore"):
        while len(selected) < k and remaining:
            best_i, best_score, hit = 0, F32_MIN, False
            for i, p in enumerate(remaining):
                rel = -dist[p]
                max_sim = F32_MIN
                for s in selected:
                    max_sim = np.fmax(max_sim, np.float32(sim(int(idx[p]), int(idx[s]))))    # f32::max: NaN is ignored
                score = np.float32(lam * rel) - np.float32(oml * max_sim)
                if score > best_score:
                    best_score, best_i, hit = score, i, True
            fallbacks += 0 if hit else 1
            selected.append(remaining.pop(best_i))
    sel = np.asarray(selected, np.int64)
    return idx[sel].copy(), dist[sel].copy(), fallbacks


def pair_sims(measure, row, cand, stride, dim):
    """sim(candidate, row) = -DistanceMeasure::distance for every row of cand [m][stride], from the oracle:
    one_to_many for SquaredL2 / L2 / DotProduct, measure_distance per pair for L1 / Cosine."""
    m = cand.shape[0]
    if measure in (orc.L1, orc.COSINE):
        d = np.array([orc.measure_distance(measure, row[:dim], cand[i, :dim]) for i in range(m)], np.float32)
    else:
        d = orc.one_to_many(np.ascontiguousarray(row[:dim]), cand, stride, m, measure)
    return -np.asarray(d, np.float32)


def mmr_apply_rows(idx, dist, k, lam, data, stride, dim, measure):
    """mmr_apply with sim(a, b) = -distance(data[a], data[b]) under `measure`, without the quadratic fold: max_sim is
    a running np.fmax against the last selected row (the fold is a max, its order is free), one oracle call per
    round over the gathered candidate rows.  Same return value as mmr_apply."""
    idx, dist = np.asarray(idx), np.asarray(dist, np.float32)
    lam = np.float32(min(max(np.float32(lam), np.float32(0)), np.float32(1)))
    oml = np.float32(1) - lam
    cnt = idx.size
    if cnt == 0 or k == 0:
        return idx[:0].copy(), dist[:0].copy(), 0
    cand = np.ascontiguousarray(np.asarray(data, np.float32).reshape(-1, stride)[idx.astype(np.int64)])
    max_sim = np.full(cnt, F32_MIN, np.float32)
    free = np.ones(cnt, bool)
    free[0] = False
    selected, last, fallbacks = [0], 0, 0
    rel = -dist
    with np.errstate(all="ignore"):
        while len(selected) < min(k, cnt):
            max_sim = np.fmax(max_sim, pair_sims(measure, cand[last], cand, stride, dim))
            score = (lam * rel).astype(np.float32) - (oml * max_sim).astype(np.float32)
            ok = free & (score > F32_MIN)        # (a NaN score compares false)
            if ok.any():
                best = score[ok].max()
                last = int(np.flatnonzero(ok & (score == best))[0])    # the first of equal scores
            else:
                last = int(np.flatnonzero(free)[0])
                fallbacks += 1
            free[last] = False
            selected.append(last)
    sel = np.asarray(selected, np.int64)
    return idx[sel].copy(), dist[sel].copy(), fallbacks

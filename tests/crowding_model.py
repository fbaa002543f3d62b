"""CrowdingConstraint::apply (restricts/crowding.rs:81-104) restated: the rule every crowded search is checked against.

Walk the row in order; keep entry i iff fewer than `limit` earlier kept entries carry its attribute; stop at k kept.
A datapoint index at or past the attribute array has attribute 0 (get_attribute(idx).unwrap_or(0), :90)."""
import numpy as np


def attribute(attrs, idx):
    return int(attrs[idx]) if idx < len(attrs) else 0


def apply(idx, dist, attrs, limit, k, enabled=True):
    """(kept indices, kept distances) of one result row (already cut to its count)."""
    idx, dist = np.asarray(idx), np.asarray(dist)
    if not enabled:
        return idx[:k].copy(), dist[:k].copy()
    counts, keep = {}, []
    for pos, i in enumerate(idx.tolist()):
        if len(keep) >= k:
            break
        a = attribute(attrs, i)
        if counts.get(a, 0) < limit:
            counts[a] = counts.get(a, 0) + 1
            keep.append(pos)
    keep = np.asarray(keep, np.int64)
    return idx[keep].copy(), dist[keep].copy()


def apply_fast(idx, dist, attrs, limit, k):
    """apply() without the Python loop (the GPU tests run it over thousands of rows): an entry's rank among the
    equal attributes before it, by a stable sort; keep rank < limit; the first k.  Equal to apply() because with one
    attribute per entry "earlier kept" and "earlier" decide alike (tests/test_crowding_model.py checks it)."""
    idx, dist = np.asarray(idx), np.asarray(dist)
    attrs = np.asarray(attrs, np.uint64)
    a = np.zeros(idx.size, np.uint64)
    have = idx < attrs.size
    a[have] = attrs[idx[have].astype(np.int64)]
    order = np.argsort(a, kind="stable")
    sa = a[order]
    start = np.flatnonzero(np.r_[True, sa[1:] != sa[:-1]]) if idx.size else np.zeros(0, np.int64)
    group_start = np.repeat(start, np.diff(np.r_[start, idx.size]))
    rank = np.empty(idx.size, np.int64)
    rank[order] = np.arange(idx.size) - group_start
    keep = np.flatnonzero(rank < limit)[:k]
    return idx[keep].copy(), dist[keep].copy()

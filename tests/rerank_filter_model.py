"""numpy statement of the re-rank row filter (txh.hip K8b): the 8-bit row stores, the bracket [L, U] of
rerank_i8_kernel, and the selection rules of rerank_short_kernel, both for the single-GPU final stage and for the
local stage of a leaf-sharded search (ShortArgs::local_head).  The checker of tests/test_gpu_rerank_rows.py.

The model follows the kernels' f32 formulas but not their summation order, so it does not match them bit for bit.  It
serves two purposes: prove in float64 that the bracket holds around the oracle's exact f32 distance, and predict each
query's shortlist size (the library does not report whether rerank_short_kernel finished a query itself or handed it
to final_topk_kernel) with a wide margin.
"""
import numpy as np

from oracle import pyoracle as orc

F32 = np.float32
INF = F32(np.inf)
SHORT_MAX_FAST = 1024   # txh.hip kShortMaxFast: longer shortlists fall back to final_topk_kernel
LOCAL_HEAD = 256        # txh.hip kLocalHead: entries of a sharded rank's list that are always re-ranked exactly
UNIFORM_SPREAD = 1.02   # api_create.hip: one scale when the largest per-row scale is within 2 % of the mean
# the bracket's three parts (rerank_i8_kernel); a mutation test drops one of them
TERMS = ("error", "f32sum", "floor")


class Store:
    """An 8-bit row store as the filter reads it: x~[r] = deq[r] * codes[r] (int8) or deq[r] * e4m3(codes[r]) (FP8),
    E[r] >= ||x[r] - x~[r]||, +inf for a row with a NaN or infinite element."""

    def __init__(self, kind, codes, deq, E, uniform=False):
        self.kind, self.codes, self.deq, self.E, self.uniform = kind, codes, deq, E, uniform

    def decoded(self):
        if self.kind == "fp8":
            v = np.array([orc.fp8_to_f32(b) for b in range(256)], F32)[self.codes]
        else:
            v = self.codes.astype(F32)
        return v * self.deq[:, None]


def _row_max(x):
    # fmaxf ignores NaN operands: a row of NaNs has the maximum 0
    with np.errstate(invalid="ignore"):
        return np.fmax.reduce(np.abs(x), axis=1, initial=F32(0.0)).astype(F32)


def _error_bound(x, xt):
    with np.errstate(all="ignore"):
        e = (x - xt).astype(F32)
        err = (e * e).sum(axis=1, dtype=F32)
        E = (np.sqrt(err) * F32(1.0001) + F32(1e-30)).astype(F32)
    return E


def i8_store(rows, uni_scale=None):
    """rows_i8_build_kernel: sc = max|x| / 127 (1 for a zero or non-finite row), or the one scale `uni_scale`;
    q = clamp(rint(x / sc), -127, 127) (0 for NaN); E = sqrt(sum e^2) 1.0001 + 1e-30, +inf for a non-finite row."""
    x = np.asarray(rows, F32)
    mx = _row_max(x)
    finite = mx < INF
    if uni_scale is not None:
        sc = np.full(x.shape[0], uni_scale, F32)
    else:
        sc = np.where((mx > 0) & finite, mx / F32(127.0), F32(1.0)).astype(F32)
    with np.errstate(all="ignore"):
        t = np.clip(np.rint(x / sc[:, None]), -127, 127).astype(F32)
    t = np.where(np.isnan(t), F32(0.0), t)
    E = _error_bound(x, (sc[:, None] * t).astype(F32))
    E = np.where(np.isnan(E) | ~finite, INF, E).astype(F32)
    return Store("int8", t.astype(np.int8), sc, E)


def uniform_choice(store, mode=1):
    """api_create.hip: the one-scale rebuild is taken when every row is finite and the largest scale is within 2 % of the mean
    scale (SCANN_HIP_RERANK_UNIFORM: 0 never, 2 whenever the rows are finite).  Returns the one scale or None."""
    if mode == 0 or store.deq.size == 0:
        return None
    spread = 1e30 if mode == 2 else UNIFORM_SPREAD
    if not (np.all(store.E < INF) and np.all(store.deq < INF)):
        return None
    smax = F32(store.deq.max())
    if float(smax) > spread * float(store.deq.astype(np.float64).mean()):
        return None
    return smax


def i8_store_chosen(rows, mode=1):
    """the int8 store the library builds at index creation: per-row, or rebuilt with one scale and one error bound"""
    st = i8_store(rows)
    smax = uniform_choice(st, mode)
    if smax is None:
        return st
    uni = i8_store(rows, uni_scale=smax)
    emax = F32(uni.E.max())
    if not emax < INF:
        return st
    return Store("int8", uni.codes, uni.deq, np.full_like(uni.E, emax), uniform=True)


def fp8_store(rows):
    """rows_fp8_build_kernel: the reference's E4M3 codec with calibrate_scale = 448 / max|x| (1e-10 floor) per row,
    x~ = dec(code) * (1 / scale)."""
    x = np.asarray(rows, F32)
    mx = _row_max(x)
    finite = mx < INF
    scale = (F32(448.0) / np.maximum(np.where(finite, mx, F32(1.0)), F32(1e-10))).astype(F32)
    for r in range(0, x.shape[0], 4096):   # (spot check: the kernel's scale is the reference's calibrate_scale)
        if finite[r] and mx[r] > 0:
            assert orc.fp8_calibrate_scale(mx[r]) == scale[r]
    inv = (F32(1.0) / scale).astype(F32)
    with np.errstate(all="ignore"):
        codes = orc.fp8_quantize((x * scale[:, None]).astype(F32), 1.0)
    st = Store("fp8", codes, inv, None)
    E = _error_bound(x, st.decoded())
    st.E = np.where(np.isnan(E) | ~finite, INF, E).astype(F32)
    return st


def make_store(kind, rows):
    """kind: 'i8-row' (SCANN_HIP_RERANK_UNIFORM=0), 'i8-one' (=2), 'fp8' (SCANN_HIP_RERANK_STORE=fp8), 'i8' (default)"""
    if kind == "fp8":
        return fp8_store(rows)
    return i8_store_chosen(rows, {"i8-row": 0, "i8-one": 2, "i8": 1}[kind])


def approx_distances(store, q, rows_idx=None):
    """d~ = ||q - x~||^2 in f32 (one sequential sum per row: not the kernel's order)"""
    xt = store.decoded() if rows_idx is None else store.decoded()[rows_idx]
    with np.errstate(all="ignore"):
        d = (np.asarray(q, F32)[None, :] - xt).astype(F32)
        return (d * d).sum(axis=1, dtype=F32)


def bracket(acc, E, dim, nan_sign=+1, terms=TERMS, overflow_fix=True):
    """rerank_i8_kernel's [L, U] in f32.  slack = (2 sqrt(acc) E + E^2) 1.0001 + acc (dim + 8) 1.2e-7 + 1e-30; the bracket
    is unbounded when acc or slack is NaN or (overflow_fix) infinite.  numpy on x86 makes inf - inf the negative NaN,
    CDNA the positive one: nan_sign picks the sign the ordered-u32 comparison then sees (see ordered())."""
    acc = np.asarray(acc, F32)
    E = np.broadcast_to(np.asarray(E, F32), acc.shape)
    with np.errstate(all="ignore"):
        slack = np.zeros(acc.shape, F32)
        if "error" in terms:
            slack = ((F32(2.0) * np.sqrt(acc) * E + E * E) * F32(1.0001)).astype(F32)
        if "f32sum" in terms:
            slack = (slack + acc * (F32(dim + 8) * F32(1.2e-7))).astype(F32)
        if "floor" in terms:
            slack = (slack + F32(1e-30)).astype(F32)
        L = (acc - slack).astype(F32)
        U = (acc + slack).astype(F32)
    bad = np.isnan(slack) | np.isnan(acc)
    if overflow_fix:
        bad |= ~(slack < INF) | ~(acc < INF)
    L = np.where(bad, -INF, L).astype(F32)
    U = np.where(bad, INF, U).astype(F32)
    return _set_nan_sign(L, nan_sign), _set_nan_sign(U, nan_sign)


def _set_nan_sign(v, sign):
    b = v.view(np.uint32).copy()
    nan = np.isnan(v)
    b[nan] = (b[nan] & np.uint32(0x7FFFFFFF)) | np.uint32(0x80000000 if sign < 0 else 0)
    return b.view(F32)


def ordered(v):
    """common.h f32_to_ordered: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN"""
    b = np.ascontiguousarray(v, F32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def bracket_holds(L, U, exact):
    """float64 proof: L <= exact <= U for every candidate with a non-NaN exact distance (an infinite exact distance
    needs U = +inf).  Returns the boolean mask of the candidates where it fails."""
    L64, U64, x64 = (np.asarray(a, F32).astype(np.float64) for a in (L, U, exact))
    with np.errstate(invalid="ignore"):
        ok = (L64 <= x64) & (x64 <= U64)
    return ~ok & ~np.isnan(x64)


def tau(U, k, head=0):
    """the k-th smallest ordered upper bound among the first `head` entries (all when head == 0); +inf-ordered
    (0xFFFFFFFF) when there are at most k of them -- everything is shortlisted then"""
    u = ordered(U)
    if head:
        u = u[:head]
    if u.size <= k:
        return np.uint32(0xFFFFFFFF)
    return np.partition(u, k - 1)[k - 1]


def shortlist(L, U, k, head=0):
    """rerank_short_kernel's keep rule: entry i is re-ranked exactly when i < head or ordered(L_i) <= tau"""
    t = tau(U, k, head)
    keep = ordered(L) <= t
    if head:
        keep[:head] = True
    return keep


def final_path(ns, nsel, k):
    """'fast' when rerank_short_kernel writes the rows itself, else 'topk256' / 'topk1024' (final_topk_kernel over
    cand_exact; the launcher picks 1024 threads above m = 2048).  A shortlist under min(k, nsel) rows re-ranks the
    query without the filter."""
    if ns <= SHORT_MAX_FAST and ns >= min(k, nsel):
        return "fast"
    return "unfiltered" if ns < min(k, nsel) else "fallback"


def topk_by_exact_key(exact, keys, k):
    """the stable sort's first k by (exact, merge key): candidate positions"""
    o = ordered(exact).astype(np.uint64)
    return np.lexsort((np.asarray(keys, np.uint64), o))[:k]


def pruned_dominated(exact, keys, pruned, k, head=LOCAL_HEAD):
    """Local stage: every pruned entry must have at least k entries among the first `head` of its list that come
    before it in (exact, key) order (exact distances of the unpruned run).  Returns the pruned positions that do not."""
    o = ordered(exact).astype(np.uint64)
    kk = np.asarray(keys, np.uint64)
    ho, hk = o[:head], kk[:head]
    bad = []
    for i in np.nonzero(pruned)[0]:
        before = (ho < o[i]) | ((ho == o[i]) & (hk < kk[i]))
        if int(before.sum()) < k:
            bad.append(int(i))
    return bad


def filter_applies(dim, measure=0):
    """the launcher's conditions on the index: squared L2 and dim % 16 == 0 (the store is not even built otherwise)"""
    return measure == 0 and dim % 16 == 0

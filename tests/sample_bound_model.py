"""numpy statement of the flat hasher's filter bound from an integer sample (txh.hip K5d / K5e): the plain
quantiser of lut8_build_kernel (fold < 0), the integer sums adc_sample_mfma_kernel stores, and the two passes of
threshold_tail16_kernel; next to them the bound it has to reproduce, threshold_tail_kernel's over the f32 sample.

A sample is `codes` [ns, S] (one 4-bit code per subspace) scored against one query's table [S, 16] f32; sample slot i
is row i.  Keys are (ordered f32 distance << 32) | slot, as the kernels form them; KEY_MAX = no bound.
"""
import numpy as np

F32 = np.float32
KEY_MAX = (1 << 64) - 1
ABSENT32 = 0xFFFFFFFF
ABSENT16 = 0xFFFF
THREADS = 256     # txh.hip kThrTailThreads
LIST = 2048       # txh.hip kThrTailList
EPS23 = 2.0 ** -23


def ordered(d):
    """common.h f32_to_ordered on an f32 array -> uint64 (values < 2^32)"""
    b = np.asarray(d, F32).view(np.uint32).astype(np.uint64)
    neg = (b >> np.uint64(31)) != 0
    return np.where(neg, b ^ np.uint64(0xFFFFFFFF), b | np.uint64(0x80000000))


def distances(table, codes):
    """the reference's sums (hashes/lut.rs:74-82): acc = t[0][c0]; acc += t[s][cs], sequential f32"""
    t = np.asarray(table, F32)
    with np.errstate(all="ignore"):
        acc = t[0, codes[:, 0]].copy()
        for s in range(1, t.shape[0]):
            acc = (acc + t[s, codes[:, s]]).astype(F32)
    return acc


def keys_of(d, present=None):
    """merge keys of the sample in slot order; absent slots get KEY_MAX"""
    k = (ordered(d) << np.uint64(32)) | np.arange(d.size, dtype=np.uint64)
    if present is not None:
        k = np.where(present, k, np.uint64(KEY_MAX))
    return k


def quantise(table):
    """lut8_build_kernel, plain tables: (q [S, 16] in 0..255, bias_sum f64, scale f64); scale 0 = not quantised"""
    t = np.asarray(table, F32)
    with np.errstate(all="ignore"):
        bad = bool(np.any(~(t >= 0)) or np.any(~(t < np.inf)))
        mn = np.fmin.reduce(t, axis=1)
        mx = np.fmax.reduce(t, axis=1)
        rng = (mx - mn).astype(F32)
        r = F32(np.fmax.reduce(rng, initial=F32(0.0)))
    bias = float(np.sum(mn.astype(np.float64))) if not bad else float("nan")
    if bad or not r > 0:
        return np.zeros(t.shape, np.int64), bias, 0.0
    sc = float(r) / 255.0
    q = np.floor((t.astype(np.float64) - mn.astype(np.float64)[:, None]) / sc + 0.5)
    return np.clip(q, 0, 255).astype(np.int64), bias, sc


def integer_sample(q, codes, present=None):
    """adc_sample_mfma_kernel: u = sum_s q[s][code_s] (the MFMA sums + 128 S), 0xFFFF for a rejected sample"""
    u = q[np.arange(q.shape[0])[None, :], codes].sum(axis=1)
    assert u.max(initial=0) < ABSENT16
    if present is not None:
        u = np.where(present, u, ABSENT16)
    return u.astype(np.int64)


def _kept(vals, absent):
    """the two smallest values of every thread: thread t takes the groups of four samples t, t + 256, ..."""
    n4 = -(-vals.size // 4)
    v = np.full(n4 * 4, absent, np.int64)
    v[:vals.size] = vals
    g = v.reshape(n4, 4)
    rounds = -(-n4 // THREADS)
    pad = np.full((rounds * THREADS, 4), absent, np.int64)
    pad[:n4] = g
    per_thread = pad.reshape(rounds, THREADS, 4).transpose(1, 0, 2).reshape(THREADS, -1)
    return np.sort(per_thread, axis=1)[:, :2].ravel()


def _jth(sorted_vals, J, absent):
    return int(sorted_vals[J - 1]) if J <= sorted_vals.size else absent


def round_up_f32(x):
    f = F32(x)
    if float(f) < x:
        f = np.nextafter(f, F32(np.inf))
    return f


def collect_limit(P, S, bias, scale):
    """(Dmax, qlim) of a present pivot P (threshold_tail16_kernel, f64)"""
    eps = S * EPS23
    dmax = (bias + scale * (P + S * (0.5 + 1e-9))) * (1.0 + eps)
    with np.errstate(all="ignore"):
        ql = np.floor((dmax * (1.0 + eps) - bias) / scale + 0.5 * S + 1.0)
    return dmax, (ABSENT16 - 1 if not ql < ABSENT16 - 1 else int(ql))


def tail32_bound(d, present, J, list_cap=LIST):
    """threshold_tail_kernel over the f32 sample: (bound key, flooded)"""
    o = ordered(d).astype(np.int64)
    vals = np.where(present, o, ABSENT32) if present is not None else o
    if J == 0 or vals.size < J:
        return KEY_MAX, False
    pivot = _jth(np.sort(_kept(vals, ABSENT32)), J, ABSENT32)
    if pivot == ABSENT32:
        pivot = ABSENT32 - 1
    sel = np.flatnonzero(vals <= pivot)
    if sel.size < J:
        return KEY_MAX, False
    if sel.size > list_cap:
        return (pivot << 32) | 0xFFFFFFFF, True
    k = np.sort((vals[sel].astype(np.uint64) << np.uint64(32)) | sel.astype(np.uint64))
    return int(k[J - 1]), False


class Sample:
    """One query's sample, with everything that does not depend on J computed once: the f32 distances and keys of the
    reference, the quantiser's output, the integer sums and the threads' kept values."""

    def __init__(self, table, codes, present=None):
        self.table = np.asarray(table, F32)
        self.S, self.ns = self.table.shape[0], codes.shape[0]
        self.present = present
        self.d = distances(self.table, codes)
        self.keys = keys_of(self.d, present)
        self.q, self.bias, self.scale = quantise(self.table)
        self.u = integer_sample(self.q, codes, present)
        self.kept16 = np.sort(_kept(self.u, ABSENT16))

    def reference(self, J):
        """the J-th smallest f32 sample key (KEY_MAX with fewer than J present samples)"""
        k = np.sort(self.keys)
        return int(k[J - 1]) if 0 < J <= k.size else KEY_MAX


def tail16_bound(smp, J, list_cap=LIST):
    """lut8_build(plain) -> adc_sample_mfma -> threshold_tail16 on a Sample: (bound key, collected slots or None for
    the f32 passes, flooded)"""
    if J == 0 or smp.ns < J:
        return KEY_MAX, None, False
    if not smp.scale > 0.0:   # the f32 passes, sample to thread as threshold_tail_kernel
        key, flooded = tail32_bound(smp.d, smp.present, J, list_cap)
        return key, None, flooded
    P = _jth(smp.kept16, J, ABSENT16)
    if P == ABSENT16:
        lim, flood = ABSENT16 - 1, ABSENT32 - 1
    else:
        dmax, lim = collect_limit(P, smp.S, smp.bias, smp.scale)
        flood = int(ordered(np.array([round_up_f32(dmax)], F32))[0])
    sel = np.flatnonzero(smp.u <= lim)
    if sel.size < J:
        return KEY_MAX, sel, False
    if sel.size > list_cap:
        return (flood << 32) | 0xFFFFFFFF, sel, True
    k = np.sort(smp.keys[sel])   # (the kernel recomputes these distances: the same arithmetic)
    return int(k[J - 1]), sel, False


# ---- table families of tests/test_sample_bound_model.py ---------------------------------------------------------------
FAMILIES = ("uniform", "range", "bias", "flat-some", "subnormal", "three-valued", "bias-mild")
# Families whose list may flood: the huge-range one and the tie families.  "bias" is a tie family in f32: at a bias
# 10^6 x the range every distance is ~S 10^6 with a spacing of 0.5-4 between neighbouring f32 values against a spread
# of the sums of a few units, so the sample holds a few dozen distinct distances (asserted by the test), and the
# rounding term of the collect limit, ~2 S^2 2^-23 bias / scale, alone exceeds the whole range 255 S of the sums.
# There the new path publishes the looser (Dmax, MAX) where threshold_tail_kernel may still find the exact key (its
# f32 pivot group can fit the list): a deliberate widening of "tie and huge-range families only", stated in DESIGN 3.1d.
FLOOD_ALLOWED = ("range", "three-valued", "bias")


def family_table(family, S, seed):
    rng = np.random.default_rng([seed, FAMILIES.index(family), S])
    t = rng.uniform(0.0, 1.0, (S, 16)).astype(F32)
    if family == "range":          # one subspace's range 10^6 x the others'
        t[S // 2] *= F32(1e6)
    elif family == "bias":         # bias 10^6 x the range
        t = (t + F32(1e6)).astype(F32)
    elif family == "bias-mild":    # bias 10^3 x the range: the rounding term stays a few steps
        t = (t + F32(1e3)).astype(F32)
    elif family == "flat-some":    # all entries equal in some subspaces
        t[::3] = t[::3, :1]
    elif family == "subnormal":
        t = (t * F32(1e-40)).astype(F32)
        assert np.all(t < np.finfo(F32).tiny)
    elif family == "three-valued":  # thousands of exact ties
        t = rng.choice(np.array([0.0, 1.0, 4.0], F32), (S, 16))
    return t


def family_codes(ns, S, seed):
    return np.random.default_rng([seed, 99, S]).integers(0, 16, (ns, S))

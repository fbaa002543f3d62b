"""Allow-list filters on brute-force handles (scann_hip_search_opts.allow_bitmap; include/scann_hip.h).

The contract: a filtered brute-force search answers exactly as an unfiltered search over a handle built from the
allowed rows alone, in ascending datapoint order, indices mapped back.  So the expected rows need nothing new from
the oracle: orc.bf_search_batched / orc.bf_search_radius (f32 rows) or the quantized checker + orc.topk_run run on
`rows[allowed]`, and their indices go back through `allowed`.  Distances are compared bitwise, indices up to exact
distance ties (H.assert_topk_equal_up_to_ties), and no returned index may be a disallowed one.

Every kernel family of bf.hip is crossed with both plans (n <= 8192: the sorted sample is the answer; n above it:
sample + filter pass + select), with both mechanisms (SCANN_HIP_BF_FILTER = 1: compacted id list, 2: bit test at
the emit) and the default rule, and with the filter families of `allow_of`."""
import ctypes

import numpy as np
import pytest

from oracle import pyoracle as orc
from scann_rust_amd import hip, synth
from tests import helpers as H
from tests import quantized_checker as qc
from tests.test_gpu_quantized_bf import make_rows, same

pytestmark = pytest.mark.gpu

SQL2, L2, DOT, L1, COS = hip.SQUARED_L2, hip.L2, hip.DOT_PRODUCT, hip.L1, hip.COSINE
SAMPLE = 8192           # kBfSampleRows
N_DIRECT = 3001         # <= SAMPLE: the direct plan
N_BIG = 20013           # > SAMPLE: the sample reads every 2nd row (rs = 2); not a multiple of 32 or 64
MECHS = (("default", None), ("compact", "1"), ("bittest", "2"))
FAMILIES = ("all", "f50", "f10", "f1", "lt-k", "one", "none", "cap0", "cap-short", "head", "tail", "sampled",
            "unsampled")
FEW = ("f50", "f1", "lt-k", "cap-short", "unsampled")   # the subset every kernel instantiation sees
EMPTY = ("none", "cap0")


def sample_stride(n):
    return 1 if n <= SAMPLE else n // SAMPLE


def allow_of(family, n, k, seed=5):
    """(words, capacity) of a filter family over n rows; deterministic.  Every family but "none" / "cap0" allows at
    least one row by construction."""
    rng = np.random.default_rng([seed, FAMILIES.index(family)])
    rs = sample_stride(n)
    sampled = np.arange(min(n, SAMPLE), dtype=np.int64) * rs     # the rows the sample pass reads
    if family == "all":
        return np.full(-(-n // 64), np.uint64(0xFFFFFFFFFFFFFFFF)), n
    if family[0] == "f":
        ids = np.flatnonzero(rng.random(n) < float(family[1:]) / 100.0)
        assert ids.size > 0
        return H.words_of(ids, n)
    if family == "lt-k":       # fewer allowed rows than k
        return H.words_of(np.unique(np.linspace(0, n - 1, max(1, k // 2)).astype(np.int64)), n)
    if family == "one":
        return H.words_of([n // 3], n)
    if family == "none":
        return H.words_of([], n)
    if family == "cap0":       # a word of stray bits, capacity 0
        return np.full(1, np.uint64(0xFFFFFFFFFFFFFFFF)), 0
    if family == "cap-short":  # every bit of every word set, the garbage past the capacity in the last word included
        cap = n // 2 + 7
        return np.full(-(-cap // 64), np.uint64(0xFFFFFFFFFFFFFFFF)), cap
    if family == "head":
        return H.words_of(np.arange(n // 8), n)
    if family == "tail":
        return H.words_of(np.arange(n - n // 8, n), n)
    s = np.zeros(n, bool)
    s[sampled] = True
    if family == "sampled":    # only the rows the sample pass reads
        return H.words_of(np.flatnonzero(s), n)
    assert family == "unsampled" and rs >= 2   # none of them: no bound from the sample
    return H.words_of(np.flatnonzero(~s), n)


def families_for(n, names=FAMILIES):
    return [f for f in names if f != "unsampled" or sample_stride(n) >= 2]


def set_mech(monkeypatch, value):
    monkeypatch.delenv("SCANN_HIP_BF_FILTER_COMPACT_MAX", raising=False)
    if value is None:
        monkeypatch.delenv("SCANN_HIP_BF_FILTER", raising=False)
    else:
        monkeypatch.setenv("SCANN_HIP_BF_FILTER", value)


class F32:
    def __init__(self, measure, n, dim, nq, seed, rows=None):
        self.measure, self.n, self.dim = measure, n, dim
        self.rows = (synth.uniform_f32(n, dim, seed) * np.float32(2) - np.float32(1)) if rows is None else rows
        self.q = synth.uniform_f32(nq, dim, seed + 1) * np.float32(2) - np.float32(1)
        self.data, self.stride = orc.to_strided(self.rows)
        self.index = hip.bf_create(self.data, n, dim, self.stride, measure)
        self.index.enable_timing(True)

    def expected(self, allowed, q, k):
        """the unfiltered oracle over the allowed rows alone, indices mapped back"""
        if allowed.size == 0:
            z = np.zeros((q.shape[0], 0))
            return z.astype(np.uint32), z.astype(np.float32), np.zeros(q.shape[0], np.uint32)
        sub, st = orc.to_strided(self.rows[allowed])
        oi, od, oc = orc.bf_search_batched(sub, allowed.size, self.dim, st, self.measure, q, k)
        return allowed[oi.astype(np.int64)].astype(np.uint32), od, oc


class Quant:
    def __init__(self, fmt, measure, n, dim, nq, seed):
        self.fmt, self.measure, self.n, self.dim = fmt, measure, n, dim
        self.rows, self.inv = make_rows(fmt, n, dim, dim, seed)
        self.q = synth.uniform_f32(nq, dim, seed + 1)
        self.index = hip.bf_create_quantized(self.rows, n, dim, dim, fmt, measure, self.inv)
        self.index.enable_timing(True)
        self._d = qc.distances(self.q, self.rows, dim, fmt, measure, self.inv)

    def expected(self, allowed, q, k):
        nq = q.shape[0]
        kk = min(k, allowed.size)
        oi = np.zeros((nq, kk), np.uint32); od = np.zeros((nq, kk), np.float32)
        for i in range(nq):
            if kk:
                ti, td = orc.topk_run(kk, np.arange(allowed.size, dtype=np.uint32), self._d[i, allowed])
                oi[i], od[i] = allowed[ti.astype(np.int64)], td
        return oi, od, np.full(nq, kk, np.uint32)


def check_rows(got, want, allowed, k, what):
    """count = min(k, allowed rows); rows = the oracle's over the allowed subset (distances bitwise, indices up to
    exact ties); every index allowed; slots past the count padded."""
    idx, dist, cnt = got
    oi, od, oc = want
    m = min(k, allowed.size)
    aset = set(allowed.tolist())
    for i in range(idx.shape[0]):
        assert cnt[i] == m, "%s q%d: count %d, want %d" % (what, i, cnt[i], m)
        assert all(int(j) in aset for j in idx[i, :m]), "%s q%d: a disallowed index came back" % (what, i)
        assert same(dist[i, :m], od[i, :m]), "%s q%d: distances" % (what, i)
        H.assert_topk_equal_up_to_ties(idx[i, :m], dist[i, :m], oi[i, :m], od[i, :m], what="%s q%d" % (what, i))
        assert np.all(idx[i, m:] == 0xFFFFFFFF) and np.all(np.isinf(dist[i, m:])), "%s q%d: padding" % (what, i)


def run_families(case, nq, k, families, monkeypatch, kernel=None, mechs=MECHS):
    q = case.q[:nq]
    for fam in families:
        words, cap = allow_of(fam, case.n, k)
        allowed = H.allowed_ids(words, cap, case.n)
        assert (allowed.size == 0) == (fam in EMPTY)
        want = case.expected(allowed, q, k)
        for name, value in mechs:
            set_mech(monkeypatch, value)
            what = "%s n%d dim%d m%d nq%d k%d %s" % (fam, case.n, case.dim, case.measure, nq, k, name)
            got = case.index.search_batched(q, k, allow=words, allow_bits=cap)
            if kernel and allowed.size:
                assert case.index.last_kernel_ms()[1] == kernel, what
            check_rows(got, want, allowed, k, what)


@pytest.fixture
def no_small(monkeypatch):
    monkeypatch.setenv("SCANN_HIP_SMALL", "0")


# ---- 1. every kernel family x both plans x both mechanisms x the filter families ------------------------------
@pytest.mark.parametrize("n", [N_DIRECT, N_BIG])
def test_generic_kernel_every_family(n, no_small, monkeypatch):
    case = F32(SQL2, n, 50, 64, 11)
    run_families(case, 64, 10, families_for(n), monkeypatch, kernel="bf_generic_kernel")


@pytest.mark.parametrize("n", [N_DIRECT, N_BIG])
@pytest.mark.parametrize("measure", [L1, COS])
def test_l1_and_cosine(measure, n, no_small, monkeypatch):
    case = F32(measure, n, 40, 20, 12)
    run_families(case, 20, 10, families_for(n, FEW + ("all", "one")), monkeypatch, kernel="bf_generic_kernel")


@pytest.mark.parametrize("n", [N_DIRECT, N_BIG])
@pytest.mark.parametrize("measure", [SQL2, DOT])
def test_stream_kernel_every_family(measure, n, no_small, monkeypatch):
    case = F32(measure, n, 128, 3, 13)
    run_families(case, 3, 10, families_for(n), monkeypatch, kernel="bf_stream_kernel")
    run_families(case, 1, 10, families_for(n, FEW), monkeypatch, kernel="bf_stream_kernel")


@pytest.mark.parametrize("n", [N_DIRECT, N_BIG])
@pytest.mark.parametrize("dim", [32, 64, 96, 128])
@pytest.mark.parametrize("measure", [SQL2, L2])
def test_vq_kernel(measure, dim, n, no_small, monkeypatch):
    case = F32(measure, n, dim, 130, 14 + dim)
    fams = families_for(n) if dim == 128 and measure == SQL2 else families_for(n, FEW)
    run_families(case, 130, 10, fams, monkeypatch, kernel="bf_vq_kernel")


@pytest.mark.parametrize("n", [N_DIRECT, N_BIG])
@pytest.mark.parametrize("dim", [32, 64, 96, 128, 192, 256])
def test_mfma_dot_kernel(dim, n, no_small, monkeypatch):
    case = F32(DOT, n, dim, 70, 15 + dim)
    fams = families_for(n) if dim == 128 else families_for(n, FEW)
    run_families(case, 70, 10, fams, monkeypatch, kernel="bf_mfma_dot_kernel")


@pytest.mark.parametrize("n", [N_DIRECT, N_BIG])
@pytest.mark.parametrize("fmt", [hip.ROWS_BF16, hip.ROWS_FP8_E4M3, hip.ROWS_INT8])
@pytest.mark.parametrize("measure", [SQL2, DOT])
def test_quantized_rows(measure, fmt, n, no_small, monkeypatch):
    case = Quant(fmt, measure, n, 64, 20, 16 + fmt)
    fams = families_for(n) if fmt == hip.ROWS_INT8 else families_for(n, FEW + ("all", "none"))
    run_families(case, 20, 10, fams, monkeypatch, kernel="bf_quant_kernel")
    run_families(case, 2, 10, families_for(n, FEW), monkeypatch, kernel="bf_quant_kernel")   # the two-query form


# ---- 2. batch sizes, the few-query host pipeline, all-allowed = unfiltered -------------------------------------
@pytest.mark.parametrize("measure", [SQL2, DOT])
def test_batch_sizes(measure, no_small, monkeypatch):
    case = F32(measure, N_BIG, 128, 1024, 21)
    for nq in (1, 3, 64, 1024):
        run_families(case, nq, 10, ("f50", "f10", "f1", "unsampled"), monkeypatch)


@pytest.mark.parametrize("n", [N_DIRECT, N_BIG])
@pytest.mark.parametrize("measure", [SQL2, DOT, COS])
def test_small_batch_host_pipeline(measure, n, monkeypatch):
    """SCANN_HIP_SMALL unset: up to 16 queries with k <= 64 take bf_small_search_host, which applies the bit test
    in its scan (the mechanism knob does not apply to it)."""
    monkeypatch.delenv("SCANN_HIP_SMALL", raising=False)
    case = F32(measure, n, 96, 16, 22)
    for nq in (1, 3, 16):
        run_families(case, nq, 10, families_for(n), monkeypatch, mechs=MECHS[:1])


@pytest.mark.parametrize("nq", [3, 64, 1024])
@pytest.mark.parametrize("measure", [SQL2, DOT])
def test_all_allowed_equals_unfiltered_bitwise(measure, nq, no_small, monkeypatch):
    case = F32(measure, N_BIG, 128, nq, 23)
    ref = case.index.search_batched(case.q, 10)
    words, cap = allow_of("all", case.n, 10)
    for name, value in MECHS:
        set_mech(monkeypatch, value)
        got = case.index.search_batched(case.q, 10, allow=words, allow_bits=cap)
        assert np.array_equal(got[0], ref[0]) and same(got[1], ref[1]) and np.array_equal(got[2], ref[2]), name


# ---- 3. the shortlist regime: filtered calls are routed to the exact kernels -----------------------------------
@pytest.mark.parametrize("measure", [SQL2, DOT])
def test_shortlist_regime_routes_filtered_calls_to_exact_kernels(measure, monkeypatch):
    monkeypatch.setenv("SCANN_HIP_BF_SHORTLIST_MIN_ROWS", "1")
    monkeypatch.setenv("SCANN_HIP_BF_SHORTLIST_MIN_QUERIES", "1")
    monkeypatch.setenv("SCANN_HIP_SMALL", "0")
    case = F32(measure, N_BIG, 128, 64, 24)
    case.index.search_batched(case.q, 10)
    assert case.index.last_kernel_ms()[1] == "bf_bf16_kernel"     # the unfiltered batch takes the shortlist
    exact = "bf_mfma_dot_kernel" if measure == DOT else "bf_generic_kernel"
    run_families(case, 64, 10, ("all", "f50", "f1", "lt-k", "unsampled"), monkeypatch, kernel=exact)
    case.index.search_batched(case.q, 10)
    assert case.index.last_kernel_ms()[1] == "bf_bf16_kernel"


# ---- 4. ties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [N_DIRECT, N_BIG])
@pytest.mark.parametrize("measure", [SQL2, DOT])
def test_ties_between_allowed_and_disallowed_copies(measure, n, no_small, monkeypatch):
    """8 prototype rows repeated: thousands of rows tie at every distance.  With rows i % 3 == 0 disallowed, the k
    best are the LOWEST allowed copies of the nearest prototype -- no disallowed copy appears or displaces one."""
    dim, k = 64, 10
    protos = synth.uniform_f32(8, dim, 31) * np.float32(2) - np.float32(1)
    rows = np.ascontiguousarray(protos[np.arange(n) % 8])
    case = F32(measure, n, dim, 24, 32, rows=rows)
    case.q[:8] = protos
    ids = np.flatnonzero(np.arange(n) % 3 != 0)
    words, cap = H.words_of(ids, n)
    want = case.expected(ids, case.q, k)
    for nq in (3, 24):
        for name, value in MECHS:
            set_mech(monkeypatch, value)
            idx, dist, cnt = case.index.search_batched(case.q[:nq], k, allow=words, allow_bits=cap)
            check_rows((idx, dist, cnt), tuple(w[:nq] for w in want), ids, k, "ties nq%d %s" % (nq, name))
            for i in range(nq):   # (distance, index) order over the allowed rows: the lowest allowed copies win
                d = orc.one_to_many(case.q[i], case.data, case.stride, n, measure)
                b = d.view(np.uint32)
                key = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))[ids]
                order = ids[np.lexsort((ids, key))[:k]]
                assert np.array_equal(idx[i].astype(np.int64), order), "ties nq%d %s q%d" % (nq, name, i)


# ---- 5. entry points -------------------------------------------------------------------------------------------
def test_params_entry_with_mixed_k(no_small, monkeypatch):
    case = F32(SQL2, N_BIG, 64, 12, 41)
    ks = np.array([1, 10, 3, 10, 100, 1, 3, 100, 10, 7, 7, 2048], np.uint32)
    for fam in ("f10", "lt-k", "none"):
        words, cap = allow_of(fam, case.n, 10)
        allowed = H.allowed_ids(words, cap, case.n)
        for name, value in MECHS:
            set_mech(monkeypatch, value)
            idx, dist, cnt = case.index.search_batched_with_params(case.q, ks, allow=words, allow_bits=cap)
            for i, k in enumerate(ks):
                want = case.expected(allowed, case.q[i:i + 1], int(k))
                check_rows((idx[i:i + 1, :k], dist[i:i + 1, :k], cnt[i:i + 1]), want, allowed, int(k),
                           "params %s %s q%d" % (fam, name, i))
                assert np.all(idx[i, k:] == 0xFFFFFFFF)


def _device_call(index, q, k, words, cap, reserve=True):
    """reserve + a filtered scann_hip_search_batched_device on torch's stream.  Returns (status, idx, dist, count,
    free bytes before the call, free bytes after it): the library allocates with hipMalloc, which the device's free
    memory shows; every torch tensor is made before the first reading."""
    import torch
    dev = torch.device("cuda:0")
    L = hip.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    nq, dim = q.shape
    qd = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(dev)
    oi = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
    od = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    oc = torch.full((nq,), 7, dtype=torch.int32, device=dev)
    o = hip.default_opts()
    da = None
    if words is not None:
        da = torch.from_numpy(np.ascontiguousarray(words, np.uint64).view(np.int64).copy()).to(dev)
        o.allow_bitmap = ctypes.cast(ctypes.c_void_p(da.data_ptr()), ctypes.POINTER(ctypes.c_uint64))
        o.allow_bitmap_bits = int(cap)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if reserve:
        hip.check(L.scann_hip_index_reserve(index.h, nq, k, ctypes.byref(o)))
        # a call of half the batch first: the runtime's own first-launch allocations (code, events) happen here, while
        # the full batch below still needs every byte that reserve sized for it
        hip.check(L.scann_hip_search_batched_device(index.h, p(qd), max(1, nq // 2), dim, k, ctypes.byref(o), p(oi), p(od),
                                                    p(oc), st))
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(dev)[0]
    hip.check(L.scann_hip_search_batched_device(index.h, p(qd), nq, dim, k, ctypes.byref(o), p(oi), p(od), p(oc), st))
    status = L.scann_hip_index_last_device_status(index.h, st)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(dev)[0]
    return status, oi.cpu().numpy().view(np.uint32), od.cpu().numpy(), oc.cpu().numpy().view(np.uint32), free0, free1


@pytest.mark.parametrize("n", [N_DIRECT, N_BIG])
@pytest.mark.parametrize("measure", [SQL2, DOT])
def test_device_entry_after_reserve(measure, n, no_small, monkeypatch):
    """The device entry with a device bitmap: Ok with the oracle's rows, and no allocation after reserve.  The one
    documented failure (scann_hip_index_last_device_status): the bit test's bound comes from the allowed rows of the
    8192-row sample (rows j * rs); a filter that leaves fewer than k of them ("unsampled"; "tail", whose rows lie past
    the last sampled one) gives no bound, and with more allowed rows than the candidate buffer sized from k holds
    (2 k rs + 16 rs + 256) -> ResourceExhausted, every query's count 0, never wrong rows; the host entry answers the
    same call exactly."""
    case = F32(measure, n, 128, 64, 51)
    k = 10
    rs = sample_stride(n)
    failing = []
    for fam in families_for(n):
        words, cap = allow_of(fam, n, k)
        allowed = H.allowed_ids(words, cap, n)
        want = case.expected(allowed, case.q, k)
        status, idx, dist, cnt, free0, free1 = _device_call(case.index, case.q, k, words, cap)
        what = "device %s n%d m%d" % (fam, n, measure)
        assert free1 == free0, "%s: the call allocated %d bytes" % (what, free0 - free1)
        in_sample = np.count_nonzero((allowed % rs == 0) & (allowed // rs < SAMPLE))
        if n > SAMPLE and in_sample < k and allowed.size > min(n, 2 * k * rs + 16 * rs + 256):
            failing.append(fam)
            assert status == hip.RESOURCE_EXHAUSTED, what
            assert np.all(cnt == 0), what
            check_rows(case.index.search_batched(case.q, k, allow=words, allow_bits=cap), want, allowed, k, what + " host")
            continue
        assert status == hip.OK, "%s: status %d" % (what, status)
        check_rows((idx, dist, cnt), want, allowed, k, what)
    assert failing == (["tail", "unsampled"] if n > SAMPLE else [])


@pytest.mark.parametrize("n", [N_DIRECT, N_BIG])
@pytest.mark.parametrize("kind", ["f32-sql2", "f32-dot", "f32-cos", "int8-sql2"])
def test_radius_search_with_a_filter(kind, n, monkeypatch):
    dim = 32
    if kind == "int8-sql2":
        case = Quant(hip.ROWS_INT8, SQL2, n, dim, 2, 61)
    else:
        case = F32({"f32-sql2": SQL2, "f32-dot": DOT, "f32-cos": COS}[kind], n, dim, 2, 61)
    for fam in families_for(n, ("all", "f50", "f1", "one", "none", "cap0", "cap-short", "tail")):
        words, cap = allow_of(fam, n, 10)
        allowed = H.allowed_ids(words, cap, n)
        for qi in range(2):
            if kind == "int8-sql2":
                d = case._d[qi, allowed]
            else:
                sub, st = orc.to_strided(case.rows[allowed]) if allowed.size else (np.zeros((0, dim), np.float32), dim)
                d = orc.one_to_many(case.q[qi], sub, st, allowed.size, case.measure) if allowed.size else np.zeros(0, np.float32)
            radius = float(np.sort(d)[min(d.size - 1, 40)]) if d.size else 1.0
            if kind == "int8-sql2":
                keep = np.flatnonzero(d <= np.float32(radius))
                order = keep[np.argsort(d[keep], kind="stable")]
                oi, od = allowed[order].astype(np.uint32), d[order]
            elif allowed.size:
                ri, od = orc.bf_search_radius(sub, allowed.size, dim, st, case.measure, case.q[qi], radius)
                oi = allowed[ri.astype(np.int64)].astype(np.uint32)
            else:
                oi, od = np.zeros(0, np.uint32), np.zeros(0, np.float32)
            for name, value in MECHS:
                set_mech(monkeypatch, value)
                what = "radius %s %s n%d q%d %s" % (kind, fam, n, qi, name)
                gi, gd, found = case.index.search_radius(case.q[qi], radius, allow=words, allow_bits=cap)
                assert found == oi.size == gi.size, what
                assert same(gd, od), what
                assert set(gi.tolist()) <= set(allowed.tolist()), what
                H.assert_topk_equal_up_to_ties(gi, gd, oi, od, what=what)
        # the old symbol and a null bitmap: unfiltered
        a = hip.bf_search_radius(case.index, case.q[0], radius)
        b = case.index.search_radius(case.q[0], radius)
        assert np.array_equal(a[0], b[0]) and same(a[1], b[1]) and a[2] == b[2]


# ---- 6. state hygiene ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small", ["0", None])
@pytest.mark.parametrize("nq", [3, 64])
def test_filter_does_not_stick(nq, small, monkeypatch):
    """a filtered call followed by an unfiltered one on the same handle (and, device entry, stream): the unfiltered
    answer of a fresh handle.  A null bitmap must not inherit the previous call's."""
    if small is None:
        monkeypatch.delenv("SCANN_HIP_SMALL", raising=False)
    else:
        monkeypatch.setenv("SCANN_HIP_SMALL", small)
    case = F32(SQL2, N_BIG, 64, nq, 71)
    fresh = hip.bf_create(case.data, case.n, case.dim, case.stride, SQL2).search_batched(case.q, 10)
    for fam in ("f1", "none", "cap0"):
        words, cap = allow_of(fam, case.n, 10)
        for name, value in MECHS:
            set_mech(monkeypatch, value)
            case.index.search_batched(case.q, 10, allow=words, allow_bits=cap)
            got = case.index.search_batched(case.q, 10)
            assert np.array_equal(got[0], fresh[0]) and same(got[1], fresh[1]) and np.array_equal(got[2], fresh[2]), \
                "%s %s" % (fam, name)
        _device_call(case.index, case.q, 10, words, cap)
        status, idx, dist, cnt, _, _ = _device_call(case.index, case.q, 10, None, 0, reserve=False)
        assert status == hip.OK
        assert np.array_equal(idx, fresh[0]) and same(dist, fresh[1]) and np.array_equal(cnt, fresh[2]), fam


# ---- 7. the headline size --------------------------------------------------------------------------------------
def test_headline_1m_x_128_under_a_5_percent_filter(monkeypatch):
    """1M x 128, 1024 queries, a 5 % uniform filter, the default path of the host entry; sampled queries against the
    oracle on the allowed subset, every query's distances against exact re-computation of its rows."""
    for name in ("SCANN_HIP_BF_FILTER", "SCANN_HIP_BF_FILTER_COMPACT_MAX", "SCANN_HIP_SMALL",
                 "SCANN_HIP_BF_SHORTLIST_MIN_ROWS", "SCANN_HIP_BF_SHORTLIST_MIN_QUERIES"):
        monkeypatch.delenv(name, raising=False)
    n, dim, nq, k = 1_000_000, 128, 1024, 10
    rows = synth.uniform_f32(n, dim, 42)
    q = synth.uniform_f32(nq, dim, 123)
    data, stride = orc.to_strided(rows)
    ids = np.flatnonzero(np.random.default_rng(7).random(n) < 0.05)
    words, cap = H.words_of(ids, n)
    sub, st = orc.to_strided(rows[ids])
    aset = np.zeros(n, bool)
    aset[ids] = True
    for measure in (SQL2, DOT):
        index = hip.bf_create(data, n, dim, stride, measure)
        idx, dist, cnt = index.search_batched(q, k, allow=words, allow_bits=cap)
        assert np.all(cnt == k) and aset[idx.astype(np.int64)].all()
        sel = np.arange(0, nq, 64)
        oi, od, oc = orc.bf_search_batched(sub, ids.size, dim, st, measure, q[sel], k)
        for j, i in enumerate(sel):
            assert same(dist[i], od[j]), "m%d q%d" % (measure, i)
            H.assert_topk_equal_up_to_ties(idx[i], dist[i], ids[oi[j].astype(np.int64)], od[j], what="m%d q%d" % (measure, i))
        for i in range(0, nq, 7):
            want = orc.one_to_many(q[i], data[idx[i].astype(np.int64)].ravel(), stride, k, measure)
            assert same(dist[i], want), "m%d q%d recompute" % (measure, i)


# ---- 8. the C++ mirror -----------------------------------------------------------------------------------------
def test_cpp_mirror_search_with_filter():
    """BruteForceSearcher::search_with_filter / search_radius_with_filter (scann.hpp) with a RestrictDenylist on the
    5-point cube set of brute_force/searcher.rs:280-376: the excluded exact match does not come back, counts right."""
    import os
    import subprocess
    from scann_rust_amd import build
    build.build_host()
    exe = os.path.join(os.path.dirname(os.path.abspath(build.__file__)), "host", "bf_filter_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bf_filter_test ok" in r.stdout

"""The cases of tests/test_gpu_partition_front.py -- the front end of every tree search (centroid scores, leaf
selection, work lists) at thousands of leaves and probes -- and a mirror of the launcher rules that decide what such a
case runs.  Pure Python and numpy: no GPU and no library.  tests/test_partition_cases.py holds the table to hitting
both sides of every switch.

Every rule below restates one place of the library, named beside it; DESIGN.md "Limits" carries the same arithmetic."""
import collections

import numpy as np

# csrc/launch.h kMaxLdsBytes; csrc/txh.h kMaxLeavesSelect, kMaxPartitionsToSearch, kSelectThreads, kDecodeStage,
# kSmallBatch, kSmallMaxCandidates, kSmallMaxStream, kWideBatch, kWideMaxCandidates, kWideMaxStream, kFusedChunk,
# kFusedMaxWgs; csrc/txh_prefilter.hip kRefineTablesMax; csrc/txh.hip kSelRegCaps
LDS_MAX = 160 * 1024
MAX_LEAVES, MAX_P = 16384, 4096
SELECT_THREADS, DECODE_STAGE, REFINE_TABLES_MAX = 1024, 512, 40
SMALL_BATCH, SMALL_MAX_CANDIDATES, SMALL_MAX_STREAM = 16, 1024, 262144
WIDE_BATCH, WIDE_MAX_CANDIDATES, WIDE_MAX_STREAM = 4, 8192, 4 << 20
FUSED_CHUNK, FUSED_MAX_WGS = 1024, 512
SEL_REG_CAP = 18432
SELECT_STATIC = 0           # select_leaves_kernel has no __shared__ array of its own (hipFuncGetAttributes: 0 bytes)
INLINE_MAX_LEAVES = 4096    # api_create.hip / api_search.hip: the transposed centroid copy (centers_t) and the Small / Wide pipelines
NQ = 33                     # queries of a partition case: no multiple of centroid_scores_kernel's 4- or 16-query tile
K = 10

Case = collections.namedtuple("Case", "name L P dim centroids queries leaves avg fix")
Search = collections.namedtuple("Search", "name L P dim nq mode leaves avg ms wide")


def next_pow2(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def sel_cfg(n):
    """csrc/common.h sel_cfg: (histogram bins, exact-rank list) of block_select"""
    return (1024, 256) if n <= 4096 else (4096, 1024)


def select_lds(L, p2):
    """csrc/txh.hip launch_partition_stage, lds_of: the keys, the select path's survivors, block_select's tables, its
    reduction words and the scan words"""
    bins, lst = sel_cfg(L)
    return (next_pow2(L) + p2) * 8 + bins * 4 + lst * 8 + 48 * 8 + 64 * 4


def wants_select(L, P):
    """csrc/txh.hip launch_partition_stage / launch_search_small: rank-select the P-th key and sort P keys when
    4 P <= next_pow2(L), else sort all next_pow2(L) keys"""
    return 4 * P <= next_pow2(L)


def wanted_lds(L, P):
    """what the select path asks for where the rule above picks it (the parent of the fix launched exactly this)"""
    return select_lds(L, next_pow2(max(1, P)) if wants_select(L, P) else 0)


def staged_select(L, P):
    """csrc/txh.hip launch_partition_stage: (p2, threads, LDS bytes) of select_leaves_kernel behind
    centroid_scores_kernel.  The select path is dropped where its request, plus the kernel's static LDS, passes the
    CU's 160 KB: that happens only above 8192 leaves with more than 512 partitions."""
    p2 = next_pow2(max(1, P)) if wants_select(L, P) else 0
    if p2 and select_lds(L, p2) + SELECT_STATIC > LDS_MAX:
        p2 = 0
    return p2, (256 if p2 and L <= 4096 else SELECT_THREADS), select_lds(L, p2)


def pipeline(L, P, nq, m, ms, wide=False, exact_scan=False, sharded=False, k=K):
    """csrc/api_search.hip plan_txh_search: Staged, Small (at most 16 queries) or Wide (at most 4, where SCANN_HIP_WIDE=2
    forces it).  ms: the longest stream, the sum of the P largest leaves."""
    pipe = "Staged"
    if nq <= SMALL_BATCH and not sharded and m <= SMALL_MAX_CANDIDATES and k <= 64 and ms <= SMALL_MAX_STREAM and \
            L <= INLINE_MAX_LEAVES:
        pipe = "Small"
    if wide and nq <= WIDE_BATCH and not sharded and 1 <= m <= WIDE_MAX_CANDIDATES and k <= 64 and \
            ms <= WIDE_MAX_STREAM and L <= INLINE_MAX_LEAVES and P <= DECODE_STAGE and not exact_scan:
        pipe = "Wide"
    return pipe


def small_fused(P, nq, ms, exact_scan):
    """csrc/api_search.hip plan_small_launch: the Small pipeline as one launch (small_fused_kernel) or three"""
    chunk = FUSED_CHUNK
    if exact_scan:
        chunk = min(FUSED_CHUNK, max(128, (-(-ms // 256) + 127) & ~127))
    grid = max(1, -(-ms // chunk))
    return P <= DECODE_STAGE and nq * grid <= FUSED_MAX_WGS and (exact_scan or P == 1)


def plan_cap(ms, P, m):
    """csrc/api_search.hip plan_txh_search: the candidate list of the staged pipeline's first attempt (tests/helpers.py
    plan_caps has the same arithmetic; repeated here so that this module imports no library)"""
    ns = min(max(ms // 16, 4096), 32768)
    st = max(1, -(-ms // ns))
    while ((-(-ms // st) + P) + 3) & ~3 > 32768:
        st += 1 + st // 8
    r = np.float32(m) / np.float32(st)
    s = np.float32(0.5) * (np.float32(6.0) + np.sqrt(np.float32(36.0) + np.float32(4.0) * r, dtype=np.float32))
    jp = s * s + np.float32(2.0)
    j = max(1, min(m if jp >= np.float32(m) else int(jp), m))
    return min(max(int(j + 8.0 * np.sqrt(j) + 16.0) * st + 256, m), ms)


def final_select(ms, P, m, stages):
    """csrc/txh.hip launch_select: which kernel decodes the m survivors through the key bases of the P leaves.
    stages=True asks for sorted candidates, so the unsorted forms are out; without it a list of more than 4096 keys is
    selected from registers (select_regs_kernel), a shorter one in LDS (select_rerank_kernel)."""
    cap = plan_cap(ms, P, m)
    if not stages and next_pow2(max(cap, 64)) > 4096 and cap <= SEL_REG_CAP:
        return "select_regs_kernel"
    return "select_rerank_kernel"


def classify(L, P, dim, nq, m=K, ms=1, wide=False, exact_scan=False, sharded=False):
    """every switch of the front end a call of this shape passes, as a dict of classes"""
    assert 1 <= L <= MAX_LEAVES and 1 <= P <= MAX_P
    P = min(P, L)
    pipe = pipeline(L, P, nq, m, ms, wide, exact_scan, sharded)
    if pipe == "Staged":
        p2, threads, lds = staged_select(L, P)
        inline = False
    else:
        # csrc/txh.hip launch_search_small: always kSelectThreads; the leaf size tables and the query behind the keys
        p2 = next_pow2(max(1, P)) if wants_select(L, P) else 0
        threads, inline = SELECT_THREADS, True
        lds = select_lds(L, p2) + L * 8 + ((dim + 3) & ~3) * 4 + 16
    out = {
        "pipeline": pipe,
        "threads": threads,
        "select": "select" if p2 else "full-sort",
        "per": -(-P // threads),                                # select_leaves_body: tokens per thread of the prefix sums
        "per>1": -(-P // threads) > 1,
        "sel_cfg": "small" if L <= 4096 else "large",
        "scoring": "inline" if inline else "kernel",
        # centroid_scores_kernel (txh_partition.hip): float4 loads when dim % 4 == 0
        "centroid-path": None if inline else ("float4" if dim % 4 == 0 else "scalar"),
        # select_leaves_body's inline scoring: 64-dim chunks, the last one guarded by j0 + u < dim
        "inline-chunks": None if not inline else ("whole" if dim % 64 == 0 else "tail"),
        "decode": "staged" if P <= DECODE_STAGE else "global",   # kDecodeStage: key bases in LDS or read from global memory
        "refine-tables": P <= REFINE_TABLES_MAX,
        "fused": pipe == "Small" and small_fused(P, nq, ms, exact_scan),
        # worklist_scan_kernel: one block of 1024 threads over the L leaves
        "worklist-leaves-per-thread": None if pipe != "Staged" else ("one" if L <= 1024 else "many"),
        "lds": lds,
        "lds-wanted": wanted_lds(L, P) if pipe == "Staged" else lds,
    }
    return out


# ---- the partition cases: hip.txh_partition against orc.partition, NQ queries ------------------------------------------
# centroids: uniform | dup4 (every centroid four times, at scattered ids: exact ties) | identical (every key ties)
# queries:   uniform | edges (uniform, with one query equal to a centroid, one with a component of 3e19 -- every distance
#            +inf -- and one holding a NaN)
# leaves:    uniform | half-empty | skewed (leaf_sizes below); avg: rows per leaf
# fix:       the select path's request passes 160 KB: the parent refused these with RESOURCE_EXHAUSTED
CASES = (
    Case("4096x1000", 4096, 1000, 16, "uniform", "edges", "uniform", 3, False),
    Case("2500x700", 2500, 700, 16, "dup4", "edges", "half-empty", 3, False),
    Case("3000x1500", 3000, 1500, 16, "uniform", "edges", "skewed", 3, False),
    Case("4096x4096", 4096, 4096, 16, "identical", "edges", "uniform", 3, False),
    Case("4097x10", 4097, 10, 16, "dup4", "edges", "uniform", 3, False),
    Case("5000x2048", 5000, 2048, 16, "uniform", "edges", "half-empty", 3, False),
    Case("5000x2049", 5000, 2049, 16, "dup4", "edges", "uniform", 3, False),
    Case("8192x600", 8192, 600, 16, "identical", "edges", "skewed", 2, False),
    Case("8193x512", 8193, 512, 16, "uniform", "edges", "uniform", 2, False),
    Case("8193x513", 8193, 513, 16, "dup4", "edges", "uniform", 2, True),
    Case("16384x1", 16384, 1, 16, "uniform", "edges", "uniform", 2, False),
    Case("16384x4096", 16384, 4096, 16, "dup4", "edges", "half-empty", 2, True),
    # the scalar path of centroid_scores_kernel, and the small shapes the suite had (one leaf per thread everywhere)
    Case("1500x200-dim19", 1500, 200, 19, "uniform", "edges", "uniform", 3, False),
    Case("1500x200-dim6", 1500, 200, 6, "dup4", "edges", "uniform", 3, False),
    Case("1000x50", 1000, 50, 16, "uniform", "uniform", "uniform", 3, False),
)

# ---- the search cases: search_batched(stages=True) stage by stage against the oracle -----------------------------------
# mode: txh (S = 8, K = 16: LUT16) | bytes (S = 4, K = 32: byte codes, for a dim no LUT16 layout admits) |
#       partitioned (no codes: the leaves' rows scored exactly)
# ms:   the pre_reorder_k values; wide: SCANN_HIP_WIDE=2
SEARCHES = (
    Search("staged-5000x600", 5000, 600, 16, 33, "txh", "uniform", 6, (300, 3500), False),
    Search("small-4096x600", 4096, 600, 16, 8, "txh", "half-empty", 6, (300,), False),
    Search("small-4096x300", 4096, 300, 16, 8, "txh", "skewed", 3, (300,), False),
    Search("wide-4096x300", 4096, 300, 16, 2, "txh", "skewed", 3, (300,), True),
    Search("small-4096x300-dim64", 4096, 300, 64, 8, "txh", "uniform", 3, (300,), False),
    Search("small-4096x300-dim65", 4096, 300, 65, 8, "partitioned", "half-empty", 3, (K,), False),
    Search("small-4096x300-dim100", 4096, 300, 100, 8, "bytes", "uniform", 3, (300,), False),
    Search("wide-4096x300-dim64", 4096, 300, 64, 2, "txh", "uniform", 3, (300,), True),
    Search("wide-4096x300-dim100", 4096, 300, 100, 2, "bytes", "uniform", 3, (300,), True),
    Search("staged-16384x512", 16384, 512, 16, 33, "txh", "uniform", 2, (300,), False),
    Search("staged-16384x4096", 16384, 4096, 16, 5, "txh", "half-empty", 2, (300,), False),
)
# two leaf shards: the key bases are summed from the GLOBAL leaf sizes, which differ from the local ones.  5000 x 600
# runs 1024 threads, one token per thread; 4096 x 1000 runs 256 threads with four tokens each, so that a thread's own
# running sum and the carries of the waves before it all come from leaf_gsize
SHARDED = (Search("sharded-5000x600", 5000, 600, 16, 33, "txh", "uniform", 3, (60,), False),
           Search("sharded-4096x1000", 4096, 1000, 16, 33, "txh", "half-empty", 3, (60,), False))


# ---- synthetic indexes: centroids and an explicit assignment, no k-means -----------------------------------------------
def _rng(name, what):
    return np.random.default_rng([sum(name.encode()), len(name), what])


def leaf_sizes(name, L, family, avg):
    """[L] rows per leaf"""
    rng = _rng(name, 1)
    if family == "uniform":
        return rng.integers(1, 2 * avg, L).astype(np.int64)               # 1 .. 2 avg - 1
    if family == "half-empty":
        sizes = rng.integers(1, 4 * avg, L).astype(np.int64)
        sizes[rng.random(L) < 0.5] = 0
        sizes[0:4] = (0, 2 * avg, 0, 2 * avg)                             # an empty leaf beside a filled one, in id order
        sizes[L - 1] = 0
        return sizes
    assert family == "skewed"
    sizes = rng.integers(0, 4, L).astype(np.int64)                        # 0 .. 3
    sizes[L // 3] = max(1, (L * avg) // 4)                                # one leaf with a quarter of the rows
    return sizes


def max_stream(sizes, P):
    return int(np.sort(np.asarray(sizes, np.int64))[::-1][:P].sum())


def centroids(name, L, dim, family):
    rng = _rng(name, 2)
    if family == "uniform":
        return rng.random((L, dim), dtype=np.float32)
    if family == "identical":
        return np.repeat(rng.random((1, dim), dtype=np.float32), L, 0)
    assert family == "dup4"
    base = rng.random((-(-L // 4), dim), dtype=np.float32)
    out = np.empty((L, dim), np.float32)
    out[rng.permutation(L)] = np.tile(base, (4, 1))[:L]                   # copy j of base i lands at a scattered id
    return out


INF_QUERY, NAN_QUERY, HIT_QUERY = 7, 12, 3


def queries(name, nq, dim, family, centers):
    q = _rng(name, 3).random((nq, dim), dtype=np.float32)
    if family == "edges":
        q[HIT_QUERY] = centers[centers.shape[0] // 2]                     # distance +0.0 (four times over with dup4)
        q[INF_QUERY, dim // 2] = np.float32(3e19)                         # (3e19)^2 overflows: every distance +inf
        q[NAN_QUERY, 0] = np.nan
    return q


def rows_and_assign(name, centers, sizes, near=True):
    """rows in an order that mixes the leaves, and their leaf ids.  near: scattered closely about their leaf's centroid.
    Otherwise uniform over the cube whatever their leaf: then neither the approximate nor the exact distance of a row
    says anything about the rank of its leaf, so the candidates and the final rows of a query come from leaves of every
    rank -- every key base is used, not only those of the nearest leaves."""
    rng = _rng(name, 4)
    assign = rng.permutation(np.repeat(np.arange(centers.shape[0]), sizes))
    if near:
        rows = centers[assign] + rng.uniform(-0.05, 0.05, (assign.size, centers.shape[1])).astype(np.float32)
    else:
        rows = rng.random((assign.size, centers.shape[1]), dtype=np.float32)
    return np.ascontiguousarray(rows, np.float32), assign

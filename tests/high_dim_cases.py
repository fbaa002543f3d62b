"""Dimensionalities for tests/test_gpu_high_dim.py, derived from the LDS arithmetic of the kernels that run at
embedding-sized dims (no fast path takes dim > 256), and the shapes of the cases that use them.

Every formula below restates one launcher (named beside it) and is written once; DESIGN.md "Dimensionality ceilings"
carries the same table.  tests/test_high_dim_cases.py recomputes the byte counts and asserts that the dim lists straddle
every edge, so that the lists cannot drift away from the kernels silently.  No GPU is needed to import this module.

An edge is a pair (dim at the edge, next dim the kernel accepts) at which a launcher changes what it does:
  64 KB    launch.h set_dyn_lds sets the dynamic-LDS attribute only above 64 KB of dynamic LDS
  160 KB   the LDS of one compute unit: above it a launcher picks a smaller tile, another kernel, or refuses
  tile     the queries (or centres) per tile change
"""
import numpy as np

LDS_ATTR = 64 * 1024        # launch.h: no attribute at or below this
LDS_MAX = 160 * 1024        # launch.h kMaxLdsBytes
MUT_TILE = 1024             # mutable.h kMutTile / hip.MUTABLE_DELTA_TILE
EXACT_STATIC = 516          # leaf_exact_scan_kernel's static arrays: s_pq_all, s_vb_all (64 u32 each), tile_sh

COMMON = (768, 1024, 1536, 3072, 4096)
UNALIGNED = 1027            # no multiple of 4, run at stride == dim: scalar tails and the vec == false / qvec == false branches
ABOVE = 6144                # above the ceiling of every kernel that stages 8 f32 rows or more


def dimp(dim):
    return (dim + 3) & ~3


# ---- bytes of dynamic LDS per launcher ------------------------------------------------------------------------------
def stream_lds(dim):
    """bf.hip stream_lds_bytes: kStQT = 8 queries + 4 waves x 64 rows x 36 floats"""
    return 32 * dimp(dim) + 36864


def generic_lds(dim):
    """bf.hip generic_lds_bytes: kBfGenQT = 8 queries + 8 query norms"""
    return (8 * dimp(dim) + 8) * 4


def quant_qt(dim, nq):
    """bf.hip launch_quant_pass: one query pair for nq <= 2, four otherwise -- one where four exceed the LDS"""
    return 2 if nq <= 2 or 32 * dim > LDS_MAX else 8


def quant_lds(dim, nq):
    """bf.hip launch_quant: [dim][QT] floats"""
    return 4 * quant_qt(dim, nq) * dim


def exact_qpt(dim):
    """txh.hip exact_quads_per_tile"""
    q = (48 * 1024) // (dimp(dim) * 4) // 8 * 2
    return min(max(q, 2), 16)


def exact_lds(dim):
    """txh.hip exact_scan_lds_bytes: 4 qpt queries (plus EXACT_STATIC static bytes)"""
    return exact_qpt(dim) * 16 * dimp(dim)


def centroid_qt(dim, L, nq):
    """txh_partition.hip launch_centroid_scores: 16 queries per block on a full grid, if they fit"""
    waves16 = -(-L // 64) * -(-nq // 16)
    return 16 if waves16 >= 8192 and 16 * dim * 4 <= LDS_MAX else 4


def centroid_lds(dim, qt):
    return qt * dim * 4


def assign_tc(dim):
    """bf.hip launch_assign_nearest: 16 centres per tile, 8 where 16 do not fit"""
    return 16 if 16 * dimp(dim) * 4 <= LDS_MAX else 8


def assign_lds(dim):
    return assign_tc(dim) * dimp(dim) * 4


def assign_avx_lds(dim):
    """bf.hip km_launch_assign, AVX2 order: kAvxTC = 8 centres"""
    return 8 * dimp(dim) * 4


def delta_qt(dim):
    """mutable.hip delta_and_merge (before the clamp to nq)"""
    return max(1, min(8, (48 * 1024) // (4 * dimp(dim))))


def delta_lds(dim, nq=8):
    return MUT_TILE * 8 + min(delta_qt(dim), nq) * dimp(dim) * 4


def small_scan_lds(dim, S, kp):
    """txh.hip launch_search_small: the ADC tables and the query of the small-batch and wide pipelines"""
    return (S * kp + dim) * 4


def lut_build_lds(dim):
    """txh_partition.hip launch_lut_build: the residuals of a quad of queries (the batched tree / hasher search)"""
    return 4 * dim * 4


def lut_from_query_lds(dim):
    """txh_partition.hip txh_launch_lut_from_query: one query"""
    return dim * 4


def rerank_lds(dim):
    """txh.hip / txh_rows.hip: the query of rerank_kernel, rerank_i8_kernel and rerank_quant_kernel"""
    return dim * 4


def mmr_lds(dim, depth):
    """mmr.hip: one stored row and 13 bytes per entry of the row of results"""
    return dimp(dim) * 4 + depth * 13


# ---- kernel choice of a brute-force pass over f32 rows (bf.hip launch_pass; device rows are 16-byte aligned) ---------
DOT_FAMILY = (0, 1, 2)      # SquaredL2, L2, DotProduct


def bf_pass_kernel(measure, dim, stride, nq):
    if measure in DOT_FAMILY and stride % 4 == 0 and dim >= 8 and nq <= 16 and stream_lds(dim) <= LDS_MAX:
        return "bf_stream_kernel"
    assert dim > 256, "the MFMA and one-query-per-lane kernels are not mirrored here"
    return "bf_generic_kernel"


# ---- ceilings: the largest dim an entry point accepts, at every batch size ------------------------------------------
def _largest(fits, step=4, hi=1 << 16):
    d = 0
    while d + step <= hi and fits(d + step):
        d += step
    return d


CEILING = {
    "bf f32": _largest(lambda d: generic_lds(d) <= LDS_MAX),                          # 5116
    "bf quantized": _largest(lambda d: quant_lds(d, 2) <= LDS_MAX),                   # 20480
    "partitioned": _largest(lambda d: exact_lds(d) + EXACT_STATIC <= LDS_MAX),        # 5100
    "centroid scores": _largest(lambda d: centroid_lds(d, 4) <= LDS_MAX),             # 10240
    "assign nearest": _largest(lambda d: assign_lds(d) <= LDS_MAX),                   # 5120
    "k-means assign, AVX2 order": _largest(lambda d: assign_avx_lds(d) <= LDS_MAX),   # 5120
    "tree / hasher, batched": _largest(lambda d: max(lut_build_lds(d), rerank_lds(d)) <= LDS_MAX),   # 10240
    "lut_from_query": _largest(lambda d: lut_from_query_lds(d) <= LDS_MAX),           # 40960
    "delta scan": _largest(lambda d: delta_lds(d) <= LDS_MAX),                        # 38912
    "mmr, depth 2048": _largest(lambda d: mmr_lds(d, 2048) <= LDS_MAX),               # 34304
}

# ---- the edges: (kernel, what changes, dim at the edge, next dim the kernel accepts, predicate true at the edge only) --
EDGES = (
    ("bf_stream_kernel", "64 KB", 896, 900, lambda d: stream_lds(d) <= LDS_ATTR),
    ("bf_stream_kernel", "160 KB: bf_generic_kernel above", 3968, 3972, lambda d: stream_lds(d) <= LDS_MAX),
    ("bf_generic_kernel", "64 KB", 2044, 2048, lambda d: generic_lds(d) <= LDS_ATTR),
    ("bf_quant_kernel QT=8", "64 KB", 2048, 2056, lambda d: quant_lds(d, 9) <= LDS_ATTR),
    ("leaf_exact_scan_kernel", "4 -> 2 quads", 768, 1024, lambda d: exact_qpt(d) == 4),
    ("leaf_exact_scan_kernel", "64 KB + static", 2048, 2052, lambda d: exact_lds(d) <= LDS_ATTR),
    ("centroid_scores_kernel<4>", "64 KB", 4096, 4100, lambda d: centroid_lds(d, 4) <= LDS_ATTR),
    ("centroid_scores_kernel<16>", "64 KB", 1024, 1040, lambda d: centroid_lds(d, 16) <= LDS_ATTR),
    ("assign_nearest_kernel", "64 KB", 1024, 1028, lambda d: assign_lds(d) <= LDS_ATTR),
    ("assign_nearest_kernel", "160 KB: 16 -> 8 centres", 2560, 2564, lambda d: assign_tc(d) == 16),
    ("delta_scan_kernel", "qt 8 -> 7", 1536, 1540, lambda d: delta_qt(d) == 8),
)
# requests that land on exactly 64 KB of dynamic LDS: the last size launched without the attribute
EXACTLY_64K = (("bf_stream_kernel", 896, stream_lds), ("bf_quant_kernel QT=8", 2048, lambda d: quant_lds(d, 9)),
               ("leaf_exact_scan_kernel", 2048, exact_lds), ("centroid_scores_kernel<4>", 4096, lambda d: centroid_lds(d, 4)),
               ("centroid_scores_kernel<16>", 1024, lambda d: centroid_lds(d, 16)),
               ("assign_nearest_kernel", 1024, assign_lds))
DELTA_QT = {1536: 8, 1540: 7, 3072: 4, 4096: 3}

# ---- the dim lists of the GPU tests, by the kernel whose edges they straddle ----------------------------------------
BF_F32_DIMS = (768, 896, 900, 1024, UNALIGNED, 1536, 2044, 2048, 3072, 3968, 3972, 4096)
BF_QUANT_DIMS = (768, 1024, UNALIGNED, 1536, 2048, 2056, 3072, 4096)
PARTITIONED_DIMS = (768, 1024, UNALIGNED, 1536, 2048, 2052, 3072, 4096)
PARTITION16_DIMS = (1024, 1040)         # centroid_scores_kernel<16>: L = 8192, nq = 1024
PARTITION16_TOO_WIDE = 2564             # the same full grid where 16 queries exceed 160 KB: the <4> form
PARTITION4_DIMS = (4096, 4100)
BUILD_DIMS = (1024, 1028, 2560, 2564, 3072, 4096)
MUTABLE_DIMS = (1536, 1540, 3072, 4096)
MMR_DIMS = (UNALIGNED, 4096)
RERANK_DIMS = (768, 2048)
DIMS_OF = {"bf_stream_kernel": BF_F32_DIMS, "bf_generic_kernel": BF_F32_DIMS, "bf_quant_kernel QT=8": BF_QUANT_DIMS,
           "leaf_exact_scan_kernel": PARTITIONED_DIMS, "centroid_scores_kernel<4>": PARTITION4_DIMS,
           "centroid_scores_kernel<16>": PARTITION16_DIMS, "assign_nearest_kernel": BUILD_DIMS,
           "delta_scan_kernel": MUTABLE_DIMS}
ALL_DIMS = tuple(sorted(set().union(*DIMS_OF.values(), MMR_DIMS, RERANK_DIMS, (PARTITION16_TOO_WIDE,))))

BATCHES = (1, 3, 16, 17, 70)            # one query, the small pipelines, the last streaming batch, the first generic one, a ragged one
NQ = max(BATCHES)
BF_ROWS = 1500

# tree and flat-hasher shapes: (n, dim, L, S, K, use_residuals); dsub = dim / S spans 12 .. 256
TXH_SHAPES = {
    "768-res": (2048, 768, 8, 32, 16, True), "768-raw": (2048, 768, 8, 32, 16, False),
    "1024": (2048, 1024, 8, 64, 16, True), "1024-bytes": (2048, 1024, 8, 8, 256, True),
    "1536-res": (2048, 1536, 8, 32, 16, True), "1536-raw": (2048, 1536, 8, 32, 16, False),
    "2048": (1500, 2048, 6, 16, 16, True),
    "4096-res": (1500, 4096, 6, 16, 16, True), "4096-raw": (1500, 4096, 6, 16, 16, False),
}
AH_SHAPES = {"768": (2048, 768, 64), "1536": (2048, 1536, 32), "2048": (1500, 2048, 16)}   # (n, dim, S): dsub 12, 48, 128
TXH_P, TXH_MULT = 4, 3.0


def expected_above(*ceilings):
    """what an entry point that runs the kernels of these CEILING rows does at dim ABOVE: "ok", or 8
    (ResourceExhausted) if one of them lies below it"""
    return "ok" if all(CEILING[c] >= ABOVE for c in ceilings) else 8


def strided(rows, stride):
    """[n, stride] f32, zero padding (stride == dim: the rows themselves)"""
    n, dim = rows.shape
    out = np.zeros((n, stride), np.float32)
    out[:, :dim] = rows
    return out


def stride_of(dim):
    """the stride a case of this dim runs at: tight for the unaligned dim, else the next multiple of 16"""
    return dim if dim % 4 else (dim + 15) // 16 * 16


def signed_rows(n, dim, seed):
    """U[-1, 1) rows: dot products of both signs, SquaredL2 sums that cancel"""
    return np.random.default_rng([seed, dim]).uniform(-1.0, 1.0, (n, dim)).astype(np.float32)

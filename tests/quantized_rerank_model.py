"""Model of the re-rank of a tree / hasher index whose rows are stored quantized (scann_hip_txh_create_quantized,
DESIGN 3.4b), the checker of tests/test_gpu_quantized_rerank.py.

Given the merged candidates of a query in merged order (the oracle's: orc.txh_search(..., stages=True) /
orc.ah_search), the quantized rows by datapoint index, their format, the measure and inv_multiplier:
  1. every candidate gets tests/quantized_checker.py's distance to its stored row (what a quantized brute-force handle
     computes: bf16 / FP8 one sequential f32 sum, int8 the AVX2 arithmetic on f32(i8) * inv);
  2. the candidates are ordered stably by the f32_to_ordered key of that distance (csrc/common.h: -NaN < -inf < ... <
     +inf < +NaN), so equal distances keep their merged order;
  3. the first k are the result.
"""
import numpy as np

from tests import quantized_checker as qc


def f32_to_ordered(d):
    b = np.ascontiguousarray(d, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def candidate_distances(query, cand_idx, rows_q, dim, fmt, measure, inv_multiplier=1.0):
    """float32 [len(cand_idx)]: the checker's distance of every candidate's stored row"""
    ci = np.asarray(cand_idx, np.int64)
    if ci.size == 0:
        return np.zeros(0, np.float32)
    q = np.ascontiguousarray(np.asarray(query, np.float32)[None, :dim])
    return qc.distances(q, np.asarray(rows_q)[ci], dim, fmt, measure, inv_multiplier)[0]


def rerank(query, cand_idx, rows_q, dim, fmt, measure, inv_multiplier, k):
    """(indices uint32 [<= k], distances float32 [<= k]) of one query"""
    ci = np.asarray(cand_idx, np.uint32)
    d = candidate_distances(query, ci, rows_q, dim, fmt, measure, inv_multiplier)
    order = np.argsort(f32_to_ordered(d), kind="stable")[:k]
    return ci[order], d[order]

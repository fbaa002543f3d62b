"""The rule of scann_hip_txh_build (include/scann_hip.h "device build") as a function of the k-means++ seeds, from the
CPU oracle alone: orc.kmeans_lloyd (with col_offset for the subspaces), orc.partition, orc.encode_many and a stable
argsort for the CSR lists.  The checker of tests/test_gpu_device_build.py; tests/test_device_build_model.py checks
the model itself on the CPU.

Seeds are arguments because the seeding has no bit-level oracle (tests/build_model.py pins it): the GPU test takes them
from hip.kmeans_init_pp on the same rows and on the model's own training rows, the CPU test draws rows by a fixed
stream.  Everything after the seeds is bit-exact.

  1 partitioner    k = min(L, n) centres from `partition_seeds(k)`, orc.kmeans_lloyd over whole rows -> centres, leaf
  2 training rows  datapoint order: x - centres[orc.partition(x, 1)] (NOT the k-means assignment: from simd_threshold
                   dims on the two use different summation orders); x itself without residuals or when flat
  3 codebook       subspace s: kc = min(K, n) centres from `subspace_seeds(training rows, s, kc)`, orc.kmeans_lloyd
                   over the column window; codes kc .. K - 1 repeat centre kc - 1
  4 codes          orc.encode_many of x - centres[leaf] (x itself without residuals or when flat), CSR row order,
                   packed two per byte for K <= 16
"""
import numpy as np

from oracle import pyoracle as orc
from scann_rust_amd import synth, trainer

SIMD_THRESHOLD = 128


def strided(rows, stride):
    n, dim = rows.shape
    data = np.zeros((n, stride), np.float32)
    data[:, :dim] = rows
    return data


def model(rows, stride, cfg, partition_seeds, subspace_seeds):
    """rows [n, dim] f32; cfg: the dict of a case (below).  partition_seeds(k) -> [k, dim];
    subspace_seeds(train [n, dim], s, kc) -> [kc, dsub].  Returns a dict of every array of the built index, the
    training rows, and the iteration counts / converged flags of every Lloyd loop."""
    rows = np.ascontiguousarray(rows, np.float32)
    n, dim = rows.shape
    L, S, K = cfg.get("num_partitions", 0), cfg["num_subspaces"], cfg["num_codes"]
    thr = cfg.get("simd_threshold", SIMD_THRESHOLD)
    residual = bool(L) and bool(cfg.get("use_residuals", 1))
    dsub = dim // S
    data = strided(rows, stride)
    out = dict(data=data, n=n, dim=dim, stride=stride, L=0)
    if L:
        k = min(L, n)
        c0 = np.ascontiguousarray(partition_seeds(k), np.float32)
        oc, oa, _, inertia, iters, conv = orc.kmeans_lloyd(
            data, n, stride, dim, c0, max_iterations=cfg.get("kmeans_iterations", 100),
            convergence_threshold=cfg.get("kmeans_convergence", 1e-5), simd_threshold=thr)
        order = np.argsort(oa, kind="stable").astype(np.uint32)
        leaf_off = np.zeros(k + 1, np.uint32)
        leaf_off[1:] = np.cumsum(np.bincount(oa, minlength=k))
        out.update(L=k, centers=oc, leaf=oa, leaf_offsets=leaf_off, leaf_ids=order, partition_iterations=iters,
                   partition_converged=conv, partition_inertia=inertia)
    else:
        order = np.arange(n, dtype=np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        if residual:
            token = np.array([orc.partition(oc, r, 1)[0][0] for r in rows], np.int64)
            train = rows - oc[token]
            enc = rows - oc[oa]
            out["token"] = token
        else:
            train = enc = rows
    tdata = strided(train, stride)
    kc = min(K, n)
    cb = np.zeros((S, K, dsub), np.float32)
    its, convs = [], []
    for s in range(S):
        c0 = np.ascontiguousarray(subspace_seeds(train, s, kc), np.float32)
        c, _, _, _, it, cv = orc.kmeans_lloyd(
            tdata, n, stride, dsub, c0, max_iterations=cfg.get("training_iterations", 25),
            convergence_threshold=cfg.get("convergence_threshold", 1e-5), col_offset=s * dsub, simd_threshold=thr)
        cb[s, :kc] = c
        cb[s, kc:] = c[-1]
        its.append(it)
        convs.append(cv)
    codes = orc.encode_many(cb, enc)[order]
    out.update(train=train, codebook=cb, codes=codes, codes_file=trainer.pack4(codes) if K <= 16 else codes,
               subspace_iterations=its, subspace_converged=convs, order=order)
    return out


def stream_seeds(window, k, seed):
    """k rows of `window` drawn by a fixed stream (the CPU test's seeds; distinct picks are not required)"""
    pick = (synth.splitmix64(seed, 0, k) % np.uint64(window.shape[0])).astype(np.int64)
    return np.ascontiguousarray(window[pick], np.float32)


# ---- the cases of tests/test_gpu_device_build.py: the smallest shapes at which each piece can go wrong ---------------
def _clustered(n, dim, seed, clusters):
    return synth.clustered_f32(n, dim, seed, n_clusters=clusters)[0]


def _freeze_rows():
    """flat, dim 32, S = 8: subspace 0 constant, subspace 1 two-valued, the rest clustered noise"""
    n = 1500
    rows = _clustered(n, 32, 77, 12).copy()
    rows[:, 0:4] = np.float32(0.375)
    rows[:, 4:8] = np.where((np.arange(n) % 3 == 0)[:, None], np.float32(1.0), np.float32(-2.0))
    return rows


def case(name):
    """(rows [n, dim] f32, stride or None = compute_stride(dim), cfg dict) of one build case"""
    from tests import helpers as H
    rng = np.random.default_rng([97, sorted(CASES).index(name)])
    stride = None
    base = dict(num_partitions=0, num_subspaces=8, num_codes=16, kmeans_iterations=20, training_iterations=8,
                partitions_to_search=3, pre_reorder_multiplier=4.0)
    if name == "tree":                      # the shape of test_build_chain_matches_oracle_step_by_step
        rows, cfg = _clustered(3000, 32, 541, 8), dict(num_partitions=8)
    elif name == "flat":
        rows, cfg = _clustered(2500, 16, 542, 6), dict()
    elif name == "flat-no-rows":
        rows, cfg = _clustered(2500, 16, 542, 6), dict(store_rows=0)
    elif name == "byte-codes":
        rows, cfg = _clustered(3000, 16, 543, 9), dict(num_partitions=6, num_subspaces=4, num_codes=256,
                                                       training_iterations=4)
    elif name == "fewer-rows-than-codes":   # k = min(K, n), the repeated last centre
        rows, cfg = _clustered(200, 16, 544, 5), dict(num_partitions=3, num_subspaces=4, num_codes=256,
                                                      training_iterations=4)
    elif name == "subspace-groups":         # 16 x 256 x 16 x 4 B of codebook: several LDS stagings
        rows, cfg = _clustered(600, 256, 545, 7), dict(num_partitions=4, num_subspaces=16, num_codes=256,
                                                       kmeans_iterations=5, training_iterations=3)
    elif name == "freeze":                  # per-subspace stop: iteration counts differ (test_device_build_model)
        rows, cfg = _freeze_rows(), dict(training_iterations=4)
    elif name == "partition-dim-128":       # AVX2 order in the partitioner, sequential tokens
        rows, cfg = _clustered(600, 128, 546, 5), dict(num_partitions=5, kmeans_iterations=6, training_iterations=3)
    elif name == "partition-dim-136":       # ... with a tail (dsub 17: the generic batched kernel)
        rows, cfg = _clustered(600, 136, 547, 5), dict(num_partitions=5, kmeans_iterations=6, training_iterations=3)
    elif name == "codebook-dsub-128":       # AVX2 order in the codebook: the per-subspace route under either flag
        rows, cfg = _clustered(300, 1024, 548, 4), dict(num_partitions=3, kmeans_iterations=4, training_iterations=3)
    elif name == "one-row":
        rows, cfg = rng.uniform(-1, 1, (1, 8)).astype(np.float32), dict(num_partitions=4)
    elif name == "n-257":
        rows, cfg = _clustered(257, 16, 549, 5), dict(num_partitions=5)
    elif name == "more-leaves-than-rows":
        rows, cfg = rng.uniform(-1, 1, (5, 8)).astype(np.float32), dict(num_partitions=9)
    elif name == "copies":                  # empty clusters, the total == 0 seeding fallback
        rows = np.tile(rng.uniform(-1, 1, (25, 8)).astype(np.float32), (600, 1))
        cfg = dict(num_partitions=40, kmeans_iterations=6, training_iterations=4)
    elif name == "nan-row":
        rows, cfg = H.build_rows("nan", 700, 16, 550), dict(num_partitions=5, kmeans_iterations=5,
                                                            training_iterations=4)
    elif name == "no-residuals":
        rows, cfg = _clustered(1000, 16, 551, 6), dict(num_partitions=6, use_residuals=0)
    elif name == "odd-stride":              # no multiple of 4: every scalar load path
        rows, cfg, stride = _clustered(1000, 16, 552, 6), dict(num_partitions=6), 17
    elif name == "zero-iterations":
        rows, cfg = _clustered(1000, 16, 553, 6), dict(num_partitions=6, kmeans_iterations=0, training_iterations=0)
    else:
        raise ValueError(name)
    base.update(cfg)
    return np.ascontiguousarray(rows, np.float32), stride, base


CASES = ("tree", "flat", "flat-no-rows", "byte-codes", "fewer-rows-than-codes", "subspace-groups", "freeze",
         "partition-dim-128", "partition-dim-136", "codebook-dsub-128", "one-row", "n-257", "more-leaves-than-rows",
         "copies", "nan-row", "no-residuals", "odd-stride", "zero-iterations")

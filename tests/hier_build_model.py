"""The rule of scann_hip_txh_build_hierarchical (include/scann_hip.h "hierarchical device build") as a function of the
k-means++ seeds, from the CPU oracle alone: orc.kmeans_lloyd on the rows of every node, ordered f64 means for the leaf
centres, then steps 2-5 of the device build restated (tests/device_build_model.py states them for the flat partitioner).
The checker of tests/test_gpu_hier_build.py; tests/test_hier_build_model.py checks the model itself on the CPU.

`seeds(node_rows [n_node, dim], k, depth) -> [k, dim]` is an argument because the seeding has no bit-level oracle
(tests/build_model.py pins it): the GPU test takes hip.kmeans_init_pp on a brute-force handle of the node's rows with
seed + depth, the CPU test draws k-means++ picks by the same stream in numpy arithmetic.

  1 tree   LEVEL BY LEVEL: a level is the list of its nodes in order, each (members ascending, depth, leaf?).  A node
           that is no leaf yet becomes one when depth >= max_depth, n_node <= min_leaf_size or n_node <= num_children;
           otherwise k = min(num_children, n_node) centres from `seeds`, orc.kmeans_lloyd over the node's rows; its
           non-empty clusters, in cluster order, replace it in the next level -- unless there is exactly one, which
           makes the node a leaf.  A leaf keeps its place.  The last level is the leaves in depth-first order.
           Centre of a leaf: per dimension the f64 sum of its members in ascending order / count, cast to f32.
  2-5      training rows x - centres[orc.partition(x, 1)] in datapoint order, codebook per subspace, codes of
           x - centres[leaf] in CSR order, as tests/device_build_model.py has them.
"""
import numpy as np

from oracle import pyoracle as orc
from scann_rust_amd import synth, trainer

SIMD_THRESHOLD = 128
MAX_LEAVES = 16384

TREE_DEFAULTS = dict(num_children=100, max_depth=1, min_leaf_size=1, kmeans_iterations=100, kmeans_convergence=1e-5,
                     seed=42)


def strided(rows, stride):
    n, dim = rows.shape
    data = np.zeros((n, stride), np.float32)
    data[:, :dim] = rows
    return data


def ordered_mean(rows, members):
    """compute_center (kmeans_tree.rs:270-284): a sequential f64 sum per dimension (cumsum adds in order)"""
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.cumsum(rows[members].astype(np.float64), axis=0)[-1]
        return (s / np.float64(len(members))).astype(np.float32)


def train_node(rows, stride, members, depth, tree, thr, seeds):
    """k-means of one node on its own rows: (clusters = member arrays of the NON-EMPTY clusters in order, info)"""
    dim = rows.shape[1]
    sub = np.ascontiguousarray(rows[members], np.float32)
    k = min(tree["num_children"], len(members))
    c0 = np.ascontiguousarray(seeds(sub, k, depth), np.float32)
    assert c0.shape == (k, dim)
    _, oa, _, inertia, iters, conv = orc.kmeans_lloyd(
        strided(sub, stride), len(members), stride, dim, c0, max_iterations=tree["kmeans_iterations"],
        convergence_threshold=tree["kmeans_convergence"], simd_threshold=thr)
    oa = np.asarray(oa, np.int64)
    clusters = [members[oa == c] for c in range(k)]
    clusters = [m for m in clusters if m.size]
    info = dict(depth=depth, n=len(members), k=k, iterations=int(iters), converged=bool(conv), inertia=float(inertia),
                nonempty=len(clusters), seeds=c0)
    return clusters, info


def is_leaf_before_training(n_node, depth, tree):
    return depth >= tree["max_depth"] or n_node <= tree["min_leaf_size"] or n_node <= tree["num_children"]


def tree_model(rows, stride, tree, thr, seeds, centres=True):
    """Step 1, level by level.  Returns dict(leaves = [member arrays], leaf_depth, centers [L, dim] (None without
    `centres`), trained = [info of every node that ran k-means, level by level], levels = per depth 0..4 the report's
    (nodes, iterations, converged, leaves))"""
    rows = np.ascontiguousarray(rows, np.float32)
    tree = dict(TREE_DEFAULTS, **tree)
    n = rows.shape[0]
    level = [(np.arange(n, dtype=np.int64), 0, False)]
    trained = []
    d = 0
    while True:
        nxt, any_trained = [], False
        for members, depth, leaf in level:
            if leaf or is_leaf_before_training(len(members), d, tree):
                nxt.append((members, depth, True))
                continue
            any_trained = True
            clusters, info = train_node(rows, stride, members, d, tree, thr, seeds)
            trained.append(info)
            if len(clusters) == 1:
                nxt.append((members, depth, True))
            else:
                nxt.extend((m, d + 1, False) for m in clusters)
        level = nxt
        if not any_trained:
            break
        d += 1
    leaves = [m for m, _, _ in level]
    leaf_depth = [dp for _, dp, _ in level]
    levels = [dict(nodes=sum(1 for t in trained if t["depth"] == dd),
                   iterations=sum(t["iterations"] for t in trained if t["depth"] == dd),
                   converged=sum(1 for t in trained if t["depth"] == dd and t["converged"]),
                   leaves=sum(1 for x in leaf_depth if x == dd)) for dd in range(5)]
    cen = np.stack([ordered_mean(rows, m) for m in leaves]) if centres else None
    return dict(leaves=leaves, leaf_depth=leaf_depth, centers=cen, trained=trained, levels=levels)


def tree_recursive(rows, stride, tree, thr, seeds):
    """Step 1 as a plain transcription of build_node / collect_leaves (kmeans_tree.rs:212-267): (leaves, depths, centres)"""
    rows = np.ascontiguousarray(rows, np.float32)
    tree = dict(TREE_DEFAULTS, **tree)

    def build_node(members, depth):
        center = ordered_mean(rows, members)
        if is_leaf_before_training(len(members), depth, tree):
            return dict(center=center, members=members, depth=depth, children=None)
        clusters, _ = train_node(rows, stride, members, depth, tree, thr, seeds)
        if len(clusters) == 1:
            return dict(center=center, members=members, depth=depth, children=None)
        return dict(center=center, members=members, depth=depth, children=[build_node(m, depth + 1) for m in clusters])

    def collect_leaves(node, out):
        if node["children"] is None:
            out.append(node)
        else:
            for ch in node["children"]:
                collect_leaves(ch, out)

    out = []
    collect_leaves(build_node(np.arange(rows.shape[0], dtype=np.int64), 0), out)
    return [x["members"] for x in out], [x["depth"] for x in out], np.stack([x["center"] for x in out])


def model(rows, stride, tree, cfg, seeds, subspace_seeds):
    """Every array of the built index.  subspace_seeds(train [n, dim], s, kc) -> [kc, dsub]."""
    rows = np.ascontiguousarray(rows, np.float32)
    n, dim = rows.shape
    S, K = cfg["num_subspaces"], cfg["num_codes"]
    thr = cfg.get("simd_threshold", SIMD_THRESHOLD)
    residual = bool(cfg.get("use_residuals", 1))
    dsub = dim // S
    data = strided(rows, stride)
    tm = tree_model(rows, stride, tree, thr, seeds)
    leaves, oc = tm["leaves"], tm["centers"]
    L = len(leaves)
    assert L <= MAX_LEAVES
    order = np.concatenate(leaves).astype(np.uint32)
    leaf_off = np.zeros(L + 1, np.uint32)
    leaf_off[1:] = np.cumsum([m.size for m in leaves])
    oa = np.zeros(n, np.uint32)
    for l, m in enumerate(leaves):
        oa[m] = l
    out = dict(data=data, n=n, dim=dim, stride=stride, L=L, centers=oc, leaf=oa, leaf_offsets=leaf_off, leaf_ids=order,
               tree=tm)
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


def stream_pp_seeds(window, k, seed):
    """k-means++ picks of `window` by the library's stream (splitmix64(seed): output 0 mod n, then (u, fallback) per
    seed) in numpy f64 arithmetic -- the CPU test's fixed stream.  Not bit-level: the library's picks may differ where a
    cumulative sum lies next to its threshold."""
    win = np.asarray(window, np.float64)
    n = win.shape[0]
    z = synth.splitmix64(seed, 0, 2 * k - 1)
    picks = [int(z[0] % np.uint64(n))]
    min_d = None
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(1, k):
            d = ((win - win[picks[-1]]) ** 2).sum(1)
            min_d = d if min_d is None else np.where(d < min_d, d, min_d)
            u = float(int(z[2 * c - 1] >> np.uint64(11))) * 2.0 ** -53
            fallback = int(z[2 * c] % np.uint64(n))
            total = min_d.sum()
            if not total > 0:
                picks.append(fallback)
            elif np.isinf(total):
                picks.append(int(np.flatnonzero(np.isinf(min_d))[0]))
            else:
                picks.append(min(int(np.searchsorted(np.cumsum(min_d), u * total, "left")), n - 1))
    return np.ascontiguousarray(np.asarray(window, np.float32)[picks])


def tree_sum_needs_chain(dist):
    """the exactness test of the inertia (scann_hip.h, scann_hip_kmeans_lloyd): True when the f64 tree sum of these
    f32 terms is not provably the sum in datapoint order"""
    dist = np.asarray(dist, np.float32)
    pos = dist[dist > 0]
    if pos.size == 0:
        return False
    total = float(dist.astype(np.float64).sum())
    if not np.isfinite(total):
        return True
    _, e = np.frexp(np.float32(pos.min()))
    return total > 2.0 ** (max(int(e) - 24, -149) + 53)


# ---- the cases of tests/test_gpu_hier_build.py: the smallest shapes at which each piece can go wrong -----------------
def _clustered(n, dim, seed, clusters):
    return synth.clustered_f32(n, dim, seed, n_clusters=clusters)[0]


def _blobs(sizes, dim, seed):
    """well separated blobs of the given sizes, datapoints shuffled; a blob of fewer than 400 rows lies ten times as
    far out as the others, so the D^2 sampling takes it before it takes the second large one"""
    rng = np.random.default_rng([211, seed])
    cen = rng.uniform(-40.0, 40.0, (len(sizes), dim)) * np.where(np.array(sizes) < 400, 10.0, 1.0)[:, None]
    pts = np.concatenate([cen[i] + rng.standard_normal((s, dim)) for i, s in enumerate(sizes)])
    return np.ascontiguousarray(pts[rng.permutation(pts.shape[0])], np.float32)


def _chain_rows():
    """half the rows within 1e-9 of the origin, half at 1e3: with the first seed among the tiny rows, iteration 1 of the
    root has distances of 1e-18 next to 1e7"""
    n, dim = 2000, 8
    x = np.random.default_rng(212).standard_normal((n, dim)).astype(np.float32)
    first = int(synth.splitmix64(42, 0, 1)[0] % np.uint64(n))
    tiny = np.arange(n) < n // 2 if first < n // 2 else np.arange(n) >= n // 2
    x[tiny] *= np.float32(1e-9)
    x[~tiny] *= np.float32(1e3)
    return x


def case(name):
    """(rows [n, dim] f32, stride or None = compute_stride(dim), tree dict, cfg dict) of one build case"""
    from tests import helpers as H
    rng = np.random.default_rng([98, sorted(CASES).index(name)])
    stride = None
    tree = dict(num_children=4, max_depth=2, min_leaf_size=1, kmeans_iterations=20, kmeans_convergence=1e-5, seed=42)
    cfg = dict(num_subspaces=8, num_codes=16, training_iterations=6, partitions_to_search=3, pre_reorder_multiplier=4.0)
    if name == "depth-2":
        rows = _clustered(3000, 16, 641, 16)
    elif name == "depth-3":                 # the node numbering passes through two prefix sums
        rows = _clustered(2000, 8, 642, 27)
        tree.update(num_children=3, max_depth=3)
    elif name == "dim-128":                 # AVX2 order in every node's k-means, sequential tokens
        rows = _clustered(1500, 128, 643, 16)
        tree.update(kmeans_iterations=6)
        cfg.update(training_iterations=3)
    elif name == "dim-136":                 # ... with a tail
        rows = _clustered(1500, 136, 644, 16)
        tree.update(kmeans_iterations=6)
        cfg.update(training_iterations=3)
    elif name == "mixed-depth":             # small clusters stay leaves at depth 1 between siblings that split
        rows = _blobs([700, 120, 700, 120, 700, 120, 700, 120], 8, 645)
        tree.update(num_children=8, min_leaf_size=400)
    elif name == "outliers":                # three far rows: a depth-1 node with n_node <= num_children
        rows = _clustered(1200, 8, 646, 6).copy()
        rows[[17, 500, 1100]] = np.float32(500.0) + rng.uniform(-1, 1, (3, 8)).astype(np.float32)
        tree.update(num_children=8)
    elif name == "copies":                  # empty clusters dropped; nodes with one non-empty cluster
        rows = np.tile(rng.uniform(-1, 1, (25, 8)).astype(np.float32), (600, 1))
        tree.update(num_children=8, kmeans_iterations=6)
        cfg.update(training_iterations=4)
    elif name == "root-n-7":                # n <= num_children at the root: one leaf
        rows = rng.uniform(-1, 1, (7, 8)).astype(np.float32)
        tree.update(num_children=8)
    elif name == "root-depth-0":
        rows = _clustered(500, 16, 647, 5)
        tree.update(max_depth=0)
    elif name == "depth-1":                 # against the flat build (test_gpu_hier_build)
        rows = _clustered(1000, 16, 648, 6)
        tree.update(num_children=6, max_depth=1)
    elif name == "odd-stride":              # no multiple of 4: every scalar load path
        rows, stride = _clustered(1000, 16, 649, 9), 17
    elif name == "nan-row":
        rows = H.build_rows("nan", 700, 16, 650)
        tree.update(kmeans_iterations=5)
        cfg.update(training_iterations=4)
    elif name == "no-residuals":
        rows = _clustered(1000, 16, 651, 9)
        cfg.update(use_residuals=0)
    elif name == "no-rows":
        rows = _clustered(1000, 16, 652, 9)
        cfg.update(store_rows=0)
    elif name == "zero-iterations":
        rows = _clustered(1000, 16, 653, 9)
        tree.update(kmeans_iterations=0)
        cfg.update(training_iterations=0)
    elif name == "byte-codes":
        rows = _clustered(1500, 16, 654, 9)
        cfg.update(num_subspaces=4, num_codes=256, training_iterations=4)
    elif name == "inertia-chain":           # a node whose tree sum is not provably exact
        rows = _chain_rows()
        tree.update(num_children=2, kmeans_iterations=4)
    else:
        raise ValueError(name)
    return np.ascontiguousarray(rows, np.float32), stride, tree, cfg


CASES = ("depth-2", "depth-3", "dim-128", "dim-136", "mixed-depth", "outliers", "copies", "root-n-7", "root-depth-0",
         "depth-1", "odd-stride", "nan-row", "no-residuals", "no-rows", "zero-iterations", "byte-codes", "inertia-chain")


def too_many_leaves_case():
    """(rows, tree): 40 000 uniform points of the plane, 130 children, depth 2 -- more than 16384 leaves (refused).
    The two coordinates stand in the first two of 8 columns, the other six are zero: every distance is the 40 000 x 2
    set's bit for bit (the zero columns add exact zeros), and the rows have a dimensionality that a codebook shape
    exists for -- no (num_subspaces, num_codes) the build accepts divides 2 dimensions, so a 40 000 x 2 handle is
    refused for its shape before the tree stage and could never reach the leaf ceiling."""
    rows = np.zeros((40000, 8), np.float32)
    rows[:, :2] = synth.uniform_f32(40000, 2, 655)
    return rows, dict(num_children=130, max_depth=2, min_leaf_size=1, kmeans_iterations=2, kmeans_convergence=1e-5,
                      seed=42)


def condition(name, rows, tree, tm):
    """None, or why the case does not meet the condition it is named for (tm: tree_model's result)"""
    depth, sizes, trained = tm["leaf_depth"], [m.size for m in tm["leaves"]], tm["trained"]
    C = tree["num_children"]
    if name in ("depth-2", "dim-128", "dim-136", "odd-stride", "no-residuals", "no-rows", "byte-codes", "zero-iterations"):
        return None if max(depth) == 2 and tm["levels"][1]["nodes"] > 1 else "no second level"
    if name == "depth-3":
        return None if max(depth) == 3 and tm["levels"][2]["nodes"] > 1 else "no third level"
    if name == "mixed-depth":
        ok = any(depth[i] == 1 and 2 in depth[:i] and 2 in depth[i + 1:] for i in range(len(depth)))
        return None if ok else "no depth-1 leaf between split siblings: %s" % depth
    if name == "outliers":
        ok = any(d == 1 and s == 3 for d, s in zip(depth, sizes)) and max(depth) == 2
        return None if ok else "the outliers are no depth-1 leaf of their own: %s" % list(zip(depth, sizes))
    if name == "copies":
        dropped = any(1 < t["nonempty"] < t["k"] for t in trained)
        single = any(t["nonempty"] == 1 for t in trained)
        return None if dropped and single else "dropped=%s single=%s" % (dropped, single)
    if name in ("root-n-7", "root-depth-0"):
        return None if depth == [0] and not trained else "the root is no leaf"
    if name == "depth-1":
        return None if max(depth) == 1 and len(trained) == 1 else "not one k-means"
    if name == "nan-row":
        return None if np.isnan(rows).any() and len(depth) > 1 else "no NaN / no split"
    if name == "inertia-chain":
        r = np.asarray(rows, np.float32)
        c0 = trained[0]["seeds"]
        with np.errstate(over="ignore"):
            d0 = np.min(((r[:, None, :] - c0[None]) ** 2).sum(2, dtype=np.float32), axis=1)
        return None if tree_sum_needs_chain(d0) else "the root's first inertia is provably exact"
    raise ValueError(name)

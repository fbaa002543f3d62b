"""tests/hier_build_model.py on the CPU: the level-order statement of the tree against a plain recursive transcription
of build_node / collect_leaves on every case, every case's own condition, the too-many-leaves shape, and the new entry
points in the header, hip.py and the library's exports."""
import functools
import os
import re

import numpy as np
import pytest

from tests import hier_build_model as HM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cpu_seeds(tree):
    return lambda node_rows, k, depth: HM.stream_pp_seeds(node_rows, k, tree["seed"] + depth)


def _stride(dim, stride):
    return (dim + 3) // 4 * 4 if stride is None else stride


@functools.lru_cache(maxsize=None)
def trees(name):
    rows, stride, tree, cfg = HM.case(name)
    st = _stride(rows.shape[1], stride)
    thr = cfg.get("simd_threshold", HM.SIMD_THRESHOLD)
    return rows, tree, HM.tree_model(rows, st, tree, thr, cpu_seeds(tree)), HM.tree_recursive(rows, st, tree, thr,
                                                                                             cpu_seeds(tree))


@pytest.mark.parametrize("name", HM.CASES)
def test_level_order_is_the_recursion(name):
    rows, tree, tm, (leaves, depths, centres) = trees(name)
    assert len(tm["leaves"]) == len(leaves) and tm["leaf_depth"] == depths
    for a, b in zip(tm["leaves"], leaves):
        assert np.array_equal(a, b) and np.all(np.diff(a) > 0)
    assert np.array_equal(np.sort(np.concatenate(leaves)), np.arange(rows.shape[0]))
    nan = np.isnan(centres)
    assert np.array_equal(np.isnan(tm["centers"]), nan)
    assert np.array_equal(tm["centers"].view(np.uint32)[~nan], centres.view(np.uint32)[~nan])
    assert sum(lv["leaves"] for lv in tm["levels"]) == len(leaves) <= HM.MAX_LEAVES
    assert sum(lv["nodes"] for lv in tm["levels"]) == len(tm["trained"])


@pytest.mark.parametrize("name", HM.CASES)
def test_case_meets_its_condition(name):
    rows, tree, tm, _ = trees(name)
    assert HM.condition(name, rows, tree, tm) is None


def test_full_model_on_a_small_case():
    rows, stride, tree, cfg = HM.case("depth-3")
    st = _stride(rows.shape[1], stride)
    dsub = rows.shape[1] // cfg["num_subspaces"]
    m = HM.model(rows, st, tree, cfg, cpu_seeds(tree),
                 lambda train, s, kc: HM.stream_pp_seeds(train[:, s * dsub:(s + 1) * dsub], kc, 42 + s))
    n = rows.shape[0]
    assert m["leaf_offsets"][-1] == n and np.array_equal(np.sort(m["leaf_ids"]), np.arange(n))
    for l in range(m["L"]):
        ids = m["leaf_ids"][m["leaf_offsets"][l]:m["leaf_offsets"][l + 1]]
        assert np.all(m["leaf"][ids] == l) and np.all(np.diff(ids.astype(np.int64)) > 0)
    assert m["codes"].shape == (n, cfg["num_subspaces"]) and m["codebook"].shape == (cfg["num_subspaces"], 16, dsub)


def test_too_many_leaves_shape_exceeds_the_ceiling():
    rows, tree = HM.too_many_leaves_case()
    tm = HM.tree_model(rows, 8, tree, HM.SIMD_THRESHOLD, cpu_seeds(tree), centres=False)
    assert len(tm["leaves"]) > HM.MAX_LEAVES, len(tm["leaves"])


def test_entry_points_declared_bound_and_exported():
    from scann_rust_amd import build, hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scann_hip.h")).read(), flags=re.S)
    L = hip.load()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("scann_hip_txh_build_hierarchical", "scann_hip_tree_config_default"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(L, name) and name in hip.EXPORTS
        assert re.search(r"\bfn %s\s*\(" % name, doc), name
    for struct in ("scann_hip_tree_config", "scann_hip_tree_report"):
        assert re.search(r"typedef\s+struct\s+%s\s*\{" % struct, text), struct
        assert "pub struct %s {" % struct in doc
    assert "ktree.hip" in build.SOURCES and "ktree.h" in build.HEADERS
    t = hip.tree_config()
    assert (t.num_children, t.max_depth, t.min_leaf_size, t.kmeans_iterations, t.kmeans_convergence, t.seed) == \
        (100, 1, 1, 100, 1e-5, 42)
    assert hip.tree_config(num_children=7, max_depth=3).max_depth == 3
    with pytest.raises(TypeError):
        hip.tree_config(no_such_field=1)
    assert callable(hip.txh_build_hierarchical)
    import ctypes as C
    assert C.sizeof(hip.TreeConfig) == 32 and C.sizeof(hip.TreeReport) == 8 + 4 * 20 + 40

"""CPU checks of multi-attribute crowding and MMR: the numpy models of CrowdingMultidimensional::apply and
MmrDiversifier::apply against the reference's own unit-test data (restricts/crowding.rs:313-374) and the properties the
GPU tests rest on; the C++ mirror's types (host-only program); the new entry points declared, exported, bound and
documented."""
import os
import re
import subprocess

import numpy as np

import crowding_model as CM
import diversify_model as DM
from oracle import pyoracle as orc
from scann_rust_amd import build, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scann_hip.h")
NEW_SYMBOLS = ("scann_hip_search_mmr", "scann_hip_search_mmr_device", "scann_hip_index_reserve_mmr", "scann_hip_mmr_apply",
               "scann_hip_index_set_crowding_attributes_md", "scann_hip_search_crowded_md",
               "scann_hip_search_crowded_md_device", "scann_hip_crowd_md_apply")
NEW_METHODS = ("search_mmr", "search_mmr_device", "mmr_apply", "set_crowding_attributes_md", "search_crowded_md",
               "search_crowded_md_device", "crowd_md_apply", "reserve_mmr")


def _read(path):
    with open(path, encoding="utf-8") as fh:
        return fh.read()


REF_ATTRS = np.array([[1, 1, 2, 2, 3, 3], [10, 10, 10, 20, 20, 30]], np.uint64)     # crowding.rs:317-331
REF_IDX = np.arange(6, dtype=np.uint32)
REF_DIST = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6], np.float32)


def test_md_reference_vector():
    """test_multidimensional_crowding's data with limits [2, 2]: 2 is rejected by region 10 -> [0, 1, 3, 4, 5]"""
    gi, gd = DM.md_apply(REF_IDX, REF_DIST, REF_ATTRS, [2, 2], 6)
    assert gi.tolist() == [0, 1, 3, 4, 5]
    assert np.array_equal(gd, REF_DIST[[0, 1, 3, 4, 5]])
    assert DM.md_apply(REF_IDX, REF_DIST, REF_ATTRS, [2, 2], 3)[0].tolist() == [0, 1, 3]     # stops at k kept
    assert DM.md_apply(REF_IDX, REF_DIST, REF_ATTRS, [2, 2], 0)[0].size == 0


def test_mmr_reference_vector():
    """test_mmr_diversifier: lambda 0.5, identity similarity, k = 3 -> [0, 1, 2]"""
    idx = np.arange(4, dtype=np.uint32)
    dist = np.array([0.1, 0.2, 0.3, 0.4], np.float32)
    gi, gd, fb = DM.mmr_apply(idx, dist, 3, 0.5, lambda a, b: 1.0 if a == b else 0.0)
    assert gi.tolist() == [0, 1, 2] and np.array_equal(gd, dist[:3]) and fb == 0
    assert DM.mmr_apply(idx, dist, 0, 0.5, lambda a, b: 0.0)[0].size == 0
    assert DM.mmr_apply(idx[:0], dist[:0], 3, 0.5, lambda a, b: 0.0)[0].size == 0
    # pure diversity: the entry least similar to entry 0
    assert DM.mmr_apply(idx, dist, 2, 0.0, lambda a, b: -abs(a - b))[0].tolist() == [0, 3]


def test_md_one_dimension_is_the_one_attribute_rule():
    rng = np.random.default_rng(21)
    for trial in range(100):
        n = int(rng.integers(0, 120))
        row = rng.permutation(300)[:n].astype(np.uint32)
        dist = np.sort(rng.random(n).astype(np.float32))
        attrs = rng.integers(0, int(rng.integers(1, 15)), 200).astype(np.uint64)     # shorter than the index range
        for limit in (0, 1, 2, 7, 2 ** 32 - 1):
            for k in (0, 1, 5, n):
                wi, wd = CM.apply(row, dist, attrs, limit, k)
                gi, gd = DM.md_apply(row, dist, attrs[None], [limit], k)
                assert np.array_equal(gi, wi) and np.array_equal(gd, wd), (trial, limit, k)


def test_md_limit_zero_keeps_nothing_and_missing_attributes_are_zero():
    for limits in ([0, 5], [5, 0], [0, 0]):
        assert DM.md_apply(REF_IDX, REF_DIST, REF_ATTRS, limits, 6)[0].size == 0
    # indices 6.. have attribute 0 in both dimensions: they crowd together, not with anything else
    gi, _ = DM.md_apply(np.array([7, 0, 9, 8], np.uint32), np.arange(4, dtype=np.float32), REF_ATTRS, [1, 1], 4)
    assert gi.tolist() == [7, 0]


def test_md_chain_depends_on_rejections():
    """dimension 0 = p // 2, dimension 1 = (p + 1) // 2, limits (1, 1): exactly the even positions are kept.  Entry p is
    blocked by p - 1 only if p - 1 was KEPT: counting earlier entries instead of earlier kept entries keeps entry 0
    alone."""
    p = np.arange(300, dtype=np.uint64)
    attrs = np.stack([p // np.uint64(2), (p + np.uint64(1)) // np.uint64(2)])
    idx = np.arange(300, dtype=np.uint32)
    dist = np.arange(300, dtype=np.float32)
    gi, _ = DM.md_apply(idx, dist, attrs, [1, 1], 300)
    assert gi.tolist() == list(range(0, 300, 2))
    assert DM.md_apply(idx, dist, attrs, [1, 1], 70)[0].tolist() == list(range(0, 140, 2))
    by_earlier = [q for q in range(300) if q // 2 not in [r // 2 for r in range(q)]
                  and (q + 1) // 2 not in [(r + 1) // 2 for r in range(q)]]
    assert by_earlier == [0]


def test_mmr_lambda_one_returns_the_first_k():
    rng = np.random.default_rng(22)
    idx = rng.permutation(50).astype(np.uint32)
    dist = np.sort(rng.random(50).astype(np.float32))
    assert np.all(np.diff(dist) > 0)
    sims = rng.normal(size=(50, 50)).astype(np.float32)
    gi, gd, fb = DM.mmr_apply(idx, dist, 20, 1.0, lambda a, b: sims[a, b])
    assert np.array_equal(gi, idx[:20]) and np.array_equal(gd, dist[:20]) and fb == 0
    assert np.array_equal(DM.mmr_apply(idx, dist, 20, 7.5, lambda a, b: sims[a, b])[0], idx[:20])    # clamped to 1


def test_mmr_f32_min_fallback():
    """every similarity NaN: max_sim stays f32::MIN and the scores tie at -(1 - lambda) * MIN: the lowest position wins.
    Every SCORE NaN (inf - inf): no score exceeds f32::MIN, best_idx stays 0: row order, one fall-back per round."""
    idx = np.array([4, 2, 9, 1], np.uint32)
    dist = np.array([0.1, 0.2, 0.3, 0.4], np.float32)
    gi, _, fb = DM.mmr_apply(idx, dist, 4, 0.5, lambda a, b: float("nan"))
    assert gi.tolist() == [4, 2, 9, 1] and fb == 0
    ninf = np.full(4, -np.inf, np.float32)
    gi, gd, fb = DM.mmr_apply(idx, ninf, 4, 0.5, lambda a, b: float("inf"))
    assert gi.tolist() == [4, 2, 9, 1] and fb == 3
    # a -inf similarity leaves max_sim at f32::MIN; at lambda = 1 the score is -dist - 0 * MIN
    gi, _, fb = DM.mmr_apply(idx, dist, 3, 1.0, lambda a, b: float("-inf"))
    assert gi.tolist() == [4, 2, 9] and fb == 0


def test_mmr_rows_model_equals_the_walk():
    """mmr_apply_rows (a running max, one oracle call per round) == mmr_apply with the oracle's pair distance, for all
    five measures, an odd dimension (scalar tail) and rows that overflow to +-inf"""
    rng = np.random.default_rng(23)
    n, dim = 60, 11
    rows = rng.normal(size=(n, dim)).astype(np.float32)
    rows[::7] *= np.float32(2.0 ** 66)            # dot products and squared distances of these overflow
    data, stride = orc.to_strided(rows)
    falls = 0
    for measure in (hip.SQUARED_L2, hip.L2, hip.DOT_PRODUCT, hip.L1, hip.COSINE):
        sim = lambda a, b: -orc.measure_distance(measure, rows[a], rows[b])
        for lam in (0.0, 0.3, 1.0):
            idx = rng.permutation(n)[:25].astype(np.uint32)
            dist = np.sort(rng.normal(size=25).astype(np.float32))
            for k in (1, 7, 25):
                wi, wd, wf = DM.mmr_apply(idx, dist, k, lam, sim)
                gi, gd, gf = DM.mmr_apply_rows(idx, dist, k, lam, data, stride, dim, measure)
                assert np.array_equal(gi, wi) and np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), (measure, lam, k)
                assert gf == wf
                falls += gf
    assert falls > 0


def test_host_cpp_diversify_types():
    """CrowdingMultidimensional and MmrDiversifier of scann.hpp on the same vectors"""
    build.build_host()
    exe = os.path.join(os.path.dirname(os.path.abspath(build.__file__)), "host", "diversify_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "diversify_test ok" in r.stdout


def test_new_symbols_declared_exported_bound_and_documented():
    decl = re.sub(r"/\*.*?\*/", "", _read(HEADER), flags=re.S)
    lib = hip.load()
    doc = _read(os.path.join(ROOT, "INTEGRATION.md"))
    block = doc[doc.index('extern "C" {'):doc.index("<!-- END generated -->")]
    dynsym = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, decl), "%s is not declared in scann_hip.h" % name
        assert name in hip.EXPORTS and getattr(lib, name) is not None
        assert getattr(lib, name).argtypes is not None, "%s has no argtypes in hip.py" % name
        assert re.search(r"\bT %s$" % name, dynsym, flags=re.M), "%s is not exported by the library" % name
        assert "pub fn %s(" % name in block, "INTEGRATION.md's extern block lacks %s" % name
    for name in NEW_METHODS:
        assert callable(getattr(hip.Index, name, None)), "hip.Index.%s is missing" % name
    hdr = _read(HEADER)
    assert int(re.search(r"#define SCANN_HIP_MMR_MAX_DEPTH (\d+)", hdr).group(1)) == hip.MMR_MAX_DEPTH == 2048
    assert int(re.search(r"#define SCANN_HIP_CROWD_MAX_DIMS (\d+)", hdr).group(1)) == hip.CROWD_MAX_DIMS == 8
    m = re.search(r"scann_hip_search_mmr\s*\(([^;]*?)\)\s*;", decl, flags=re.S)
    assert " ".join(m.group(1).split()) == (
        "scann_hip_index *index, const float *queries, uint32_t nq, uint32_t q_stride, uint32_t q_dim, uint32_t k, "
        "uint32_t depth, float lambda, const scann_hip_search_opts *opts, uint32_t *out_idx, float *out_dist, "
        "uint32_t *out_count")
    m = re.search(r"scann_hip_search_crowded_md\s*\(([^;]*?)\)\s*;", decl, flags=re.S)
    assert " ".join(m.group(1).split()) == (
        "scann_hip_index *index, const float *queries, uint32_t nq, uint32_t q_stride, uint32_t q_dim, uint32_t k, "
        "uint32_t depth, const uint32_t *limits, uint32_t n_limits, const scann_hip_search_opts *opts, "
        "uint32_t *out_idx, float *out_dist, uint32_t *out_count")
    text = " ".join(re.sub(r"^\s*\*", " ", hdr, flags=re.M).split())
    for phrase in ("CrowdingMultidimensional::apply(search(query, depth), k)",
                   "MmrDiversifier::new(lambda).apply(search(query, depth), k, sim)",
                   "n_limits != n_dims -> InvalidArgument", "n_dims * min(k, depth) > 6144 -> Unimplemented",
                   "depth > SCANN_HIP_MMR_MAX_DEPTH -> Unimplemented", "NaN -> InvalidArgument",
                   "starting from f32::MIN"):
        assert phrase in text, phrase
    assert "MmrDiversifier, a per-query k" not in text          # the old "Not built" sentence is gone
    design = _read(os.path.join(ROOT, "DESIGN.md"))
    assert "3.3e" in design and "crowd_md_kernel" in design and "mmr_kernel" in design
    assert "mmr.hip" in build.SOURCES and "pair.h" in build.HEADERS and "mmr.h" in build.HEADERS

"""tests/partition_cases.py against the switches of the search front end: every class on both sides of every switch
is hit by a case, the issue's (L, P) list is present, and no case asks for more LDS than a compute unit has -- but the
cases that record the launcher's fix, whose select-path request does.  The mirror's constants are read back from the
sources.  No GPU."""
import os
import re

import numpy as np

from tests import partition_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scann_rust_amd", "csrc")


def _classes_of_partition_cases():
    return {c.name: PC.classify(c.L, c.P, c.dim, PC.NQ) for c in PC.CASES}


def _search_calls():
    """(case, m, stages, classes) of every search call the GPU test makes"""
    out = []
    for s in PC.SEARCHES:
        sizes = PC.leaf_sizes(s.name, s.L, s.leaves, s.avg)
        ms = PC.max_stream(sizes, s.P)
        for m in s.ms:
            cl = PC.classify(s.L, s.P, s.dim, s.nq, m=m, ms=ms, wide=s.wide, exact_scan=s.mode == "partitioned")
            for stages in (True, False):
                out.append((s, m, stages, dict(cl, final=PC.final_select(ms, s.P, m, stages))))
    return out


def test_constants_are_the_sources():
    def const(path, name):
        text = open(os.path.join(CSRC, path), encoding="utf-8").read()
        m = re.search(r"constexpr \w+ %s = ([^;]+);" % name, text)
        assert m, name
        return eval(m.group(1).replace("u", "").replace("kSelectThreads", str(PC.SELECT_THREADS)), {})   # "4u << 20", "160 * 1024"
    assert const("launch.h", "kMaxLdsBytes") == PC.LDS_MAX
    for name, want in (("kMaxLeavesSelect", PC.MAX_LEAVES), ("kMaxPartitionsToSearch", PC.MAX_P),
                       ("kSelectThreads", PC.SELECT_THREADS), ("kDecodeStage", PC.DECODE_STAGE),
                       ("kSmallBatch", PC.SMALL_BATCH), ("kSmallMaxCandidates", PC.SMALL_MAX_CANDIDATES),
                       ("kSmallMaxStream", PC.SMALL_MAX_STREAM), ("kWideBatch", PC.WIDE_BATCH),
                       ("kWideMaxCandidates", PC.WIDE_MAX_CANDIDATES), ("kWideMaxStream", PC.WIDE_MAX_STREAM),
                       ("kFusedChunk", PC.FUSED_CHUNK), ("kFusedMaxWgs", PC.FUSED_MAX_WGS)):
        assert const("txh.h", name) == want, name
    assert const("txh_prefilter.hip", "kRefineTablesMax") == PC.REFINE_TABLES_MAX
    txh = open(os.path.join(CSRC, "txh.hip"), encoding="utf-8").read()
    assert re.search(r"kSelRegCaps\[3\] = \{8192, 13312, %d\}" % PC.SEL_REG_CAP, txh)
    # the launcher's expression, as select_lds restates it, and its two thread counts
    assert "(size_t)(n2 + p_pow2) * sizeof(uint64_t) + (size_t)lcfg.bins * 4 + (size_t)lcfg.list * 8 + 48 * 8 + 64 * 4" in txh
    assert "dim3(p2 && ix.L <= 4096 ? 256u : kSelectThreads)" in txh
    assert "if (lds_of(p2) + static_bytes > kMaxLdsBytes) p2 = 0;" in txh
    common = open(os.path.join(CSRC, "common.h"), encoding="utf-8").read()
    assert "c.bins = n <= 4096u ? 1024u : kSelBinsMax;" in common and "c.list = n <= 4096u ? 256u : kSelListMax;" in common


def test_the_lds_arithmetic_of_the_staged_launch():
    assert PC.select_lds(16384, 0) == 156288 and PC.select_lds(16384, 512) == 160384 <= PC.LDS_MAX
    assert PC.select_lds(8193, 1024) == 164480 > PC.LDS_MAX and PC.select_lds(16384, 4096) == 189056
    assert PC.staged_select(8193, 512) == (512, 1024, 160384)
    assert PC.staged_select(8193, 513) == (0, 1024, 156288) == PC.staged_select(16384, 4096)
    assert PC.staged_select(8192, 2048) == (2048, 1024, 8192 * 8 + 2048 * 8 + 4096 * 4 + 1024 * 8 + 640)
    assert PC.staged_select(4096, 1000) == (1024, 256, (4096 + 1024) * 8 + 1024 * 4 + 256 * 8 + 640)
    assert PC.staged_select(4096, 1025) == (0, 1024, 4096 * 8 + 1024 * 4 + 256 * 8 + 640)
    # every documented (L, P) fits after the fix; the select path alone is dropped, and only in one corner
    dropped = set()
    for L in (1, 2, 1000, 4096, 4097, 8192, 8193, 12000, 16384):
        for P in (1, 2, 100, 512, 513, 1024, 1025, 2048, 2049, 4096):
            p2, threads, lds = PC.staged_select(L, min(P, L))
            assert lds + PC.SELECT_STATIC <= PC.LDS_MAX, (L, P)
            if PC.wants_select(L, min(P, L)) and not p2:
                dropped.add((L > 8192, min(P, L) > 512))
    assert dropped == {(True, True)}


def test_the_issues_shapes_are_in_the_table():
    have = {(c.L, c.P) for c in PC.CASES}
    assert {(4096, 1000), (2500, 700), (3000, 1500), (4096, 4096), (4097, 10), (5000, 2048), (5000, 2049), (8192, 600),
            (8193, 512), (8193, 513), (16384, 1), (16384, 4096)} <= have
    assert {c.dim for c in PC.CASES} == {16, 19, 6}
    by = {s.name: s for s in PC.SEARCHES}
    for name, L, P, nq in (("staged-5000x600", 5000, 600, 33), ("small-4096x600", 4096, 600, 8),
                           ("small-4096x300", 4096, 300, 8), ("wide-4096x300", 4096, 300, 2),
                           ("staged-16384x512", 16384, 512, 33), ("staged-16384x4096", 16384, 4096, 5)):
        assert (by[name].L, by[name].P, by[name].nq) == (L, P, nq)
    assert {s.dim for s in PC.SEARCHES if s.L == 4096 and s.P == 300} == {16, 64, 65, 100}
    assert {s.leaves for s in PC.SEARCHES} == {"uniform", "half-empty", "skewed"}
    assert len(by["staged-5000x600"].ms) == 2
    assert {c.centroids for c in PC.CASES} == {"uniform", "dup4", "identical"}
    assert PC.NQ % 4 and PC.NQ % 16
    # sizes: the largest index is about 32k x 16, the dim cases about 12k x 100
    for c in list(PC.CASES) + list(PC.SEARCHES) + list(PC.SHARDED):
        n = int(PC.leaf_sizes(c.name, c.L, c.leaves, c.avg).sum())
        assert 0 < n * c.dim <= 36000 * 16 if c.dim <= 16 else n <= 13000, (c.name, n)


def test_both_sides_of_every_switch_are_hit():
    part = list(_classes_of_partition_cases().values())
    calls = [cl for _, _, _, cl in _search_calls()]
    everything = part + calls

    def seen(key, among=everything):
        return {cl[key] for cl in among}
    assert seen("threads", part) == {256, 1024}
    assert seen("select", part) == {"select", "full-sort"}
    # the full sort beyond the 64 keys the suite had: 4096, 8192 and 16384 keys
    full = {PC.next_pow2(c.L) for c in PC.CASES if PC.classify(c.L, c.P, c.dim, PC.NQ)["select"] == "full-sort"}
    assert {4096, 8192, 16384} <= full
    assert seen("per>1", part) == {False, True} and {1, 2, 3, 4} <= seen("per", part)
    # per > 1 on both thread counts and on both paths
    assert {(cl["threads"], cl["select"]) for cl in part if cl["per>1"]} == {(256, "select"), (1024, "select"), (1024, "full-sort")}
    assert seen("sel_cfg") == {"small", "large"} == seen("sel_cfg", part)
    assert seen("scoring") == {"inline", "kernel"}
    assert {cl["sel_cfg"] for cl in calls if cl["scoring"] == "inline"} == {"small"}       # (L <= 4096 is its condition)
    small_batch = [(s, cl) for s, _, _, cl in _search_calls() if s.nq <= PC.SMALL_BATCH]
    assert max(s.L for s, cl in small_batch if cl["scoring"] == "inline") == PC.INLINE_MAX_LEAVES
    assert any(s.L > PC.INLINE_MAX_LEAVES and cl["pipeline"] == "Staged" for s, cl in small_batch)   # ... and past it
    assert seen("centroid-path") == {None, "float4", "scalar"}
    assert seen("inline-chunks") == {None, "whole", "tail"}
    assert {s.dim for s in PC.SEARCHES if s.nq <= 16} >= {64, 65, 100}                     # a whole chunk, one past, a tail
    assert seen("decode", calls) == {"staged", "global"}
    assert seen("refine-tables") == {True, False}
    assert seen("pipeline", calls) == {"Staged", "Small", "Wide"}
    assert {cl["decode"] for cl in calls if cl["pipeline"] == "Staged"} == {"staged", "global"}
    # the Small pipeline beyond kDecodeStage leaves: the three-launch form; and the one-launch form beside it
    assert {(cl["decode"], cl["fused"]) for cl in calls if cl["pipeline"] == "Small"} >= {("global", False), ("staged", False), ("staged", True)}
    assert seen("worklist-leaves-per-thread") == {None, "one", "many"}
    # both final selects decode through more than kDecodeStage key bases
    assert {cl["final"] for cl in calls if cl["pipeline"] == "Staged" and cl["decode"] == "global"} == \
        {"select_rerank_kernel", "select_regs_kernel"}


def test_the_search_cases_take_the_pipeline_their_name_says():
    for s, m, stages, cl in _search_calls():
        assert cl["pipeline"].lower() == s.name.split("-")[0], (s.name, cl["pipeline"])
    s = next(s for s in PC.SEARCHES if s.name == "staged-5000x600")
    ms = PC.max_stream(PC.leaf_sizes(s.name, s.L, s.leaves, s.avg), s.P)
    assert [PC.final_select(ms, s.P, m, False) for m in s.ms] == ["select_rerank_kernel", "select_regs_kernel"]
    assert PC.classify(s.L, s.P, s.dim, s.nq, m=300, ms=ms)["per"] == 1 and PC.staged_select(s.L, s.P)[1] == 1024
    sharded = [PC.classify(sh.L, sh.P, sh.dim, sh.nq, m=sh.ms[0], ms=1, sharded=True) for sh in PC.SHARDED]
    assert [(cl["pipeline"], cl["threads"], cl["per"]) for cl in sharded] == [("Staged", 1024, 1), ("Staged", 256, 4)]


def test_no_case_asks_for_more_lds_than_a_compute_unit_has():
    expecting_fix = set()
    for c in PC.CASES:
        cl = PC.classify(c.L, c.P, c.dim, PC.NQ)
        assert cl["lds"] + PC.SELECT_STATIC <= PC.LDS_MAX, c.name
        assert (cl["lds-wanted"] > PC.LDS_MAX) == c.fix, c.name
        if c.fix:
            expecting_fix.add((c.L, c.P))
            assert cl["select"] == "full-sort" and PC.wants_select(c.L, c.P)
    assert expecting_fix == {(8193, 513), (16384, 4096)}
    for s, m, stages, cl in _search_calls():
        # (the Small pipeline's one-launch form adds small_fused_kernel's 80 272 static bytes: launch() accounts for them)
        assert cl["lds"] + (80272 if cl["fused"] else 0) <= PC.LDS_MAX, s.name
        assert (cl["lds-wanted"] > PC.LDS_MAX) == (s.name == "staged-16384x4096"), s.name


def test_the_families_are_what_they_say():
    c = next(c for c in PC.CASES if c.centroids == "dup4" and c.L == 2500)
    cen = PC.centroids(c.name, c.L, c.dim, c.centroids)
    _, inverse, counts = np.unique(cen, axis=0, return_inverse=True, return_counts=True)
    assert set(counts.tolist()) == {4}
    ids = np.flatnonzero(np.ravel(inverse) == np.ravel(inverse)[0])
    assert ids.size == 4 and np.diff(ids).max() > 4                                     # scattered, not adjacent
    assert len(np.unique(PC.centroids("x", 100, 16, "identical"), axis=0)) == 1
    q = PC.queries(c.name, PC.NQ, c.dim, "edges", cen)
    assert np.array_equal(q[PC.HIT_QUERY], cen[c.L // 2]) and np.isnan(q[PC.NAN_QUERY]).sum() == 1
    with np.errstate(over="ignore"):
        assert np.isinf(q[PC.INF_QUERY, c.dim // 2] * q[PC.INF_QUERY, c.dim // 2])
    for L in (2500, 16384):
        half = PC.leaf_sizes("h", L, "half-empty", 2)
        assert 0.4 < (half == 0).mean() < 0.6 and half[0] == 0 and half[1] > 0 and half[2] == 0
        skew = PC.leaf_sizes("s", L, "skewed", 3)
        assert skew.max() == skew[L // 3] and 0.2 < skew.max() / skew.sum() < 0.45 and np.delete(skew, L // 3).max() <= 3
    rows, assign = PC.rows_and_assign("r", cen, PC.leaf_sizes("r", c.L, "uniform", 3))
    assert np.array_equal(np.bincount(assign, minlength=c.L), PC.leaf_sizes("r", c.L, "uniform", 3))
    assert np.abs(rows - cen[assign]).max() <= 0.05 + 1e-6


def test_design_states_the_same_arithmetic():
    """DESIGN.md "Limits" and 3.0c: the byte counts and the edge they state are the ones computed here"""
    text = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    limits = text[text.index("## 7. Limits"):]
    limits = limits[:limits.index("`search_with_filter(Some(f))`")]

    def spaced(n):
        return "{:,}".format(n).replace(",", " ")
    edge = next(P for P in range(1, PC.MAX_P + 1) if PC.select_lds(PC.MAX_LEAVES, PC.next_pow2(P)) > PC.LDS_MAX)
    assert edge == 513
    assert "`num_partitions ≤ %d`" % PC.MAX_LEAVES in limits and "`partitions_to_search ≤ %d`" % PC.MAX_P in limits
    assert spaced(PC.select_lds(PC.MAX_LEAVES, 0)) in limits and "from `P = %d`" % edge in limits
    assert "tests/test_gpu_partition_front.py" in limits
    section = text[text.index("### 3.0c"):]
    section = section[:section.index("\n### 3.1 ")]
    for n in (PC.select_lds(PC.MAX_LEAVES, 0), PC.select_lds(8193, PC.next_pow2(edge)), PC.select_lds(PC.MAX_LEAVES, PC.MAX_P)):
        assert spaced(n) in section, n
    for name in ("tests/partition_cases.py", "tests/test_partition_cases.py", "tests/test_gpu_partition_front.py"):
        assert name in section
    for c in PC.CASES[:12]:
        assert "(%d, %d)" % (c.L, c.P) in section, c.name

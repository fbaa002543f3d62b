"""tests/high_dim_cases.py against the numbers the launchers' comments and DESIGN.md state: the byte counts, the
edges and the ceilings are recomputed from the formulas, and every edge must be hit from both sides by the dim list of
the test that runs the kernel.  No GPU."""
import os
import re

from tests import high_dim_cases as HC

KB = 1024
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_byte_counts_at_the_dims_the_kernels_are_known_by():
    assert HC.stream_lds(4096) == 167936 and HC.stream_lds(896) == 64 * KB and HC.stream_lds(3968) == 160 * KB
    assert HC.generic_lds(2044) == 65440 and HC.generic_lds(2048) == 65568 and HC.generic_lds(5116) == 163744
    assert HC.quant_lds(2048, 9) == 64 * KB and HC.quant_lds(2048, 2) == 16 * KB and HC.quant_lds(6144, 9) == 48 * KB
    assert [HC.exact_qpt(d) for d in (96, 512, 768, 1024, 1536, 2048, 4096)] == [16, 6, 4, 2, 2, 2, 2]
    assert HC.exact_lds(2048) == 64 * KB and HC.exact_lds(4096) == 128 * KB and HC.exact_lds(768) == 48 * KB
    assert HC.centroid_lds(4096, 4) == 64 * KB and HC.centroid_lds(1024, 16) == 64 * KB
    assert HC.centroid_qt(1024, 8192, 1024) == 16 and HC.centroid_qt(1024, 8192, 1008) == 4
    assert HC.centroid_qt(2564, 8192, 1024) == 4 and HC.centroid_qt(2560, 8192, 1024) == 16
    assert HC.assign_lds(1024) == 64 * KB and HC.assign_lds(2560) == 160 * KB and HC.assign_lds(2564) == 82048
    assert HC.assign_lds(4096) == 128 * KB and HC.assign_avx_lds(5120) == 160 * KB
    assert {d: HC.delta_qt(d) for d in HC.DELTA_QT} == HC.DELTA_QT
    assert [HC.delta_qt(d) for d in (24, 2048, 2052, 6144, 20000)] == [8, 6, 5, 2, 1]
    assert max(HC.delta_lds(d) for d in range(4, 8192, 4)) <= HC.LDS_ATTR       # never needs the attribute
    assert HC.small_scan_lds(4096, 64, 16) == 20 * KB


def test_ceilings():
    assert HC.CEILING == {"bf f32": 5116, "bf quantized": 20480, "partitioned": 5100, "centroid scores": 10240,
                          "assign nearest": 5120, "k-means assign, AVX2 order": 5120, "tree / hasher, batched": 10240,
                          "lut_from_query": 40960, "delta scan": 38912, "mmr, depth 2048": 34304}
    assert all(c >= 4096 for c in HC.CEILING.values()), "an entry point stops below dim 4096"
    # the delta scan and the MMR stage reach further than any base search: their rows of the table say "the base's"
    assert min(HC.CEILING["delta scan"], HC.CEILING["mmr, depth 2048"]) > HC.CEILING["bf quantized"]
    assert HC.expected_above("bf f32") == 8 and HC.expected_above("tree / hasher, batched", "centroid scores") == "ok"
    # the one dim above them that the GPU test runs lies above every ceiling of a kernel that stages 8 rows
    assert all(HC.ABOVE > HC.CEILING[k] for k in ("bf f32", "partitioned", "assign nearest", "k-means assign, AVX2 order"))
    assert HC.stream_lds(HC.ABOVE) > HC.LDS_MAX and HC.quant_lds(HC.ABOVE, 9) <= HC.LDS_MAX < 32 * HC.ABOVE


def test_every_edge_is_straddled_by_the_dim_list_of_its_kernel():
    for kernel, what, at, nxt, holds in HC.EDGES:
        dims = HC.DIMS_OF[kernel]
        assert at in dims and nxt in dims, "%s (%s): %d / %d not both in %s" % (kernel, what, at, nxt, dims)
        assert holds(at) and not holds(nxt), "%s (%s): the edge is not between %d and %d" % (kernel, what, at, nxt)
        # the edge dim is the LAST dim on its side among the dims the kernel's vector paths accept
        step = 8 if "quant" in kernel else 16 if "<16>" in kernel else 4
        if what != "4 -> 2 quads":
            assert not holds(at + step), (kernel, what)
    for kernel, dim, lds in HC.EXACTLY_64K:
        assert lds(dim) == HC.LDS_ATTR and dim in HC.DIMS_OF[kernel], (kernel, dim)
    # 4 -> 2 quads happens between the two common sizes; 2 quads is the clamp from dim 2048 (the formula gives 0)
    assert HC.exact_qpt(1020) == 2 and (48 * KB) // (2048 * 4) // 8 * 2 == 0


def test_dim_lists():
    for dims in list(HC.DIMS_OF.values()) + [HC.MMR_DIMS, HC.RERANK_DIMS]:
        assert all(d <= 4100 for d in dims)
    for d in HC.COMMON:
        assert d in HC.ALL_DIMS and d in HC.BF_F32_DIMS
    assert HC.UNALIGNED % 4 and HC.stride_of(HC.UNALIGNED) == HC.UNALIGNED
    assert all(HC.UNALIGNED in dims for dims in (HC.BF_F32_DIMS, HC.BF_QUANT_DIMS, HC.PARTITIONED_DIMS, HC.MMR_DIMS))
    assert all(HC.stride_of(d) % 4 == 0 and HC.stride_of(d) >= d for d in HC.ALL_DIMS if d != HC.UNALIGNED)
    assert set(HC.BATCHES) == {1, 3, 16, 17, 70}
    # which kernel a batch takes switches between 16 and 17 queries, and at the streaming kernel's ceiling
    assert HC.bf_pass_kernel(0, 3968, 3968, 16) == "bf_stream_kernel" == HC.bf_pass_kernel(2, 768, 768, 1)
    assert HC.bf_pass_kernel(0, 3972, 3984, 16) == "bf_generic_kernel" == HC.bf_pass_kernel(0, 768, 768, 17)
    assert HC.bf_pass_kernel(3, 768, 768, 1) == "bf_generic_kernel" == HC.bf_pass_kernel(0, 1027, 1027, 1)
    # subspace widths of the trained shapes
    dsub = sorted({dim // S for _, dim, _, S, _, _ in HC.TXH_SHAPES.values()} | {dim // S for _, dim, S in HC.AH_SHAPES.values()})
    assert dsub[0] == 12 and dsub[-1] == 256 and {12, 48, 128} <= {dim // S for _, dim, S in HC.AH_SHAPES.values()}
    assert all(dim % S == 0 and 1000 <= n <= 3000 and 6 <= L <= 16 for n, dim, L, S, _, _ in HC.TXH_SHAPES.values())
    assert {768, 1536, 4096} <= {dim for _, dim, _, _, _, res in HC.TXH_SHAPES.values() if not res}


def test_design_table_agrees_with_the_formulas():
    """DESIGN.md "Dimensionality ceilings": every ceiling the table states is the one computed here"""
    text = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    section = text[text.index("### Dimensionality ceilings") + 4:]
    section = section[:section.index("\n##")]
    rows = [r for r in section.splitlines() if r.startswith("|") and not r.startswith("|---")][1:]
    assert len(rows) >= 8
    stated = {}
    for r in rows:
        cells = [c.strip() for c in r.strip("|").split("|")]
        m = re.match(r"(\d+)", cells[-1].replace(" ", "").replace(",", ""))
        if m:
            stated[cells[0]] = int(m.group(1))
    want = {"brute force, f32 rows": HC.CEILING["bf f32"], "brute force, quantized rows": HC.CEILING["bf quantized"],
            "Partitioned mode": HC.CEILING["partitioned"], "`txh_partition`": HC.CEILING["centroid scores"],
            "`bf_assign_nearest`": HC.CEILING["assign nearest"], "`kmeans_lloyd`": HC.CEILING["assign nearest"],
            "tree / flat hasher, batched": HC.CEILING["tree / hasher, batched"],
            "`lut_from_query`, `adc_distances`, `encode`": HC.CEILING["lut_from_query"]}
    assert HC.CEILING["k-means assign, AVX2 order"] == HC.CEILING["assign nearest"]      # (one figure for kmeans_lloyd)
    for name, dim in want.items():
        assert stated.get(name) == dim, "DESIGN.md states %s for %s, the formulas give %d" % (stated.get(name), name, dim)
    cells = {r.strip("|").split("|")[0].strip(): r.strip("|").split("|")[-1].strip() for r in rows}
    for name in ("mutable search", "`search_mmr`, `search_crowded`"):        # no ceiling of their own below the base's
        assert cells[name] == "the base's", (name, cells[name])
    assert cells["tree / flat hasher, nq <= 16"] == "the batched one's"
    assert cells["`kmeans_init_pp`, `scalar_quantize_device`, `quantization_stats`"] == "none"

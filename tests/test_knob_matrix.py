"""CPU checks of tests/knob_matrix.py: the all-pairs rows cover every pair and are deterministic, the plan mirror names
every kernel on both index kinds, and the shapes of tests/test_gpu_knob_matrix.py lie where the paths under test are
taken (the plan mirror of tests/helpers.py)."""
import collections

import pytest

import helpers as H
import knob_matrix as KM
import test_gpu_knob_matrix as G


@pytest.fixture(scope="module")
def shapes():
    """kind -> (stream, leaf sizes, P) of the GPU test's two indexes"""
    tree = G.Kind("txh", shapes_only=True)
    assert len(tree.leaves) == G.TREE_L and sum(tree.leaves) == G.N
    assert tree.stream == sum(sorted(tree.leaves)[-G.TREE_P:])   # (H.max_stream: the three largest leaves)
    return {"ah": (G.N, [G.N], 1), "txh": (tree.stream, tree.leaves, G.TREE_P)}


def test_rows_cover_every_pair_and_repeat():
    rows = KM.pairwise_rows(KM.SEED)
    assert rows == KM.pairwise_rows(KM.SEED)
    held = set()
    for r in rows:
        assert set(r) == {name for name, _ in KM.FACTORS}
        held |= KM.pairs_of(r)
    missing = KM.all_pairs() - held
    assert not missing, sorted(missing, key=repr)[:5]
    assert 36 <= len(rows) <= 70, len(rows)   # (36: the pairs of the two six-level factors)
    assert KM.matrix_rows() == rows + [dict(r) for r in KM.EXTRA_ROWS]


def test_rows_hold_only_declared_levels():
    levels = dict(KM.FACTORS)
    for r in KM.matrix_rows():
        for name, v in r.items():
            assert v in levels[name], (name, v)
        assert all(isinstance(v, str) for v in KM.row_env(r).values())


@pytest.mark.parametrize("kind", ["ah", "txh"])
def test_every_kernel_is_named_twice(shapes, kind):
    """or the GPU test could pass without ever leaving the gather scan"""
    stream, leaves, P = shapes[kind]
    named = collections.Counter(KM.expected_kernel(r, kind, stream, leaves, P) for r in KM.matrix_rows())
    assert set(named) == set(KM.KERNELS), named
    assert min(named.values()) >= 2, named


@pytest.mark.parametrize("kind", ["ah", "txh"])
def test_every_plan_field_takes_both_values(shapes, kind):
    """each boolean decision of the plan is taken both ways by some row (the flat-hasher-only ones on the flat hasher)"""
    stream, leaves, P = shapes[kind]
    plans = [KM.expected_plan(r, kind, stream, leaves, P) for r in KM.matrix_rows()]
    fields = ["no_threshold", "thr_tail", "sp_words", "select_direct", "select_regs", "use_i8", "i8_expand"]
    if kind == "ah":
        fields += ["sample_mfma", "sp_pairs64", "sp_bitmap", "fused"]
    for f in fields:
        assert {p[f] for p in plans} == {False, True}, (kind, f)
    assert {p["pipeline"] for p in plans} == {"small", "wide", "staged"}
    if kind == "ah":
        for f in ("sample_mfma", "sp_pairs64", "sp_bitmap", "fused"):
            assert sum(p[f] for p in plans) >= 2, (f, sum(p[f] for p in plans))
        assert any(p["sp_pairs64"] and not p["sp_bitmap"] for p in plans), "no row runs 64-pair items in the list form"
    else:   # flat hashers only (plan_txh_search), the one-launch small pipeline P = 1 only
        assert not any(p["sample_mfma"] or p["fused"] or p["sp_bitmap"] for p in plans)


def test_the_bitmap_form_follows_the_knob_alone(shapes):
    """sp_bitmap = 64-pair items, a flat hasher and the knob unset: the byte cap of plan_txh_search cannot bind at these
    shapes (the largest batch over every 1024-point range of the index stays far below it), and the sizes the GPU test
    compares with the handle's are those of the rows' batches"""
    stream, leaves, P = shapes["ah"]
    ranges = -(-G.N // KM.SP_RANGE64)
    assert -(-KM.NQ_MAX // 64) * 64 * ranges * 128 == 4 << 20 < KM.SURV_BYTES_MAX
    sizes = set()
    for r in KM.matrix_rows():
        for kind in ("ah", "txh"):
            st, lv, p = shapes[kind]
            plan = KM.expected_plan(r, kind, st, lv, p)
            assert plan["sp_bitmap"] == (kind == "ah" and plan["sp_pairs64"] and r["SCANN_HIP_SP_BITMAP"] is None)
            assert plan["sp_bitmap_bytes"] == (-(-r["nq"] // 64) * 64 * ranges * 128 if plan["sp_bitmap"] else 0)
            sizes.add(plan["sp_bitmap_bytes"])
            if r["SCANN_HIP_SP_BITMAP"] == "0":
                assert not plan["sp_bitmap"]
    assert len(sizes) >= 3, "the running maximum of the GPU test grows at least once"


@pytest.mark.parametrize("kind", ["ah", "txh"])
def test_shapes_take_the_paths_under_test(shapes, kind):
    stream, leaves, P = shapes[kind]
    st, scap = H.sample_plan(stream, P)
    assert scap > 4096
    for m in G.MS:
        assert H.sample_rank(m, st) <= KM.THR_TAIL_MAX_RANK      # with the line above: thr_tail is in force
        assert H.sample_rank(m, st) < m                          # a statistical bound
    assert H.plan_caps(stream, P, 2000)[2] > 4096                # the select reads its list in place
    assert H.plan_caps(stream, P, 600)[2] <= 4096                # the select runs in LDS
    assert 600 <= KM.SMALL_MAX_CANDIDATES and stream <= KM.SMALL_MAX_STREAM   # the small pipeline is eligible
    assert stream >= KM.WIDE_MIN_STREAM and stream >= 8 * 2000   # the wide pipeline is the default at nq <= 4
    assert P == 1 or sum(leaves) // len(leaves) >= 512
    assert sum(leaves) // len(leaves) >= 4096                    # leaves long enough for the sparse-MFMA takeover
    assert 600 * 128 <= stream < 2000 * 128                      # the prefilter "pays" at one m and not at the other
    for nq in (1, 4):
        for m in G.MS:
            assert KM.expected_plan(KM.default_row(nq=nq, m=m), kind, stream, leaves, P)["pipeline"] == "wide"
    assert KM.expected_plan(KM.default_row(nq=16, m=600), kind, stream, leaves, P)["pipeline"] == "small"
    assert KM.expected_plan(KM.default_row(nq=16, m=2000), kind, stream, leaves, P)["pipeline"] == "staged"
    assert KM.expected_plan(KM.default_row(nq=17, m=600), kind, stream, leaves, P)["pipeline"] == "staged"


def test_flat_hasher_plan_numbers():
    """the figures the flat hasher's shape was chosen for"""
    assert H.sample_plan(G.N, 1) == (16, 8196)
    assert H.plan_caps(G.N, 1, 2000)[:3] == (16, 214, 5808)
    assert H.plan_caps(G.N, 1, 600)[:3] == (16, 98, 3344)


def test_sequences():
    rows = KM.matrix_rows()
    one, two = KM.pass1_order(rows), KM.pass2_order(rows)
    assert sorted(one) == sorted(two) == list(range(len(rows)))
    assert two == KM.pass2_order(rows) and two != one
    assert KM.growth_steps(rows, one) >= 2 and KM.growth_steps(rows, two) == 0
    top = rows[two[0]]
    assert (top["nq"], top["m"]) == (KM.NQ_MAX, 2000)
    names = [d["name"] for d in KM.DISTURBANCES]
    assert len(rows) // 8 >= len(names) == len(set(names))   # every disturbance runs

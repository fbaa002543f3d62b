"""CPU tests of tests/build_model.py (the k-means++ seeding reference of tests/test_gpu_build.py) and of
scann_rust_amd.trainer.encode against the oracle's Codebook::encode on the inputs where an argmin and a strict '<'
part ways."""
import importlib.util
import os
import re

import numpy as np
import pytest

from oracle import pyoracle as orc
from scann_rust_amd import synth, trainer
from tests import build_model as BM
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the random stream ------------------------------------------------------------------------------------------
def test_splitmix_constants_match_the_library():
    """synth.splitmix64 is the stream km_splitmix (bf.hip) draws from: same increment and multipliers"""
    src = open(os.path.join(ROOT, "scann_rust_amd", "csrc", "bf.hip")).read()
    body = src[src.index("km_splitmix(uint64_t &s)"):]
    body = body[:body.index("}")]
    consts = [int(c, 16) for c in re.findall(r"0x([0-9A-Fa-f]{16})ull", body)]
    assert consts == [int(synth._GOLDEN), int(synth._M1), int(synth._M2)]
    assert ">> 30" in body and ">> 27" in body and ">> 31" in body
    # and a known answer of the generator itself (splitmix64 of seed 0: the published first outputs)
    z = synth.splitmix64(0, 0, 2)
    assert [int(v) for v in z] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4]


def test_stream_layout():
    first, rest = BM.stream(7, 1000, 4)
    z = [int(v) for v in synth.splitmix64(7, 0, 7)]
    assert first == z[0] % 1000
    assert rest == [(z[1] >> 11, z[2] % 1000), (z[3] >> 11, z[4] % 1000), (z[5] >> 11, z[6] % 1000)]


# ---- exact sums -------------------------------------------------------------------------------------------------
def test_exact_units():
    v = np.array([0.0, 2.0 ** -149, 3 * 2.0 ** -149, 2.0 ** -126, 1.0, 1.5, np.finfo(np.float32).max], np.float32)
    got = BM.exact_units(v)
    assert got[:4] == [0, 1, 3, 1 << 23]
    assert got[4] == 1 << 149 and got[5] == 3 << 148
    assert got[6] == ((1 << 24) - 1) << (127 - 23 + 149)
    rng = np.random.default_rng(1)
    w = (rng.uniform(0, 1, 200) * np.exp(rng.uniform(-80, 80, 200))).astype(np.float32)
    from fractions import Fraction
    assert all(Fraction(u, 1 << 149) == Fraction(float(x)) for u, x in zip(BM.exact_units(w), w))


def test_distances_follow_both_summation_orders():
    rng = np.random.default_rng(2)
    win = rng.uniform(-1, 1, (40, 19)).astype(np.float32)
    for avx, fn in ((False, orc.squared_l2_sequential), (True, orc.squared_l2_avx2)):
        d = BM.distances_to_row(win, 3, avx)
        assert d.dtype == np.float32 and d[3] == 0.0
        assert BM.same_bits(d, np.array([fn(win[i], win[3]) for i in range(40)], np.float32))
    # the two orders differ on these rows, so a swapped switch would show
    assert not BM.same_bits(BM.distances_to_row(win, 3, False), BM.distances_to_row(win, 3, True))


# ---- the band ---------------------------------------------------------------------------------------------------
def test_band_branches():
    md = np.array([0.0, 1.0, 0.0, 2.0, 1.0], np.float32)           # C = 0 1 1 3 4, T = 4
    u = lambda x: int(x * 2 ** 53)
    assert BM.band(md, u(0.2), 9)[0].tolist() == [1]               # thr 0.8
    assert BM.band(md, u(0.3), 9)[0].tolist() == [3]               # thr 1.2: row 2 adds nothing
    assert BM.band(md, u(0.9), 9)[0].tolist() == [4]
    # thr = 1 exactly: C(1) = 1 reaches it; a sum rounded down could also take row 3 (row 2 has min_d 0: excluded)
    rows, kind = BM.band(md, u(0.25), 9)
    assert rows.tolist() == [1, 3] and kind == "sampled"
    rows, kind = BM.band(np.zeros(5, np.float32), u(0.5), 3)
    assert rows.tolist() == [3] and kind == "zero-total"
    assert BM.band(np.array([1, np.inf, 2, np.inf], np.float32), u(0.5), 3)[0].tolist() == [1]
    rows, kind = BM.band(np.array([1, np.inf, np.nan], np.float32), u(0.5), 2)
    assert rows.tolist() == [2] and kind == "nan-total"


def test_band_contains_every_f64_evaluation_order():
    """The derivation of delta: whatever order a correctly rounded f64 evaluation sums in (a chain, numpy's pairwise
    tree, blocks of 256 then a chain), its pick lies in the band."""
    rng = np.random.default_rng(3)
    for trial in range(30):
        n = int(rng.integers(2, 5000))
        md = (rng.uniform(0, 1, n) * np.exp(rng.uniform(-30, 30, n))).astype(np.float32)
        md[rng.random(n) < 0.2] = 0.0
        if not md.any():
            continue
        u_int = int(rng.integers(1, 1 << 53))
        u = u_int * 2.0 ** -53
        rows, kind = BM.band(md, u_int, 0)
        assert kind == "sampled" and rows.size >= 1
        m64 = md.astype(np.float64)
        chain = np.cumsum(m64)
        picks = [int(np.argmax(chain >= u * chain[-1]))]
        T = float(np.sum(m64))                                      # pairwise tree
        pad = np.concatenate([m64, np.zeros(-n % 256)]).reshape(-1, 256)
        blocks = pad.sum(1)
        b = int(np.argmax(np.cumsum(blocks) >= u * T)) if (np.cumsum(blocks) >= u * T).any() else blocks.size - 1
        inner = (np.cumsum(blocks)[b - 1] if b else 0.0) + np.cumsum(pad[b])
        hit = np.flatnonzero(inner >= u * T)
        picks.append(b * 256 + int(hit[0]) if hit.size else None)
        for p in picks:
            assert p is None or p in rows.tolist(), (trial, p, rows)


@pytest.fixture(scope="module")
def seeded():
    cache = {}

    def get(name):
        if name not in cache:
            case = BM.seeding_case(name)
            win = BM.seeding_window(case)
            cache[name] = (case, win, BM.seeding_reference(win, case["k"], case["seed"], case["thr"]))
        return cache[name]

    yield get
    cache.clear()


@pytest.mark.parametrize("name", BM.SEEDING_CASES)
def test_every_band_of_the_gpu_inputs_holds_one_row(seeded, name):
    """The condition tests/test_gpu_build.py relies on: with one admissible row per pick, the GPU test demands
    equality.  An input with a wider band is replaced, the cap is not."""
    case, win, ref = seeded(name)
    assert len(ref) == case["k"]
    assert [r["rows"].size for r in ref] == [1] * case["k"], [(r["kind"], r["rows"].tolist()) for r in ref]
    assert ref[0]["kind"] == "first"


def test_bands_take_the_expected_branches(seeded):
    kinds = lambda name: [r["kind"] for r in seeded(name)[2]]
    assert set(kinds("clustered")[1:]) == {"sampled"} and set(kinds("uniform-70000")[1:]) == {"sampled"}
    k = kinds("copies")
    assert k[1:25] == ["sampled"] * 24 and k[25:] == ["zero-total"] * 15      # 25 distinct rows, then the fallback
    case, win, ref = seeded("copies")
    assert len({win[r["followed"]].tobytes() for r in ref[:25]}) == 25
    assert kinds("more-seeds-than-rows")[5:] == ["zero-total"] * 4
    assert set(kinds("all-zero")[1:]) == {"zero-total"} and set(kinds("all-equal")[1:]) == {"zero-total"}
    assert kinds("one-row") == ["first", "zero-total", "zero-total"]
    assert "inf-total" in kinds("overflow") and "sampled" in kinds("overflow")
    assert set(kinds("nan")[1:]) == {"nan-total"}
    case, win, ref = seeded("scaled-70")
    d = BM.distances_to_row(win, ref[0]["followed"], False)
    assert 0 < d[d > 0].min() < np.finfo(np.float32).tiny           # subnormal minimum distances
    # the picks of the sampled branch spread: no seed twice (a picked row has min_d 0 and is never admissible again)
    f = [r["followed"] for r in seeded("clustered")[2]]
    assert len(set(f)) == len(f)


def test_model_follows_given_picks(seeded):
    """Fed its own picks as centres the model returns the same bands; fed a wrong centre it still follows it, and the
    band it reports does not contain it (so the caller's comparison fails there and only there)."""
    case, win, ref = seeded("clustered")
    own = np.stack([win[r["followed"]] for r in ref])
    again = BM.seeding_reference(win, case["k"], case["seed"], case["thr"], picks=own)
    assert [r["rows"].tolist() for r in again] == [r["rows"].tolist() for r in ref]
    wrong = own.copy()
    other = (ref[3]["followed"] + 1) % case["n"]
    wrong[3] = win[other]
    res = BM.seeding_reference(win, case["k"], case["seed"], case["thr"], picks=wrong)
    assert res[3]["rows"].tolist() == ref[3]["rows"].tolist() and res[3]["followed"] == other
    assert [r["rows"].tolist() for r in res[:4]] == [r["rows"].tolist() for r in ref[:4]]


# ---- trainer.encode against Codebook::encode --------------------------------------------------------------------
@pytest.mark.parametrize("family", H.ENCODE_FAMILIES)
def test_trainer_encode_matches_oracle(family):
    cb, x = H.encode_inputs(family, 6, 16, 3, 300, seed=41)
    want = orc.encode_many(cb, x)
    assert np.array_equal(trainer.encode(cb, x), want)
    assert np.array_equal(trainer.encode(cb, x, chunk=7), want)
    if family == "equal":
        assert not want.any()
    if family == "nan-code":
        assert not (want[:, :4] == 0).any() and (want[:, 4] == 15).all() and (want[:, 5] == 0).all()
    if family == "nan-sub":
        assert not want[7].any()
    if family == "tiny":         # every squared difference is subnormal (a few bits of precision: many ties)
        assert orc.lut_from_query(cb, x[0]).max() < np.finfo(np.float32).tiny


def test_trainer_encode_known_answer():
    """sub-distances [1, NaN, 0.5]: strict '<' skips the NaN and takes code 2"""
    cb = np.array([[[1.0], [np.nan], [np.sqrt(0.5)]]], np.float32)
    x = np.zeros((1, 1), np.float32)
    assert orc.encode_many(cb, x).tolist() == [[2]]
    assert trainer.encode(cb, x).tolist() == [[2]]


def test_golden_fixture_unchanged_by_the_encode_fix():
    """Every fixture is built through trainer.encode; regenerate one index and compare it with the file."""
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "tests", "golden",
                                                                              "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    rows, queries, ix = mg.build_case(2, 96, 24)
    g = np.load(os.path.join(ROOT, "tests", "golden", "txh_seed2_d96_S24.npz"))
    for key in ("centers", "leaf_off", "leaf_ids", "codebook", "codes"):
        assert np.array_equal(np.asarray(ix[key]), g[key]), key
    assert np.array_equal(ix["codes"], orc.encode_many(ix["codebook"], rows[ix["leaf_ids"]]
                                                       - ix["centers"][np.repeat(np.arange(mg.L), np.diff(ix["leaf_off"]))]))

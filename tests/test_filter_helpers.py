"""CPU checks of the allow-list helpers of tests/helpers.py: the sample-plan mirror of csrc/txh.h and the allow-set
families that tests/test_gpu_filters.py feeds to the kernels."""
import numpy as np
import pytest

from tests import helpers as H


def test_sample_plan_mirror_worked_numbers():
    """plan_txh_search's numbers for a flat hasher of 80 000 rows at m = 250 (st 16, J 65: the prefilter's list of
    4 cap + 16384 survivors is a third of the stream) and for the 1M-row hashers at m = 5000 (10^6 rows: st 31, J 259)"""
    assert H.sample_stride(80000) == 16 and H.sample_plan(80000, 1) == (16, 5004)
    assert H.plan_caps(80000, 1, 250) == (16, 65, 2576, 26688)
    st, j, cap, cap32 = H.plan_caps(1 << 20, 1, 5000)
    assert (st, j) == (37, 227) and cap32 == 4 * cap + 16384
    st, j, cap, cap32 = H.plan_caps(1000000, 1, 5000)
    assert (st, j, cap32) == (31, 259, 67380)
    # short streams: 4096 samples; a bound of rank m (no statistics) once m / st is small
    assert H.sample_stride(4096) == 1 and H.sample_stride(20000) == 5
    assert H.sample_rank(250, 5) == 116 and H.sample_rank(0, 3) == 0 and H.sample_rank(3, 1) == 3
    # the stride grows until the sample fits its capacity
    st, scap = H.sample_plan(1 << 24, 64)
    assert scap <= H.SAMPLE_TARGET and st >= (1 << 24) // H.SAMPLE_TARGET
    assert H.wide_group(80000, 250) == 8 and H.wide_group(80000, 8192) == 4 and H.wide_group(1 << 21, 250) == 64
    assert H.wide_group(1000, 250) == 1


def _tree(n=5000, L=7, seed=3):
    rng = np.random.default_rng(seed)
    sizes = rng.multinomial(n, np.ones(L) / L)
    off = np.zeros(L + 1, np.int64)
    off[1:] = np.cumsum(sizes)
    return off, rng.permutation(n).astype(np.uint32)


@pytest.mark.parametrize("fam", H.FILTER_FAMILIES)
def test_allow_families(fam):
    off, ids = _tree()
    n, k, m, st = int(off[-1]), 10, 200, 3
    tokens = np.array([[2, 0, 5], [1, 2, 3]])
    rng = np.random.default_rng(0)
    topk = [rng.choice(n, k, replace=False) for _ in range(2)]
    topm = [rng.choice(n, m, replace=False) for _ in range(2)]
    words, cap = H.allow_family(fam, off, ids, tokens, k, m, st, 1, topk=topk, topm=topm)
    again = H.allow_family(fam, off, ids, tokens, k, m, st, 1, topk=topk, topm=topm)
    assert np.array_equal(words, again[0]) and cap == again[1]            # deterministic
    assert words.dtype == np.uint64 and words.size == max(1, -(-cap // 64))
    a = H.allowed_ids(words, cap, n)
    assert np.all(a < min(cap, n)) and np.all(np.diff(a) > 0)
    probed0 = ids[np.concatenate([np.arange(off[l], off[l + 1]) for l in tokens[0]])]
    want = {"empty": 0, "one": 1, "k-1": k - 1, "m-1": m - 1, "m": m, "m+1": m + 1, "cap0": 0, "cap1": 1, "cap63": 63,
            "cap64": 64, "cap65": 65, "cap-n-1": n - 1, "cap-n": n, "cap-over": n}
    if fam in want:
        assert a.size == want[fam]
    if fam in ("one", "k-1", "m-1", "m", "m+1"):
        assert np.isin(a, probed0).all()
    if fam == "one-leaf":
        assert np.array_equal(np.sort(ids[off[2]:off[3]]), a)
    if fam == "unprobed":
        probed = ids[np.concatenate([np.arange(off[l], off[l + 1]) for l in (0, 1, 2, 3, 5)])]
        assert not np.isin(a, probed).any() and a.size == n - probed.size
    if fam in ("not-topk", "not-topm"):
        drop = np.concatenate(topk if fam == "not-topk" else topm)
        assert not np.isin(a, drop).any() and a.size == n - np.unique(drop).size
    if fam in ("sampled", "unsampled"):
        s = np.sort(ids[H.sampled_rows(off, st)])
        assert np.array_equal(a, s) if fam == "sampled" else (a.size == n - s.size and not np.isin(a, s).any())
    if fam == "wide-one-per-group":
        g = H.wide_group(probed0.size, m)
        assert a.size == len(range(g // 2, probed0.size, g))
    if fam == "wide-one-group":
        assert 1 <= a.size <= H.wide_group(probed0.size, m)
    if fam[0] == "f":
        f = float(fam[1:]) / 100.0
        assert abs(a.size - f * n) <= 5 * np.sqrt(f * n) + 2
    if fam.startswith("cap") and cap % 64:
        assert words[-1] >> np.uint64(cap % 64) != 0          # stray bits past the capacity
    if fam == "prefix":
        assert np.array_equal(a, np.arange(0, cap, 2))


def test_masked_words_and_bitmaps():
    words = np.full(2, np.uint64(0xFFFFFFFFFFFFFFFF))
    assert np.array_equal(H.allowed_ids(words, 65, 100), np.arange(65))
    assert np.array_equal(H.allowed_ids(words, 128, 70), np.arange(70))
    m = H.masked_words(words, 65, 200)
    assert m.size == 4 and int(m[0]) == 2 ** 64 - 1 and int(m[1]) == 1 and not m[2:].any()
    w, cap = H.words_of([0, 63, 64, 130], 131)
    assert cap == 131 and w.size == 3 and list(H.allowed_ids(w, cap, 200)) == [0, 63, 64, 130]
    assert H.words_of([], 0)[0].size == 1

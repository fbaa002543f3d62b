"""CPU checks of the integer-sample filter bound (tests/sample_bound_model.py): for every rank J the tail kernel can
take, the collected set holds every sample at or under the J-th smallest f32 key, the published bound IS that key
unless the list floods, and a flooded bound is at or above it."""
import numpy as np
import pytest

import sample_bound_model as M

J_MAX = 384          # txh.h kThrTailMaxRank
NS_SMALL = 5004      # the smallest sample the tail kernels take (scap > 4096)
NS_REFERENCE = 32259  # the sample of the 1M x 128 flagship run (stride 32)


def _check_all_ranks(smp, flood_allowed, what):
    order = np.sort(smp.keys)
    floods = 0
    for J in range(1, J_MAX + 1):
        want = int(order[J - 1])
        got, sel, flooded = M.tail16_bound(smp, J)
        w = "%s J=%d" % (what, J)
        if want == M.KEY_MAX:   # fewer than J present samples
            assert got == M.KEY_MAX, w
            continue
        if sel is not None:
            need = np.flatnonzero(smp.keys <= np.uint64(want))
            assert np.isin(need, sel).all(), w + ": a sample under the J-th key was not collected"
        if flooded:
            floods += 1
            assert flood_allowed, w + ": the list flooded (%d collected)" % (sel.size if sel is not None else -1)
            assert got >= want, w
        else:
            assert got == want, w
    return floods


@pytest.mark.parametrize("S", [8, 24, 32, 64])
@pytest.mark.parametrize("family", M.FAMILIES)
def test_every_rank(family, S):
    ns = NS_REFERENCE if family == "uniform" else NS_SMALL
    t = M.family_table(family, S, 1)
    smp = M.Sample(t, M.family_codes(ns, S, 2))
    assert smp.scale > 0.0
    if family == "bias":   # a tie family in f32: see sample_bound_model.FLOOD_ALLOWED
        assert np.unique(smp.d).size <= 64
    _check_all_ranks(smp, family in M.FLOOD_ALLOWED, "%s S%d" % (family, S))


@pytest.mark.parametrize("S", [8, 32])
def test_uniform_tables_collect_little(S):
    """reference sizes, uniform tables: the list never comes near its capacity"""
    smp = M.Sample(M.family_table("uniform", S, 3), M.family_codes(NS_REFERENCE, S, 4))
    for J in (1, 133, 259, J_MAX):
        _, sel, flooded = M.tail16_bound(smp, J)
        assert not flooded and sel.size <= M.LIST


def test_duplicated_rows_do_flood():
    """the flood branch is exercised: nine samples in ten carry one code row, thousands of keys tie on the distance"""
    S = 32
    codes = M.family_codes(NS_SMALL, S, 2)
    codes[np.arange(NS_SMALL) % 10 != 0] = codes[1]
    smp = M.Sample(M.family_table("uniform", S, 1), codes)
    assert _check_all_ranks(smp, True, "duplicates") > 0


@pytest.mark.parametrize("share", [0.5, 0.02, 0.001])
def test_rejected_samples(share):
    """an allow-bitmap rejects most samples (0xFFFF): absent ones never count, too few present ones give no bound"""
    S = 32
    codes = M.family_codes(NS_SMALL, S, 5)
    present = np.random.default_rng(6).random(NS_SMALL) < share
    smp = M.Sample(M.family_table("uniform", S, 7), codes, present)
    _check_all_ranks(smp, False, "present %.3f" % share)


@pytest.mark.parametrize("kind", ["nan", "inf", "negative", "flat"])
def test_unquantised_tables_take_the_f32_passes(kind):
    """scale = 0: the bound is threshold_tail_kernel's, flood case included"""
    S = 24
    t = M.family_table("uniform", S, 8)
    if kind == "nan":
        t[3, 5] = np.nan
    elif kind == "inf":
        t[3, 5] = np.inf
    elif kind == "negative":
        t[3, 5] = -1.0
    else:
        t[:] = 0.25
    codes = M.family_codes(NS_SMALL, S, 9)
    smp = M.Sample(t, codes)
    assert smp.scale == 0.0
    for J in (1, 2, 133, 259, J_MAX):
        got, sel, flooded = M.tail16_bound(smp, J)
        assert sel is None
        assert (got, flooded) == M.tail32_bound(M.distances(t, codes), None, J)
        if not flooded:
            assert got == smp.reference(J)
    if kind == "flat":
        assert M.tail16_bound(smp, 133)[2], "an all-equal table floods the f32 list"


def test_margin_is_needed():
    """mutation: a collect limit without the quantisation margin (qlim = P) loses samples under the J-th key"""
    S, misses = 32, 0
    smp = M.Sample(M.family_table("uniform", S, 10), M.family_codes(NS_REFERENCE, S, 11))
    order = np.sort(smp.keys)
    for J in range(1, J_MAX + 1, 7):
        P = M._jth(smp.kept16, J, M.ABSENT16)
        need = np.flatnonzero(smp.keys <= order[J - 1])
        misses += int((smp.u[need] > P).any())
    assert misses > 0

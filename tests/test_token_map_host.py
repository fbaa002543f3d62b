"""Tag filters, the parts that need no GPU: the token-map and block-combination symbols (exported, declared, bound,
documented), the stateless host form scann_hip_allow_bitmaps_from_tokens against the dict-of-lists model of
RestrictTokenMap (tests/token_map_model.py), the host form of the block combination against numpy, the refusals, and
scann.hpp's RestrictTokenMap / search_batched_with_tokens compiled in the host C++ harness."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.token_map_model import TokenMapModel, combine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("scann_hip_token_map_create", "scann_hip_token_map_destroy", "scann_hip_token_map_num_tokens",
               "scann_hip_token_map_num_datapoints", "scann_hip_token_map_get_indices",
               "scann_hip_token_map_allow_bitmaps_device", "scann_hip_token_map_allow_bitmaps",
               "scann_hip_allow_bitmaps_from_tokens", "scann_hip_search_batched_tokens", "scann_hip_allow_bitmaps_combine",
               "scann_hip_allow_bitmaps_combine_device")
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)
U64_MAX = 2 ** 64 - 1


def _hip():
    from scann_rust_amd import build, hip
    build.build()
    return hip


def test_token_symbols_are_exported_and_documented():
    hip = _hip()
    lib = ctypes.CDLL(hip.LIB_PATH)
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    header = open(os.path.join(ROOT, "include", "scann_hip.h")).read()
    L = hip.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in hip.EXPORTS
        assert getattr(L, name).argtypes is not None, name + " has no argtypes"
        assert re.search(r"\bfn %s\s*\(" % name, text), "INTEGRATION.md lacks " + name
        assert re.search(r"\b%s\s*\(" % name, header)
    # the handle is opaque (no struct body in the header), the tile size is mirrored
    assert re.search(r"typedef\s+struct\s+scann_hip_token_map\s+scann_hip_token_map\s*;", header)
    assert "pub struct scann_hip_token_map { _p: [u8; 0] }" in text
    m = re.search(r"#define\s+SCANN_HIP_TOKEN_TILE_BITS\s+(\d+)", header)
    assert m and int(m.group(1)) == hip.TOKEN_TILE_BITS
    t = hip.TOKEN_TILE_BITS
    assert t & (t - 1) == 0 and 4 * (t // 8) <= 160 * 1024, "a power of two; several tiles fit a CU's 160 KB of LDS"
    for op, name in ((hip.ALLOW_AND, "AND"), (hip.ALLOW_OR, "OR"), (hip.ALLOW_ANDNOT, "ANDNOT"), (hip.ALLOW_NOT, "NOT")):
        assert re.search(r"#define\s+SCANN_HIP_ALLOW_%s\s+%d\b" % (name, op), header)
    for name in ("TokenMap", "allow_bitmaps_from_tokens", "allow_bitmaps_combine", "allow_bitmaps_combine_device"):
        assert hasattr(hip, name)
    for name in ("num_tokens", "get_indices", "allow_bitmaps", "allow_bitmaps_device", "close", "destroy"):
        assert hasattr(hip.TokenMap, name)


def _pairs(n, rng):
    """(indices, tokens): duplicated pairs, indices at and past the capacity, tokens 0 and 2^64 - 1, a token with only
    out-of-range indices, two tokens that share words, unsorted insertion"""
    p = []
    inside = lambda k: rng.integers(0, n, k).tolist() if n else []
    p += [(i, 0) for i in inside(20)]
    p += [(i, U64_MAX) for i in inside(20)]
    p += [(i, 7) for i in ([n - 1, 0, n - 1, 0] if n else [])]               # duplicated pairs
    p += [(i, 7) for i in (n, n + 63, 0xFFFFFFFF)]                             # at and past the capacity
    p += [(i, 8) for i in (n, n + 1, n + 63, 0xFFFFFFFF, 0xFFFFFFFF)]          # only out-of-range indices
    p += [(i, 20) for i in range(0, min(n, 64), 2)] + [(i, 21) for i in range(1, min(n, 64), 2)]   # share word 0
    p += [(i, 22) for i in inside(40)] + [(i, 22) for i in inside(5)]
    order = rng.permutation(len(p))
    idx = np.array([p[i][0] for i in order], np.uint32)
    tok = np.array([p[i][1] for i in order], np.uint64)
    return idx, tok


def _queries(nq):
    """token lists: empty, unknown, repeated, two tokens sharing words, the extreme token values"""
    kinds = [[], [12345], [7, 7, 7], [20, 21], [0, U64_MAX, 8, 22, 999]]
    if nq == 1:
        return [[0, 12345, 7, 7, 20, 21, U64_MAX, 8]]
    return [kinds[i % len(kinds)] for i in range(nq)]


@pytest.mark.parametrize("nq", [1, 5])
@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_host_from_tokens_matches_the_model(n, extra, nq):
    hip = _hip()
    L = hip.load()
    rng = np.random.default_rng([n, extra, nq])
    idx, tok = _pairs(n, rng)
    model = TokenMapModel(n).add_pairs(idx, tok)
    lists = _queries(nq)
    words = -(-n // 64)
    stride = words + extra
    want = model.allow_bitmaps(lists, stride)
    qt = np.array([t for l in lists for t in l], np.uint64)
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    out = np.full(max(nq * stride, 1) + 1, SENTINEL)   # the function writes every word of the block: gaps come back zero
    status = L.scann_hip_allow_bitmaps_from_tokens(hip.ptr(idx, hip.u32p), hip.ptr(tok, hip.u64p), idx.size, n,
                                                   hip.ptr(qt, hip.u64p) if qt.size else None, hip.ptr(off, hip.u64p), nq,
                                                   stride, hip.ptr(out, hip.u64p))
    assert status == hip.OK
    got = out[:nq * stride].reshape(nq, stride)
    assert np.array_equal(got, want)
    assert np.all(got[:, words:] == 0), "gap words"
    assert np.all(out[nq * stride:] == SENTINEL), "a word past the block was written"
    assert np.array_equal(hip.allow_bitmaps_from_tokens(idx, tok, n, lists, stride), want)
    if n >= 63 and nq == 5:   # the cases are not vacuous: bits are set, two tokens share a word, an unknown token sets none
        assert got[3, 0] == (ONES if n >= 64 else ONES >> np.uint64(1)) and not got[1].any() and not got[0].any()
        assert got[2].any() and got[4].any()


def test_host_from_tokens_refusals_and_empty_map():
    hip = _hip()
    L = hip.load()
    idx, tok = np.array([1, 2, 3], np.uint32), np.array([5, 5, 6], np.uint64)
    qt, off = np.array([5], np.uint64), np.array([0, 1], np.uint64)
    out = np.full(20, SENTINEL)
    call = lambda n, stride, i=idx, t=tok, npairs=3: L.scann_hip_allow_bitmaps_from_tokens(
        hip.ptr(i, hip.u32p) if i is not None else None, hip.ptr(t, hip.u64p) if t is not None else None, npairs, n,
        hip.ptr(qt, hip.u64p), hip.ptr(off, hip.u64p), 1, stride, hip.ptr(out, hip.u64p))
    for n, stride in ((65, 1), (1000, 15), (1, 0), (64, 2 ** 32)):
        assert call(n, stride) == hip.INVALID_ARGUMENT
    assert call(2 ** 32 - 1, 2 ** 26) == hip.OUT_OF_RANGE
    assert call(64, 1, i=None) == hip.INVALID_ARGUMENT and call(64, 1, t=None) == hip.INVALID_ARGUMENT
    assert np.all(out == SENTINEL), "a refused call wrote"
    with pytest.raises(hip.ScannError) as e:
        hip.allow_bitmaps_from_tokens(idx, tok, 65, [[5]], 1)
    assert e.value.code == hip.INVALID_ARGUMENT
    # n_pairs = 0 is a valid empty map: every bitmap zero (null arrays allowed)
    assert call(64, 2, i=None, t=None, npairs=0) == hip.OK
    assert np.all(out[:2] == 0) and np.all(out[2:] == SENTINEL)


def _blocks(nq, words, stride, rng):
    b = rng.integers(0, 2 ** 63, (nq, stride), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (nq, stride), dtype=np.uint64)
    return b


@pytest.mark.parametrize("bits", [1, 63, 64, 65, 1000, 1024])
@pytest.mark.parametrize("op", [1, 2, 3, 4])
def test_host_combine_matches_numpy(op, bits):
    hip = _hip()
    rng = np.random.default_rng([op, bits])
    words = -(-bits // 64)
    nq = 5
    for sa, sb, so in ((words, words, words), (words + 3, words + 1, words + 2), (0, words, words), (words + 1, 0, words + 3)):
        a = _blocks(nq if sa else 1, words, sa or words, rng)
        b = _blocks(nq if sb else 1, words, sb or words, rng)
        out = np.full((nq, so), SENTINEL)
        want = combine(op, a if sa else a[0], b if sb else b[0], bits)
        got = hip.allow_bitmaps_combine(op, a if sa else a[0], None if op == 4 else (b if sb else b[0]), bits, out=out)
        assert got is out
        assert np.array_equal(out[:, :words], np.broadcast_to(want, (nq, words))), "op %d strides %s" % (op, (sa, sb, so))
        assert np.all(out[:, words:] == SENTINEL), "gap words are not touched"
        if bits % 64:
            assert np.all(out[:, words - 1] >> np.uint64(bits % 64) == 0), "a bit at or past the capacity"
    # NOT of an all-zero block: exactly `bits` ones
    z = np.zeros((2, words), np.uint64)
    n = hip.allow_bitmaps_combine(hip.ALLOW_NOT, z, None, bits)
    assert [sum(bin(int(w)).count("1") for w in row) for row in n] == [bits, bits]
    # in place: out is a
    a = _blocks(nq, words, words, rng)
    b = _blocks(nq, words, words, rng)
    want = combine(op, a, b, bits)
    hip.allow_bitmaps_combine(op, a, b, bits, out=a)
    assert np.array_equal(a, want)


def test_host_combine_refusals():
    hip = _hip()
    L = hip.load()
    a = np.zeros((2, 4), np.uint64)
    out = np.full((2, 4), SENTINEL)
    p = lambda x: hip.ptr(x, hip.u64p)
    for op in (0, 5, -1, 100):
        assert L.scann_hip_allow_bitmaps_combine(op, p(a), 4, p(a), 4, 2, 200, p(out), 4) == hip.INVALID_ARGUMENT
    for sa, sb, so in ((3, 4, 4), (4, 3, 4), (4, 4, 3), (4, 4, 0), (1, 0, 4)):
        assert L.scann_hip_allow_bitmaps_combine(hip.ALLOW_AND, p(a), sa, p(a), sb, 2, 200, p(out), so) == hip.INVALID_ARGUMENT
    assert L.scann_hip_allow_bitmaps_combine(hip.ALLOW_AND, p(a), 4, None, 4, 2, 200, p(out), 4) == hip.INVALID_ARGUMENT
    assert np.all(out == SENTINEL), "a refused call wrote"
    # NOT reads no b: a short b stride and a null b are fine
    assert L.scann_hip_allow_bitmaps_combine(hip.ALLOW_NOT, p(a), 4, None, 1, 2, 200, p(out), 4) == hip.OK


def test_token_map_needs_a_gpu():
    """no quiet host fall-back: without a device the handle cannot be created"""
    import torch
    if torch.cuda.device_count() > 0:
        pytest.skip("GPU present")
    hip = _hip()
    with pytest.raises(hip.ScannError) as e:
        hip.TokenMap(10, [1, 2], [3, 4])
    assert e.value.code in (hip.UNAVAILABLE, hip.INTERNAL)


CPP = r"""
#include "scann.hpp"
#include <cstdio>
using namespace scann;
int main(int argc, char **argv) {
    // the batched entry exists on the tree and the hasher types, with this signature
    std::vector<NNResultsVector> (TreeXHybridSearcher::*pt)(const std::vector<std::vector<float>> &, size_t,
        const std::vector<std::vector<uint64_t>> &, const DeviceTokenMap &) const = &TreeXHybridSearcher::search_batched_with_tokens;
    std::vector<NNResultsVector> (AsymmetricHasher::*pa)(const std::vector<std::vector<float>> &, size_t,
        const std::vector<std::vector<uint64_t>> &, const DeviceTokenMap &) const = &AsymmetricHasher::search_batched_with_tokens;
    if (!pt || !pa) return 3;
    RestrictTokenMap m(100);
    m.add_token(5, 7);
    m.add_token(3, 7);
    m.add_token(5, 7);          // duplicates stay, insertion order stays
    m.add_token(100, 7);        // out of range stays in the list, never in an allowlist
    m.set_tokens(64, {9, 7, 0xFFFFFFFFFFFFFFFFull});
    if (m.num_tokens() != 3 || m.num_datapoints() != 100) return 4;
    const auto *ix = m.get_indices(7);
    if (!ix || *ix != std::vector<DatapointIndex>({5, 3, 5, 100, 64})) return 5;
    if (m.get_indices(8)) return 6;
    RestrictAllowlist a = m.create_allowlist({7, 8, 7});
    if (a.num_allowed() != 3 || !a.is_allowed(3) || !a.is_allowed(5) || !a.is_allowed(64) || a.is_allowed(100)) return 7;
    const auto w = m.create_allowlist({9, 0xFFFFFFFFFFFFFFFFull}).to_bitmap(100);
    if (w.size() != 2 || w[0] != 0 || w[1] != 1) return 8;
    if (m.create_allowlist({}).num_allowed() != 0) return 9;
    std::printf("token map ok\n");
    if (argc > 1) {   // without a device the upload fails loudly; a default handle makes the search throw
        TreeXHybridSearcher *none = nullptr;
        (void)none;
        try {
            DeviceTokenMap d = m.to_device(context(0));
            std::printf("on device %zu\n", d.num_tokens());
        } catch (const ScannError &e) {
            std::printf("to_device failed: %d\n", (int)e.code);
        }
        try {
            detail::run_search_tokens(nullptr, {{1.0f}}, 1, {{7}}, DeviceTokenMap(), scann_hip_search_opts());
            return 10;
        } catch (const ScannError &e) {
            std::printf("search failed: %d\n", (int)e.code);
        }
    }
    return 0;
}
"""


def test_scann_hpp_token_map_compiles_and_matches_the_model(tmp_path):
    """RestrictTokenMap in the host C++ harness (the flags of build.build_host): the reference's methods and its exact
    get_indices order, the same answers as the Python model; search_batched_with_tokens exists on both searcher types and
    fails loudly without a device map"""
    import torch
    from scann_rust_amd import build
    build.build()
    model = TokenMapModel(100)
    for i, t in ((5, 7), (3, 7), (5, 7), (100, 7)):
        model.add_token(i, t)
    model.set_tokens(64, [9, 7, U64_MAX])
    assert model.get_indices(7) == [5, 3, 5, 100, 64] and model.get_indices(8) is None and model.num_tokens() == 3
    assert model.stored_posting(7).tolist() == [3, 5, 64]
    assert model.create_allowlist([9, U64_MAX]).tolist() == [0, 1]
    src = tmp_path / "token_map_test.cpp"
    src.write_text(CPP)
    exe = str(tmp_path / "token_map_test")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I" + build.HOST, "-o", exe, str(src), "-L" + build.HERE, "-lscann_hip",
           "-Wl,-rpath," + build.HERE, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "device"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "token map ok" in r.stdout, r.stdout + r.stderr
    assert "search failed: %d" % 9 in r.stdout, r.stdout   # FailedPrecondition: no device map
    if torch.cuda.device_count() == 0:
        assert re.search(r"to_device failed: (13|14)\b", r.stdout), r.stdout   # Internal / Unavailable: never a quiet host map
    else:
        assert "on device 3" in r.stdout, r.stdout

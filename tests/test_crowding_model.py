"""CPU checks of crowding: the numpy/dict model of CrowdingConstraint::apply against the reference's own unit-test
vectors (restricts/crowding.rs:274-311) and the prefix property the exact crowded search rests on; the C++ mirror's
CrowdingConstraint (host-only program); the new entry points declared, exported, bound and documented; the table's
slot count."""
import os
import re
import subprocess

import numpy as np

import crowding_model as CM
from scann_rust_amd import build, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scann_hip.h")
NEW_SYMBOLS = ("scann_hip_crowd_table_slots", "scann_hip_index_set_crowding_attributes", "scann_hip_search_crowded",
               "scann_hip_index_reserve_crowded", "scann_hip_search_crowded_device")


def _read(path):
    with open(path, encoding="utf-8") as fh:
        return fh.read()


def test_reference_vector():
    """crowding.rs:275-299: attributes [0,0,0,1,1,2], limit 2 -> [0,1,3,4,5]"""
    idx = np.arange(6, dtype=np.uint32)
    dist = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6], np.float32)
    gi, gd = CM.apply(idx, dist, [0, 0, 0, 1, 1, 2], 2, 6)
    assert gi.tolist() == [0, 1, 3, 4, 5] and len(gi) == 5
    assert np.array_equal(gd, dist[[0, 1, 3, 4, 5]])


def test_disabled_limit_zero_and_missing_attributes():
    idx = np.arange(3, dtype=np.uint32)
    dist = np.array([0.1, 0.2, 0.3], np.float32)
    gi, _ = CM.apply(idx, dist, [0, 0, 0], 1, 3, enabled=False)      # crowding.rs:301-311
    assert gi.tolist() == [0, 1, 2]
    assert CM.apply(idx, dist, [0, 1, 2], 0, 3)[0].size == 0           # limit 0 keeps nothing
    # index past the array -> attribute 0, crowding with the real zeros
    gi, _ = CM.apply(np.array([5, 1, 0, 9], np.uint32), np.arange(4, dtype=np.float32), [7, 0], 1, 4)
    assert gi.tolist() == [5, 0]
    assert CM.attribute([7, 0], 1) == 0 and CM.attribute([7, 0], 2) == 0 and CM.attribute([], 0) == 0
    # stops at k kept; limit >= depth returns the first k
    assert CM.apply(np.arange(10), np.arange(10.0), np.arange(10) % 2, 10, 4)[0].tolist() == [0, 1, 2, 3]
    assert CM.apply(np.arange(10), np.arange(10.0), np.arange(10) % 2, 1, 4)[0].tolist() == [0, 1]


def test_prefix_property():
    """apply(row[:d], k) of length k equals apply(row, k) for every d"""
    rng = np.random.default_rng(11)
    full = 0
    for trial in range(60):
        n = int(rng.integers(1, 80))
        row = rng.permutation(200)[:n].astype(np.uint32)
        dist = np.sort(rng.random(n).astype(np.float32))
        attrs = rng.integers(0, int(rng.integers(1, 12)), 150).astype(np.uint64)   # shorter than the index range
        for limit in (1, 2, 5):
            for k in (1, 3, 10):
                want_i, want_d = CM.apply(row, dist, attrs, limit, k)
                for d in range(n + 1):
                    gi, gd = CM.apply(row[:d], dist[:d], attrs, limit, k)
                    if gi.size == k:
                        full += 1
                        assert np.array_equal(gi, want_i) and np.array_equal(gd, want_d), (trial, limit, k, d)
                    else:   # a short answer is a prefix of the full one
                        assert np.array_equal(gi, want_i[:gi.size])
    assert full > 1000


def test_vectorised_model_equals_the_walk():
    """apply_fast (what the GPU tests call per row) == apply on random rows, every limit and k edge"""
    rng = np.random.default_rng(12)
    for trial in range(200):
        n = int(rng.integers(0, 150))
        row = rng.permutation(400)[:n].astype(np.uint32)
        dist = np.sort(rng.random(n).astype(np.float32))
        kind = trial % 4
        attrs = (rng.integers(0, int(rng.integers(1, 20)), 300).astype(np.uint64) if kind < 2 else
                 (rng.integers(0, 3, 300).astype(np.uint64) << np.uint64(40)) if kind == 2 else
                 np.where(rng.random(300) < 0.5, np.uint64(0), np.uint64(0xFFFFFFFFFFFFFFFF)))
        for limit in (0, 1, 2, 7, n, 2 ** 32 - 1):
            for k in (0, 1, 5, n, n + 3):
                wi, wd = CM.apply(row, dist, attrs, limit, k)
                gi, gd = CM.apply_fast(row, dist, attrs, limit, k)
                assert np.array_equal(gi, wi) and np.array_equal(gd, wd), (trial, limit, k)


def test_host_cpp_crowding_constraint():
    """CrowdingConstraint of scann.hpp: apply on the reference's vectors, set_attribute's resize with 0"""
    build.build_host()
    exe = os.path.join(os.path.dirname(os.path.abspath(build.__file__)), "host", "crowding_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "crowding_test ok" in r.stdout


def test_new_symbols_declared_exported_bound_and_documented():
    decl = re.sub(r"/\*.*?\*/", "", _read(HEADER), flags=re.S)
    lib = hip.load()
    doc = _read(os.path.join(ROOT, "INTEGRATION.md"))
    block = doc[doc.index('extern "C" {'):doc.index("<!-- END generated -->")]
    dynsym = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, decl), "%s is not declared in scann_hip.h" % name
        assert name in hip.EXPORTS and getattr(lib, name) is not None
        assert re.search(r"\bT %s$" % name, dynsym, flags=re.M), "%s is not exported by the library" % name
        assert "pub fn %s(" % name in block, "INTEGRATION.md's extern block lacks %s" % name
    m = re.search(r"scann_hip_search_crowded\s*\(([^;]*?)\)\s*;", decl, flags=re.S)
    assert " ".join(m.group(1).split()) == (
        "scann_hip_index *index, const float *queries, uint32_t nq, uint32_t q_stride, uint32_t q_dim, uint32_t k, "
        "uint32_t depth, uint32_t per_crowd_limit, const scann_hip_search_opts *opts, uint32_t *out_idx, "
        "float *out_dist, uint32_t *out_count")
    text = " ".join(re.sub(r"^\s*\*", " ", _read(HEADER), flags=re.M).split())
    for phrase in ("CrowdingConstraint::apply(search(query, depth), k)", "depth < k -> InvalidArgument",
                   "no attributes attached -> FailedPrecondition", "depth = 0 means depth = k",
                   "per_crowd_limit = 0 keeps nothing", "has attribute 0"):
        assert phrase in text, phrase
    design = _read(os.path.join(ROOT, "DESIGN.md"))
    assert "3.3d" in design and "CrowdingMultidimensional" in design


def test_table_slots():
    """clamp(next_pow2(2 depth), 128, SCANN_HIP_CROWD_MAX_SLOTS): always more slots than a row has entries"""
    hdr = _read(HEADER)
    max_slots = int(re.search(r"#define SCANN_HIP_CROWD_MAX_SLOTS (\d+)", hdr).group(1))
    max_depth = int(re.search(r"#define SCANN_HIP_CROWD_MAX_DEPTH (\d+)", hdr).group(1))
    assert max_slots * 12 <= 160 * 1024 and max_depth == 8192
    for depth in (0, 1, 63, 64, 65, 100, 1000, 2048, 4096, 6144, 6145, 8191, 8192):
        want = 128
        while want < 2 * max(depth, 1):
            want *= 2
        want = min(want, max_slots)
        assert hip.crowd_table_slots(depth) == want, depth
        assert hip.crowd_table_slots(depth) > depth

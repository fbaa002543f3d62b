"""CPU-only checks of the filtered brute-force interface: the radius entry point with options is declared, exported,
bound and documented; the header states the brute-force filter contract; and the host-side count that filtered
searches are planned with (the mirror of the device compaction's total) equals numpy's on every capacity edge."""
import os
import re
import subprocess

import numpy as np

from scann_rust_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scann_hip.h")
NEW_SYMBOLS = ("scann_hip_bf_search_radius_opts", "scann_hip_allow_bitmap_count")


def _read(path):
    with open(path, encoding="utf-8") as fh:
        return fh.read()


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
    m = re.search(r"scann_hip_bf_search_radius_opts\s*\(([^;]*?)\)\s*;", decl, flags=re.S)
    args = " ".join(m.group(1).split())
    assert args == ("scann_hip_index *index, const float *query, uint32_t q_dim, float radius, "
                    "const scann_hip_search_opts *opts, uint32_t *out_idx, float *out_dist, uint64_t capacity, "
                    "uint64_t *out_count")


def test_header_states_the_brute_force_filter_contract():
    text = " ".join(re.sub(r"^\s*\*", " ", _read(HEADER), flags=re.M).split())
    assert "is not applied" not in text
    for phrase in ("A filtered search answers exactly as an unfiltered search over a handle built from the allowed rows alone",
                   "k = min(k, number of allowed rows)", "never appears and never displaces one",
                   "Filtered calls never take the bf16-shortlist path"):
        assert phrase in text, phrase
    design = _read(os.path.join(ROOT, "DESIGN.md"))
    assert "SCANN_HIP_BF_FILTER_COMPACT_MAX" in design and "SCANN_HIP_BF_FILTER" in _read(os.path.join(ROOT, "README.md"))


def _numpy_count(words, bits, n):
    eff = min(bits, n, words.size * 64)
    i = np.arange(eff, dtype=np.uint64)
    return int(np.count_nonzero((words[(i >> np.uint64(6)).astype(np.int64)] >> (i & np.uint64(63))) & np.uint64(1)))


def test_host_count_mirror_against_numpy():
    """popcount, clipping to the capacity and to the row count, tail-bit masking"""
    rng = np.random.default_rng(3)
    full = np.uint64(0xFFFFFFFFFFFFFFFF)
    for n in (1, 63, 64, 65, 1000, 8192, 20013):
        nw = -(-n // 64)
        for words in (np.full(nw + 2, full), rng.integers(0, 1 << 63, nw + 2, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
                      np.zeros(nw + 2, np.uint64)):
            for bits in (0, 1, 63, 64, 65, n - 1, n, n + 1, n + 100, (nw + 2) * 64):
                if bits < 0:
                    continue
                got = hip.allow_bitmap_count(words, bits, n)
                assert got == _numpy_count(words, bits, n), (n, bits)
    ones = np.full(4, full)
    assert hip.allow_bitmap_count(ones, 0, 200) == 0            # capacity 0 allows nothing
    assert hip.allow_bitmap_count(ones, 70, 200) == 70          # garbage past the capacity in the last word is ignored
    assert hip.allow_bitmap_count(ones, 256, 100) == 100        # datapoints >= n do not exist

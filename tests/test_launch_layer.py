"""CPU-only source checks: kernels are launched, their launch errors checked, their LDS attribute set and the CU count
read in csrc/launch.h alone; the hand-counted static LDS sizes stay gone."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scann_rust_amd", "csrc")
LAUNCH_H = os.path.join(CSRC, "launch.h")
ONLY_IN_LAUNCH_H = ["hipLaunchKernelGGL", "hipGetLastError", "hipFuncSetAttribute",
                    "hipDeviceAttributeMultiprocessorCount"]


def _sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".hip")))


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as fh:
        return fh.read()


def test_launch_h_is_the_only_place_that_launches():
    text = _read(LAUNCH_H)
    assert [n for n in ONLY_IN_LAUNCH_H if n not in text] == []
    offenders = ["%s: %s" % (os.path.basename(p), n) for p in _sources() if p != LAUNCH_H
                 for n in ONLY_IN_LAUNCH_H if re.search(r"\b%s\b" % n, _read(p))]
    assert offenders == []
    # no second spelling of a launch either
    assert [os.path.basename(p) for p in _sources() if p != LAUNCH_H and
            re.search(r"<<<|\bhipLaunchKernel\b|\bhipModuleLaunchKernel\b", _read(p))] == []


def test_static_lds_sizes_are_not_typed_by_hand():
    assert [os.path.basename(p) for p in _sources() if "set_dyn_lds_with_static" in _read(p)] == []
    assert "hipFuncGetAttributes" in _read(LAUNCH_H)


def test_the_kernel_files_launch_through_launch_h():
    for f in ("txh.hip", "txh_partition.hip", "txh_prefilter.hip", "txh_rows.hip", "txh_blocks.hip",
              "bf.hip", "comm.hip", "crowd.hip"):
        text = _read(os.path.join(CSRC, f))
        assert '#include "launch.h"' in text, f
        assert re.search(r"\blaunch\(", text), f


def test_every_source_and_header_is_in_the_build():
    """A source the build does not list is not compiled; a header it does not list neither triggers a rebuild nor
    enters src_sha256.  txh.h is the tree search's interface: the units' internal headers stay behind it."""
    from scann_rust_amd import build
    files = os.listdir(CSRC)
    assert sorted(f for f in files if f.endswith(".hip")) == sorted(build.SOURCES)
    assert [f for f in files if f.endswith(".h") and f not in build.HEADERS] == []
    assert re.findall(r'#include\s+"(txh_dev|txh_stages)\.h"', _read(os.path.join(CSRC, "txh.h"))) == []
    for f in files:   # and only the tree-search units include them
        if not f.startswith("txh"):
            assert re.findall(r'#include\s+"(txh_dev|txh_stages)\.h"', _read(os.path.join(CSRC, f))) == [], f


def test_launch_h_is_a_build_dependency():
    from scann_rust_amd import build
    assert "launch.h" in build.HEADERS

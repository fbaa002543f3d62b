"""build_hierarchical_on_device of the C++ mirror (scann_rust_amd/host/scann.hpp) through
scann_hip_txh_build_hierarchical, and its program hier_build_test: compiles on a CPU and fails loudly there; on a GPU it
builds a depth-2 tree twice and once through the C ABI and compares the searches bit for bit."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "scann_rust_amd", "host", "hier_build_test")


def _compile():
    from scann_rust_amd import build
    assert "hier_build_test" in build.HOST_PROGRAMS and "ktree.hip" in build.SOURCES and "ktree.h" in build.HEADERS
    build.build_host()
    assert os.path.exists(EXE)
    return EXE


def test_hier_build_test_compiles_and_fails_loudly_without_gpu():
    exe = _compile()
    import torch
    if torch.cuda.device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 2 and "no HIP device" in r.stdout   # Unavailable, no CPU fallback
        assert "hier_build_test ok" not in r.stdout


@pytest.mark.gpu
def test_hier_build_test_on_the_device():
    r = subprocess.run([_compile()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hier_build_test ok" in r.stdout

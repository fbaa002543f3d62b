"""scann::MutableIndex of the C++ mirror (scann_rust_amd/host/scann.hpp) and its program mutable_test: compiles on a CPU
and fails loudly there; on a GPU it replays the mutation script, export / compact and the host-side refusals."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "scann_rust_amd", "host", "mutable_test")


def _compile():
    from scann_rust_amd import build
    assert "mutable_test" in build.HOST_PROGRAMS and "mutable.hip" in build.SOURCES
    build.build_host()
    assert os.path.exists(EXE)
    return EXE


def test_mutable_test_compiles_and_fails_loudly_without_gpu():
    exe = _compile()
    import torch
    if torch.cuda.device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 2 and "no HIP device" in r.stdout   # Unavailable, no CPU fallback
        assert "mutable_test ok" not in r.stdout


def test_mutable_symbols_bound_and_documented():
    """every scann_hip_mutable_* declaration is exported, bound by hip.py and listed in INTEGRATION.md's extern block"""
    import re
    from scann_rust_amd import hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scann_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(scann_hip_mutable_[a-z0-9_]+)\s*\(", text)))
    assert len(declared) == 15, declared
    L = hip.load()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in declared:
        assert hasattr(L, name) and name in hip.EXPORTS
        assert re.search(r"\bfn %s\s*\(" % name, doc), name
    assert "pub struct scann_hip_mutable {" in doc
    assert (hip.MUTABLE_MAX_CAPACITY, hip.MUTABLE_MAX_K, hip.MUTABLE_DELTA_TILE) == tuple(
        int(re.search(r"#define SCANN_HIP_MUTABLE_%s (\d+)" % n, text).group(1))
        for n in ("MAX_CAPACITY", "MAX_K", "DELTA_TILE"))


@pytest.mark.gpu
def test_mutable_test_on_the_device():
    r = subprocess.run([_compile()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mutable_test ok" in r.stdout

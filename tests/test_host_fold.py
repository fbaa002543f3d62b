"""scann::MutableIndex::compact of the C++ mirror (scann_rust_amd/host/scann.hpp) through scann_hip_fold_mutable, and its
program fold_test: compiles on a CPU and fails loudly there; on a GPU it compacts a mutated index twice and compares every
search with a searcher built from the live rows."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "scann_rust_amd", "host", "fold_test")


def _compile():
    from scann_rust_amd import build
    assert "fold_test" in build.HOST_PROGRAMS and "fold.hip" in build.SOURCES
    build.build_host()
    assert os.path.exists(EXE)
    return EXE


def test_fold_test_compiles_and_fails_loudly_without_gpu():
    exe = _compile()
    import torch
    if torch.cuda.device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 2 and "no HIP device" in r.stdout   # Unavailable, no CPU fallback
        assert "fold_test ok" not in r.stdout


def test_fold_symbols_bound_and_documented():
    """the fold and the handle writer are declared, exported, bound by hip.py and listed in INTEGRATION.md; the chunk
    length is published and mirrored"""
    from scann_rust_amd import hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scann_hip.h")).read(), flags=re.S)
    L = hip.load()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("scann_hip_fold_mutable", "scann_hip_fold_mutable_stage_ms", "scann_hip_index_write_file"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(L, name) and name in hip.EXPORTS
        assert re.search(r"\bfn %s\s*\(" % name, doc), name
    assert hip.FOLD_CHUNK == int(re.search(r"#define SCANN_HIP_FOLD_CHUNK (\d+)", text).group(1))
    assert callable(hip.Mutable.fold) and callable(hip.index_write_file)
    assert len(hip.abi_layout()) == 6                          # no new struct: the layout words are those of before


@pytest.mark.gpu
def test_fold_test_on_the_device():
    r = subprocess.run([_compile()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fold_test ok" in r.stdout

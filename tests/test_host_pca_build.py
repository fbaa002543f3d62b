"""Projection::train_pca_on_device and build_projected_on_device of the C++ mirror (scann_rust_amd/host/scann.hpp) through
scann_hip_pca_train and scann_hip_txh_build_projected, and their program pca_build_test: compiles on a CPU and fails
loudly there; on a GPU it trains, builds a projected tree and a projected hasher, searches them, and compares with a
second build and with the chained route."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "scann_rust_amd", "host", "pca_build_test")


def _compile():
    from scann_rust_amd import build
    assert "pca_build_test" in build.HOST_PROGRAMS and "pca.hip" in build.SOURCES and "pca.h" in build.HEADERS
    build.build_host()
    assert os.path.exists(EXE)
    return EXE


def test_pca_build_test_compiles_and_fails_loudly_without_gpu():
    exe = _compile()
    import torch
    if torch.cuda.device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 2 and "no HIP device" in r.stdout   # Unavailable, no CPU fallback
        assert "pca_build_test ok" not in r.stdout


def test_pca_symbols_bound_and_documented():
    from scann_rust_amd import hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scann_hip.h")).read(), flags=re.S)
    L = hip.load()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("scann_hip_pca_train", "scann_hip_projection_arrays", "scann_hip_txh_build_projected",
                 "scann_hip_pca_last_stage_ms"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(L, name) and name in hip.EXPORTS
        assert re.search(r"\bfn %s\s*\(" % name, doc), name
    assert callable(hip.pca_train) and callable(hip.txh_build_projected) and callable(hip.Projection.arrays)
    # the mirror offers both, next to build_on_device
    hpp = open(os.path.join(ROOT, "scann_rust_amd", "host", "scann.hpp")).read()
    assert "train_pca_on_device" in hpp and hpp.count("void build_projected_on_device(") == 2
    # the covariance is the f64 MFMA's, and the unit is compiled without contraction like the rest
    src = open(os.path.join(ROOT, "scann_rust_amd", "csrc", "pca.hip")).read()
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in src
    from scann_rust_amd import build
    assert "-ffp-contract=off" in build.CFLAGS


@pytest.mark.gpu
def test_pca_build_test_on_the_device():
    r = subprocess.run([_compile()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pca_build_test ok" in r.stdout

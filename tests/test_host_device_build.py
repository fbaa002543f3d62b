"""build_on_device of the C++ mirror (scann_rust_amd/host/scann.hpp) through scann_hip_txh_build, and its program
device_build_test: compiles on a CPU and fails loudly there; on a GPU it builds a flat hasher and a tree on the device
and compares their searches with the host-built hasher, with a second build and with the per-subspace route."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "scann_rust_amd", "host", "device_build_test")


def _compile():
    from scann_rust_amd import build
    assert "device_build_test" in build.HOST_PROGRAMS and "build.hip" in build.SOURCES and "build.h" in build.HEADERS
    build.build_host()
    assert os.path.exists(EXE)
    return EXE


def test_device_build_test_compiles_and_fails_loudly_without_gpu():
    exe = _compile()
    import torch
    if torch.cuda.device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 2 and "no HIP device" in r.stdout   # Unavailable, no CPU fallback
        assert "device_build_test ok" not in r.stdout


def test_build_symbols_bound_and_documented():
    from scann_rust_amd import hip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scann_hip.h")).read(), flags=re.S)
    L = hip.load()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("scann_hip_txh_build", "scann_hip_build_config_default"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(L, name) and name in hip.EXPORTS
        assert re.search(r"\bfn %s\s*\(" % name, doc), name
    for struct in ("scann_hip_build_config", "scann_hip_build_report"):
        assert re.search(r"typedef\s+struct\s+%s\s*\{" % struct, text), struct
        assert "pub struct %s {" % struct in doc
    assert callable(hip.txh_build) and len(hip.abi_layout(10)) == 10
    # the build unit is compiled without contraction, like every unit that follows the reference's f32 arithmetic
    from scann_rust_amd import build
    assert "-ffp-contract=off" in build.CFLAGS


@pytest.mark.gpu
def test_device_build_test_on_the_device():
    r = subprocess.run([_compile()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "device_build_test ok" in r.stdout

"""CPU-only checks of the stacked-quantizer handle: the symbols are declared, exported, bound and in the Rust block;
csrc/stacked.h's planning rules hold at their edges (compiled into a stand-alone host program); trainer.train_stacked
lowers the reconstruction error level by level on the reference's own test data (hashes/stacked.rs:331-340)."""
import os
import re
import subprocess

import numpy as np
import pytest

from scann_rust_amd import build, hip, trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["scann_hip_stacked_" + n for n in ("create", "destroy", "encode", "decode", "set_rows", "set_codes", "distances",
                                            "search_batched", "size", "info", "last_kernel_ms")]
PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "stacked.h"
using namespace scann;
int main(int argc, char **argv) {   // dim quads k n S_0 K_0 S_1 K_1 ...
    const uint32_t dim = atoi(argv[1]), quads = atoi(argv[2]), k = atoi(argv[3]);
    const uint64_t n = strtoull(argv[4], 0, 10);
    uint32_t S[16], K[16], L = 0;
    for (int i = 5; i + 1 < argc; i += 2, ++L) S[L] = atoi(argv[i]), K[L] = atoi(argv[i + 1]);
    StackedShape sh;
    const char *why = "";
    const int status = stacked_shape(dim, L, S, K, &sh, &why);
    printf("status %d\n", status);
    if (status) return 0;
    std::vector<uint32_t> eoff, slab;
    stacked_entry_offsets(sh, &eoff);
    stacked_plan_slabs(sh, eoff, quads, &slab);
    uint32_t worst = 0;
    for (size_t i = 0; i + 1 < slab.size(); ++i)
        if (eoff[4 * slab[i + 1]] - eoff[4 * slab[i]] > worst) worst = eoff[4 * slab[i + 1]] - eoff[4 * slab[i]];
    uint32_t rows = 0, chunks = 0, group = 0, run = 0;
    stacked_chunks(n, kStackedMergeKeys / k, &rows, &chunks);
    stacked_enc_slab(K[0], dim / S[0], &group, &run);
    const uint32_t tile = stacked_tile_rows(dim, sh.T);
    printf("T %u\nentries %u\ntile %u\nenc_lds %zu\ngroup %u\nrun %u\nslabs %zu\nlast_dword %u\nslab_bytes %u\n", sh.T, sh.entries, tile,
           stacked_enc_lds(dim, sh.T, tile), group, run, slab.size() - 1, slab.back(), worst * 16 * quads);
    printf("scan_lds %zu\nchunk_rows %u\nchunks %u\n", stacked_scan_lds(quads, k, true, (uint32_t)slab.size() - 1), rows, chunks);
    return 0;
}
"""


def test_symbols_are_declared_exported_bound_and_in_the_rust_block():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scann_hip.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    source = open(os.path.join(ROOT, "scann_rust_amd", "hip.py")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in hip.EXPORTS, name
        assert "L.%s.argtypes" % name in source, name
        assert "pub fn %s(" % name in rust, name
    assert "pub struct scann_hip_stacked {" in rust and "hashes/stacked.rs" in rust


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("stacked")
    src, exe = d / "plan.cpp", d / "plan"
    src.write_text(PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + build.CSRC, "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(dim, quads, k, n, *levels):
        out = subprocess.run([str(exe)] + [str(x) for x in (dim, quads, k, n) + levels], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        return {a: int(b) for a, b in (line.split() for line in out.stdout.splitlines())}
    return run


@pytest.mark.parametrize("dim,tile", [(1, 256), (63, 256), (64, 252), (128, 127), (4095, 4)])
def test_tile_rows_fill_64_kb_and_dim_4095_is_the_last(plan, dim, tile):
    p = plan(dim, 1, 10, 1000, 1, 256)
    assert p["status"] == 0 and p["tile"] == tile and p["enc_lds"] <= 160 * 1024 - 8192
    assert tile == 256 or (tile + 1) * (dim | 1) * 4 > 65536
    assert p["run"] >= 2 and (p["group"] == 1) == (256 * dim * 2 > 8192)
    assert plan(4096, 1, 10, 1000, 1, 256)["status"] == hip.UNIMPLEMENTED


def test_tile_rows_leave_room_for_the_codes(plan):
    assert plan(32, 1, 10, 1000, *(32, 2) * 8)["tile"] == 16384 // 256   # T = 256


@pytest.mark.parametrize("quads", [1, 2])
@pytest.mark.parametrize("levels,slabs", [((4, 16), 1), ((16, 256, 16, 256), None), ((16, 256) * 4, None), ((4, 16, 3, 16), 1)])
def test_table_slabs_fit_their_buffer_and_cover_every_dword(plan, levels, slabs, quads):
    p = plan(48, quads, 256, 1000, *levels)
    assert p["slab_bytes"] <= 32 * 1024 and p["last_dword"] == (p["T"] + 3) // 4
    assert p["slabs"] == (slabs or -(-p["entries"] * 16 * quads // (32 * 1024)))   # (full dwords of 256-code tables pack exactly)
    assert p["scan_lds"] <= 160 * 1024 - 1024
    assert p["entries"] == sum(s * k for s, k in zip(levels[::2], levels[1::2])) + (-p["T"]) % 4


@pytest.mark.parametrize("n", [0, 1, 8192, 8193, 10 ** 6, 2 ** 32 - 2])
@pytest.mark.parametrize("k", [1, 10, 256])
def test_chunks_times_k_stay_within_the_merge(plan, n, k):
    p = plan(16, 1, k, n, 4, 16)
    assert p["chunks"] * k <= 8192 and p["chunks"] * p["chunk_rows"] >= n > (p["chunks"] - 1) * p["chunk_rows"] - (n == 0)
    assert p["chunk_rows"] % 2048 == 0 and p["chunk_rows"] >= 8192


def test_train_stacked_lowers_the_error_level_by_level():
    i, j = np.arange(100)[:, None], np.arange(16)[None, :]
    X = np.sin((i * j).astype(np.float32) / np.float32(100.0)).astype(np.float32)
    errors = [float((X ** 2).sum())]
    for levels in (1, 2, 3):
        books, R = trainer.train_stacked(X, (4,) * levels, (16,) * levels)
        assert [b.shape for b in books] == [(4, 16, 4)] * levels
        errors.append(float((R ** 2).sum()))
    assert errors[0] > errors[1] > errors[2] > errors[3]
    assert trainer.train_stacked(X, (1, 1), (16, 16))[0][1].shape == (1, 16, 16)   # the additive form

"""csrc/txh_arena.h on the host: a stand-alone program (its own main, the host compiler, no HIP) includes the header and
prints the arena's buffer names in placement order and, for a few vectors of sizes, where txh_arena_place puts every
buffer.

The names are compared with the list below, spelled out: the order is the arena's layout, and a buffer that moved would
change where every later one lies.  The placement is compared with a Python mirror of the arithmetic: buffer i is preceded
by a skew of (((i + 1) * 37) % 509) * 256 bytes, its capacity is its size rounded up to 256, and a buffer of size 0 gets
no place while its skew still counts.  The program is built once more with the address and undefined-behaviour
sanitizers and run directly."""
import subprocess

import pytest

from scann_rust_amd import build

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "txh_arena.h"
int main(int argc, char **argv) {
    // no arguments: the names; else one size per buffer
    if (argc == 1) {
        printf("count %zu\n", scann::kTxhArenaCount);
        for (size_t i = 0; i < scann::kTxhArenaCount; ++i) printf("name %s\n", scann::kTxhArenaNames[i]);
        scann::TxhArenaBufs bufs;
        size_t members = 0;
        bufs.for_each([&](scann::WsBuf &b) { members += b.p == nullptr && b.bytes == 0 && b.need == 0; });
        printf("members %zu\n", members);
        return 0;
    }
    if ((size_t)argc - 1 != scann::kTxhArenaCount) return 2;
    std::vector<size_t> need(scann::kTxhArenaCount), off(scann::kTxhArenaCount), cap(scann::kTxhArenaCount);
    for (size_t i = 0; i < need.size(); ++i) need[i] = strtoull(argv[i + 1], nullptr, 10);
    const size_t total = scann::txh_arena_place(need.data(), need.size(), off.data(), cap.data());
    for (size_t i = 0; i < need.size(); ++i) {
        if (off[i] == scann::kArenaNoPlace) printf("buf %s - %zu\n", scann::kTxhArenaNames[i], cap[i]);
        else printf("buf %s %zu %zu\n", scann::kTxhArenaNames[i], off[i], cap[i]);
    }
    printf("total %zu\n", total);
    return 0;
}
"""

NAMES = ["queries", "cdist", "tokens", "token_dists", "vbase", "leaf_cnt", "leaf_cursor", "pair_off", "tile_off",
         "counters", "pair_q", "pair_leaf", "pair_vbase", "pair_thr", "slot_of", "lutq", "thr", "cand_cnt", "cand",
         "cand_key", "cand_idx", "cand_dist", "cand_exact", "cand_row", "cand_count", "out_idx", "out_dist", "out_count",
         "allow", "sbase", "pair_sbase", "stile_off", "samp", "lut8", "lut8_meta", "cand32", "cand32_codes", "cand32_cnt",
         "mfma_thr1", "rr_lb", "rr_ub", "small_tickets", "wide_min", "wide_ckey", "wide_ceb", "wide_cidx", "wide_cnt",
         "proj_q", "surv"]

# the [nq][m] per-candidate arrays that rerank_short_kernel and the kernels around it walk in step
PER_CANDIDATE = ["cand_idx", "cand_dist", "cand_exact", "cand_row", "rr_lb", "rr_ub"]


def mirror(need):
    """([(offset or None, capacity)], total) of the arena for the sizes `need`, in placement order"""
    off, out = 0, []
    for i, n in enumerate(need):
        off += (((i + 1) * 37) % 509) * 256
        cap = (n + 255) // 256 * 256
        out.append((off if n else None, cap))
        off += cap
    return out, off


def _build(d, flags, name):
    src, exe = d / "arena_main.cpp", d / name
    src.write_text(PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + build.CSRC] + flags + ["-o", str(exe), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("arena_" + request.param)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    return _build(d, flags, "arena_main")


def _place(exe, need):
    r = subprocess.run([exe] + [str(n) for n in need], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr
    rows, total = [], None
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "buf":
            rows.append((f[1], None if f[2] == "-" else int(f[2]), int(f[3])))
        elif f[0] == "total":
            total = int(f[1])
    return rows, total


def test_the_49_buffers_in_placement_order(program):
    assert len(NAMES) == 49 == len(set(NAMES)) and NAMES[-2:] == ["proj_q", "surv"]
    r = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "count 49" and lines[-1] == "members 49", "one member per name, each visited once by for_each"
    assert [l.split()[1] for l in lines[1:-1]] == NAMES


NEEDS = {
    "all zero": [0] * 49,
    "all one": [1] * 49,
    "only the last": [0] * 48 + [1000],
    "per-candidate arrays of 1024 x 8192": [1024 * 8192 * 4 if n in PER_CANDIDATE else 16 for n in NAMES],
}


@pytest.mark.parametrize("case", list(NEEDS))
def test_placement_equals_the_mirror(program, case):
    need = NEEDS[case]
    rows, total = _place(program, need)
    want, want_total = mirror(need)
    assert [r[0] for r in rows] == NAMES
    assert [(r[1], r[2]) for r in rows] == want, case
    assert total == want_total, case
    placed = sorted((off, cap) for _, off, cap in rows if off is not None)
    for (o0, c0), (o1, _) in zip(placed, placed[1:]):
        assert o0 % 256 == 0 and o0 + c0 <= o1, "256-aligned, no overlap"
    if placed:
        assert placed[-1][0] + placed[-1][1] <= total
    if case == "all zero":
        assert all(off is None and cap == 0 for _, off, cap in rows)
        assert total == sum((((i + 1) * 37) % 509) * 256 for i in range(49)), "the skews count without a buffer"


def test_per_candidate_arrays_do_not_alias(program):
    """Back to back the six arrays lie 32 MiB apart, element (q, i) of all of them in the same HBM channel and bank; the
    skew exists so that no two of them start a multiple of 128 KiB apart."""
    rows, _ = _place(program, NEEDS["per-candidate arrays of 1024 x 8192"])
    start = {name: off for name, off, _ in rows}
    for i, a in enumerate(PER_CANDIDATE):
        for b in PER_CANDIDATE[i + 1:]:
            assert (start[a] - start[b]) % (128 << 10) != 0, (a, b)

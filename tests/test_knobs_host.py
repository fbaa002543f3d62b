"""csrc/knobs.h read_knobs on the host: a stand-alone program (its own main, the host compiler, no HIP) includes the
header, reads the environment this test hands it and prints every field of the Knobs struct.

Every name of the header's table is set to a value that is not its default and the field it feeds is checked; a name
given twice keeps its first value (as getenv); the table's length is tied to the width of the first-occurrence mask by
a static_assert in the header, which the program repeats."""
import subprocess

import pytest

from scann_rust_amd import build

PROGRAM = r"""
#include <stdio.h>
#include "knobs.h"
static_assert(scann::kKnobCount <= 32, "one bit of the mask per name");
int main(int argc, char **argv) {
    environ = argv + 1;   // the arguments ARE the environment: "NAME=value" strings, NULL-terminated, duplicates kept
    const scann::Knobs k = scann::read_knobs();
    printf("names %d\n", scann::kKnobCount);
    for (int i = 0; i < scann::kKnobCount; ++i) printf("name %s\n", scann::kKnobNames[i]);
    printf("device_slots %d\n", k.device_slots);
    printf("search_slots %u\n", k.search_slots);
    printf("rccl_lib %s\n", k.rccl_lib ? k.rccl_lib : "(null)");
    printf("smfmac %d\n", (int)k.smfmac);
    printf("rerank_i8 %d\n", k.rerank_i8);
    printf("rerank_fp8 %d\n", (int)k.rerank_fp8);
    printf("rerank_uniform %d\n", k.rerank_uniform);
    printf("bf_shortlist_min_rows %u\n", k.bf_shortlist_min_rows);
    printf("load_pin %d\n", (int)k.load_pin);
    printf("small %d\n", (int)k.small);
    printf("wide %d\n", k.wide);
    printf("resident %d\n", k.resident);
    printf("res_cl %u\n", k.res_cl);
    printf("mfma %d\n", k.mfma);
    printf("rerank_i8_min %u\n", k.rerank_i8_min);
    printf("rerank_expand %d\n", (int)k.rerank_expand);
    printf("sp_words %d\n", k.sp_words);
    printf("sp_pairs %d\n", k.sp_pairs);
    printf("sp_bitmap %d\n", (int)k.sp_bitmap);
    printf("thr_ties %d\n", (int)k.thr_ties);
    printf("thr_tail %d\n", (int)k.thr_tail);
    printf("sample_mfma %d\n", (int)k.sample_mfma);
    printf("fused %d\n", (int)k.fused);
    printf("select_direct %d\n", (int)k.select_direct);
    printf("select_regs %d\n", (int)k.select_regs);
    printf("local_prune %d\n", (int)k.local_prune);
    printf("comm_fill %.6f\n", k.comm_fill);
    printf("bf_shortlist_tail %.6f\n", k.bf_shortlist_tail);
    printf("bf_shortlist_min_queries %u\n", k.bf_shortlist_min_queries);
    printf("bf_filter %d\n", k.bf_filter);
    printf("bf_filter_compact_max %.6f\n", k.bf_filter_compact_max);
    return 0;
}
"""

# name: (field, default as printed, a value that is not the default, that value as printed)
TABLE = {
    "SCANN_HIP_DEVICE_SLOTS": ("device_slots", "2", "3", "3"),
    "SCANN_HIP_SEARCH_SLOTS": ("search_slots", "4", "9", "9"),
    "SCANN_HIP_RCCL_LIB": ("rccl_lib", "(null)", "/some/librccl.so", "/some/librccl.so"),
    "SCANN_HIP_SMFMAC": ("smfmac", "1", "0", "0"),
    "SCANN_HIP_RERANK_I8": ("rerank_i8", "1", "2", "2"),
    "SCANN_HIP_RERANK_STORE": ("rerank_fp8", "0", "fp8", "1"),
    "SCANN_HIP_RERANK_UNIFORM": ("rerank_uniform", "1", "0", "0"),
    "SCANN_HIP_BF_SHORTLIST_MIN_ROWS": ("bf_shortlist_min_rows", "65536", "777", "777"),
    "SCANN_HIP_LOAD_PIN": ("load_pin", "1", "0", "0"),
    "SCANN_HIP_SMALL": ("small", "1", "0", "0"),
    "SCANN_HIP_WIDE": ("wide", "1", "2", "2"),
    "SCANN_HIP_RESIDENT": ("resident", "1", "2", "2"),
    "SCANN_HIP_RES_CL": ("res_cl", "0", "3", "3"),
    "SCANN_HIP_MFMA": ("mfma", "1", "3", "3"),
    "SCANN_HIP_RERANK_I8_MIN": ("rerank_i8_min", "512", "100000", "100000"),
    "SCANN_HIP_RERANK_EXPAND": ("rerank_expand", "1", "0", "0"),
    "SCANN_HIP_SP_WORDS": ("sp_words", "-1", "0", "0"),
    "SCANN_HIP_SP_PAIRS": ("sp_pairs", "0", "64", "64"),
    "SCANN_HIP_SP_BITMAP": ("sp_bitmap", "1", "0", "0"),
    "SCANN_HIP_THR_TIES": ("thr_ties", "1", "0", "0"),
    "SCANN_HIP_THR_TAIL": ("thr_tail", "1", "0", "0"),
    "SCANN_HIP_SAMPLE_MFMA": ("sample_mfma", "1", "0", "0"),
    "SCANN_HIP_FUSED": ("fused", "1", "0", "0"),
    "SCANN_HIP_SELECT_DIRECT": ("select_direct", "1", "0", "0"),
    "SCANN_HIP_SELECT_REGS": ("select_regs", "1", "0", "0"),
    "SCANN_HIP_LOCAL_PRUNE": ("local_prune", "1", "0", "0"),
    "SCANN_HIP_COMM_FILL": ("comm_fill", "2.500000", "1.25", "1.250000"),
    "SCANN_HIP_BF_SHORTLIST_TAIL": ("bf_shortlist_tail", "0.000001", "0.5", "0.500000"),
    "SCANN_HIP_BF_SHORTLIST_MIN_QUERIES": ("bf_shortlist_min_queries", "32", "5", "5"),
    "SCANN_HIP_BF_FILTER": ("bf_filter", "0", "2", "2"),
    "SCANN_HIP_BF_FILTER_COMPACT_MAX": ("bf_filter_compact_max", "1.000000", "0.25", "0.250000"),
}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("knobs")
    src, exe = d / "knobs_main.cpp", d / "knobs_main"
    src.write_text(PROGRAM)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + build.CSRC, "-o", str(exe), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def _run(exe, envp):
    """{field: printed value} and the table's names, under an environment given as a LIST of "NAME=value": the program
    takes its arguments as its environ, so that a name can stand in it twice (execve's envp from Python is a dict)"""
    r = subprocess.run([exe] + list(envp), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    fields, names = {}, []
    for line in r.stdout.splitlines():
        key, _, val = line.partition(" ")
        if key == "name":
            names.append(val)
        else:
            fields[key] = val
    return fields, names


def test_the_table_is_the_one_checked_here(program):
    fields, names = _run(program, [])
    assert int(fields.pop("names")) == len(names) <= 32
    assert sorted(names) == sorted(TABLE) and len(set(names)) == len(names)
    assert len({f for f, _, _, _ in TABLE.values()}) == len(TABLE) == len(fields), "one field per name"


def test_defaults(program):
    fields, _ = _run(program, ["PATH=/usr/bin", "SCANN_HIPX=1", "SCANN_HIP_NO_SUCH_KNOB=1", "SCANN_HIP_MFMA"])
    for name, (field, default, _, _) in TABLE.items():
        assert fields[field] == default, (name, fields[field])


def test_every_knob_reaches_its_field(program):
    """all at once (the last name of the table sits in the mask's highest used bit), and each one alone: only its
    own field leaves the default"""
    fields, names = _run(program, ["%s=%s" % (n, v[2]) for n, v in TABLE.items()])
    for name, (field, _, _, printed) in TABLE.items():
        assert fields[field] == printed, (name, fields[field])
    for name, (field, _, value, printed) in TABLE.items():
        fields, _ = _run(program, ["%s=%s" % (name, value)])
        for other, (f, default, _, _) in TABLE.items():
            assert fields[f] == (printed if other == name else default), (name, other, fields[f])


def test_the_first_occurrence_of_a_name_wins(program):
    """every name twice, the non-default value first and the default second -- in the table's order and in reverse, so
    that the first and the last bit of the mask are both set while other names are still to come"""
    for order in (list(TABLE), list(TABLE)[::-1]):
        envp = []
        for name in order:
            field, default, value, _ = TABLE[name]
            second = {"(null)": "/other.so", "0.000001": "0.001"}.get(default, default)
            if name == "SCANN_HIP_RERANK_STORE":
                second = "int8"
            envp += ["%s=%s" % (name, value), "%s=%s" % (name, second)]
        fields, _ = _run(program, envp)
        for name, (field, _, _, printed) in TABLE.items():
            assert fields[field] == printed, (name, fields[field])
    # ... and the other way round: the default first keeps the default
    fields, _ = _run(program, ["SCANN_HIP_SP_BITMAP=1", "SCANN_HIP_SP_BITMAP=0", "SCANN_HIP_BF_FILTER_COMPACT_MAX=1",
                               "SCANN_HIP_BF_FILTER_COMPACT_MAX=0.25"])
    assert fields["sp_bitmap"] == "1" and fields["bf_filter_compact_max"] == "1.000000"

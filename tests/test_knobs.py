"""CPU-only source checks: every SCANN_HIP_* process-environment knob is read by knobs.h alone, listed in its
table and documented in INTEGRATION.md; the knobs that were retired stay gone."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scann_rust_amd", "csrc")
KNOBS_H = os.path.join(CSRC, "knobs.h")
# retired sweep knobs (their defaults are plain code now); spelled in pieces so this file does not name them whole
RETIRED = ["SCANN_HIP_" + n for n in ("SQPT", "QPT", "WGS", "MFMA" + "_WGS", "MFMA" + "_CODES",
                                      "BF_STREAM" + "_MAX_QUERIES")]


def _sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".hip")))


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as fh:
        return fh.read()


def _table():
    """Knob names of the comment table at the top of knobs.h."""
    names = []
    for line in _read(KNOBS_H).splitlines():
        m = re.match(r"//\s+(SCANN_HIP_[A-Z0-9_]+)\s", line)
        if m:
            names.append(m.group(1))
    return names


def test_only_knobs_h_reads_the_environment():
    offenders = [os.path.basename(p) for p in _sources() if p != KNOBS_H and "getenv" in _read(p)]
    assert offenders == []


def test_every_knob_literal_is_in_the_table_and_documented():
    table = _table()
    assert len(table) == len(set(table)) >= 20
    literals = set()
    for p in _sources():
        literals.update(re.findall(r'"SCANN_HIP_([A-Z0-9_]+)', _read(p)))
    assert literals, "knobs.h names its knobs"
    assert sorted("SCANN_HIP_" + n for n in literals if "SCANN_HIP_" + n not in table) == []
    # every name the reader matches is a table entry, and the other way round
    assert sorted("SCANN_HIP_" + n for n in literals) == sorted(table)
    doc = _read(os.path.join(ROOT, "INTEGRATION.md"))
    assert [n for n in table if not re.search(r"`%s`" % n, doc)] == []


def test_retired_knobs_appear_nowhere():
    skip = {"__pycache__", "_obj", "_ref"}   # (and hidden directories: .git, caches)
    me = os.path.abspath(__file__)
    pat = re.compile(r"\b(%s)\b" % "|".join(RETIRED))
    hits = []
    for d, dirs, files in os.walk(ROOT):
        dirs[:] = [x for x in dirs if x not in skip and not x.startswith(".")]
        for f in files:
            path = os.path.join(d, f)
            if path == me or os.path.getsize(path) > (16 << 20):
                continue
            with open(path, "rb") as fh:
                data = fh.read()
            if b"\0" in data[:4096]:
                continue
            hits += ["%s: %s" % (os.path.relpath(path, ROOT), m) for m in pat.findall(data.decode("utf-8", "replace"))]
    assert hits == []

"""An all-pairs matrix over the per-call decisions of a tree / flat-hasher search (api_search.hip plan_txh_search), and a mirror
of the two decisions scann_hip_index_last_kernel_ms reports: the pipeline and the batched scan.

Pure Python: no GPU and no library.  tests/test_knob_matrix.py checks the generator and the mirror's coverage,
tests/test_gpu_knob_matrix.py runs the rows.

A row is a dict {factor: level}.  The level None of a SCANN_HIP_* factor means the variable is removed from the
environment; every other level of such a factor is the variable's value."""
import random

K = 10
NQ_MAX = 230
ENTRIES = ("host", "stages", "shared", "perq", "device", "device-shared")
FACTORS = (
    ("nq", (1, 4, 16, 17, 40, NQ_MAX)),
    ("m", (600, 2000)),
    ("entry", ENTRIES),
    ("SCANN_HIP_SMALL", (None, "0")),
    ("SCANN_HIP_WIDE", (None, "0", "2")),
    ("SCANN_HIP_FUSED", (None, "0")),
    ("SCANN_HIP_MFMA", (None, "0", "2", "3")),
    ("SCANN_HIP_SMFMAC", (None, "0")),
    ("SCANN_HIP_RESIDENT", (None, "0", "2")),
    ("SCANN_HIP_RES_CL", (None, "1", "3")),
    ("SCANN_HIP_SP_WORDS", (None, "0", "1")),
    ("SCANN_HIP_SP_PAIRS", (None, "32", "64")),
    ("SCANN_HIP_SP_BITMAP", (None, "0")),
    ("SCANN_HIP_THR_TIES", (None, "0")),
    ("SCANN_HIP_THR_TAIL", (None, "0")),
    ("SCANN_HIP_SAMPLE_MFMA", (None, "0")),
    ("SCANN_HIP_SELECT_DIRECT", (None, "0")),
    ("SCANN_HIP_SELECT_REGS", (None, "0")),
    ("SCANN_HIP_RERANK_I8_MIN", (None, "1", "100000")),
    ("SCANN_HIP_RERANK_EXPAND", (None, "0")),
)
KNOBS = tuple(name for name, _ in FACTORS if name.startswith("SCANN_HIP_"))
SEED = 20
KERNELS = ("small_scan_kernel", "wide_scan_kernel", "adc_scan_kernel", "adc_scan_res_kernel", "adc_mfma_kernel",
           "adc_mfma16_kernel", "adc_smfmac_kernel")

# csrc/txh.h
SMALL_BATCH, SMALL_MAX_CANDIDATES, SMALL_MAX_STREAM = 16, 1024, 262144
WIDE_BATCH, WIDE_MAX_CANDIDATES, WIDE_MAX_STREAM, WIDE_MIN_STREAM = 4, 8192, 4 << 20, 16384
SCAN_PPT, RES_THREADS, RES_QUADS = 2, 512, 4
FUSED_CHUNK, FUSED_MAX_WGS, DECODE_STAGE, THR_TAIL_MAX_RANK = 1024, 512, 512, 384
SP_RANGE64, SURV_BYTES_MAX = 1024, 512 << 20   # points per 64-pair item; api_search.hip plan_txh_search kSurvBytesMax
S, TREE_P = 16, 3   # subspaces and partitions_to_search of the matrix's indexes (tests/test_gpu_knob_matrix.py)


def all_pairs():
    """every ((factor a, level), (factor b, level)) with a before b in FACTORS"""
    out = set()
    for a in range(len(FACTORS)):
        for b in range(a + 1, len(FACTORS)):
            for la in FACTORS[a][1]:
                for lb in FACTORS[b][1]:
                    out.add(((a, la), (b, lb)))
    return out


def pairs_of(row):
    lv = [row[name] for name, _ in FACTORS]
    return {((a, lv[a]), (b, lv[b])) for a in range(len(lv)) for b in range(a + 1, len(lv))}


def pairwise_rows(seed=SEED, tries=40):
    """Greedy all-pairs rows: each new row is the best of `tries` candidates; a candidate starts from a pair no row
    holds yet and takes, factor by factor in a shuffled order, the level that adds most pairs not yet held (ties to a
    seeded draw).  Deterministic for a seed; no third-party package."""
    rng = random.Random(seed)
    todo = all_pairs()
    nf = len(FACTORS)
    rows = []
    while todo:
        best, best_gain = None, -1
        first = sorted(todo, key=repr)
        for _ in range(tries):
            (a, la), (b, lb) = first[rng.randrange(len(first))]
            lv = {a: la, b: lb}
            order = [f for f in range(nf) if f not in lv]
            rng.shuffle(order)
            for f in order:
                scored = []
                for level in FACTORS[f][1]:
                    g = sum(1 for o, lo in lv.items()
                            if (((o, lo), (f, level)) if o < f else ((f, level), (o, lo))) in todo)
                    scored.append((g, rng.random(), level))
                lv[f] = max(scored, key=lambda s: s[:2])[2]
            row = {FACTORS[f][0]: lv[f] for f in range(nf)}
            gain = len(pairs_of(row) & todo)
            if gain > best_gain:
                best, best_gain = row, gain
        rows.append(best)
        todo -= pairs_of(best)
    return rows


def default_row(**levels):
    """a row with every knob unset; nq, m and entry as given"""
    row = {name: (None if name.startswith("SCANN_HIP_") else lv[0]) for name, lv in FACTORS}
    row.update(levels)
    for name, lv in FACTORS:
        assert row[name] in lv, (name, row[name])
    return row


# Rows appended by hand, so that the mirror below names every kernel at least twice on both index kinds (the dense
# 32-pair MFMA needs SMFMAC = 0 on a staged call with MFMA = 2 or six quads per leaf; the resident scan RESIDENT = 2
# without a prefilter): tests/test_knob_matrix.py test_every_kernel_is_named_twice.
EXTRA_ROWS = (
    default_row(nq=40, m=600, entry="host", SCANN_HIP_MFMA="2", SCANN_HIP_SMFMAC="0"),
    default_row(nq=NQ_MAX, m=2000, entry="device", SCANN_HIP_MFMA="2", SCANN_HIP_SMFMAC="0", SCANN_HIP_SELECT_REGS="0"),
    default_row(nq=17, m=2000, entry="shared", SCANN_HIP_MFMA="0", SCANN_HIP_RESIDENT="2", SCANN_HIP_RES_CL="3"),
    default_row(nq=4, m=600, entry="device", SCANN_HIP_RESIDENT="2", SCANN_HIP_RES_CL="1"),
    default_row(nq=40, m=2000, entry="stages", SCANN_HIP_MFMA="3", SCANN_HIP_THR_TAIL="0"),
    default_row(nq=NQ_MAX, m=600, entry="perq", SCANN_HIP_MFMA="3", SCANN_HIP_SAMPLE_MFMA="0"),
    default_row(nq=1, m=600, entry="host", SCANN_HIP_WIDE="0", SCANN_HIP_FUSED="0"),
    default_row(nq=16, m=600, entry="host", SCANN_HIP_RERANK_I8_MIN="1"),
    default_row(nq=4, m=2000, entry="host", SCANN_HIP_SELECT_DIRECT="0"),
    default_row(nq=1, m=600, entry="host"),
    # (and, on the flat hasher, more than one row each of the 64-pair items, the integer-MFMA sample and the one-launch
    # small pipeline)
    default_row(nq=40, m=600, entry="device-shared"),
    default_row(nq=NQ_MAX, m=2000, entry="shared", SCANN_HIP_MFMA="2", SCANN_HIP_SP_PAIRS="64"),
    default_row(nq=4, m=600, entry="host", SCANN_HIP_WIDE="0"),
)


def matrix_rows(seed=SEED):
    return pairwise_rows(seed) + [dict(r) for r in EXTRA_ROWS]


def row_env(row):
    """{variable: value} of the row's knobs that are set"""
    return {name: row[name] for name in KNOBS if row[name] is not None}


def row_id(row):
    knobs = " ".join("%s=%s" % (name[len("SCANN_HIP_"):], v) for name, v in row_env(row).items())
    return "nq%d m%d %s [%s]" % (row["nq"], row["m"], row["entry"], knobs)


def _int(row, name, unset):
    return unset if row[name] is None else int(row[name])


def expected_plan(row, kind, stream, leaves, P=None):
    """The TxhPlan fields plan_txh_search derives for the row's FIRST attempt on an index of kind "ah" (flat hasher) /
    "txh" (tree) with 4-bit codes, S = 16, operand planes and an int8 / FP8 re-rank store: `stream` = the longest
    stream of P leaves, `leaves` = the leaf sizes.  Unsharded, ADC scan, k = 10.  The sample plan comes from
    tests/helpers.py (sample_plan, sample_rank, plan_caps)."""
    import helpers as H
    n, L = int(sum(leaves)), len(leaves)
    ah = kind == "ah"
    P = 1 if ah else min(TREE_P if P is None else P, L)
    nq, m, k = row["nq"], row["m"], K
    ms = max(1, int(stream))
    small_on = row["SCANN_HIP_SMALL"] is None
    wide = _int(row, "SCANN_HIP_WIDE", 1)
    mfma_knob = _int(row, "SCANN_HIP_MFMA", 1)
    resident_knob = _int(row, "SCANN_HIP_RESIDENT", 1)
    smfmac = row["SCANN_HIP_SMFMAC"] is None
    st, scap = H.sample_plan(ms, P)
    J = H.sample_rank(m, st)
    pipeline = "staged"
    if small_on and nq <= SMALL_BATCH and m <= SMALL_MAX_CANDIDATES and k <= 64 and ms <= SMALL_MAX_STREAM and L <= 4096:
        pipeline = "small"
    limits = (small_on and wide != 0 and nq <= WIDE_BATCH and 1 <= m <= WIDE_MAX_CANDIDATES and k <= 64 and
              ms <= WIDE_MAX_STREAM and L <= 4096 and P <= 512)
    long_leaves = P == 1 or n // max(1, L) >= 512
    pays = ms >= WIDE_MIN_STREAM and ms >= 8 * m and long_leaves
    if limits and (wide == 2 or pays):
        pipeline = "wide"
    no_threshold = pipeline != "staged"
    cap = ms if no_threshold else H.plan_caps(ms, P, m)[2]
    fused = False
    if pipeline == "small":
        grid = max(1, -(-cap // FUSED_CHUNK))
        fused = row["SCANN_HIP_FUSED"] is None and P <= DECODE_STAGE and nq * grid <= FUSED_MAX_WGS and P == 1
    quads = (nq * P + 3) // 4
    qpl = max(1, quads // max(1, L))
    rtp = RES_THREADS * SCAN_PPT
    res_chunks_per_leaf = max(1, (n // max(1, L)) // rtp)
    qgroups = max(1, (qpl + RES_QUADS - 1) // RES_QUADS)
    units = (n // rtp + L) * qgroups
    res_cl = min(64, max(8, units // 4096))
    res_layout = S <= 32
    resident = res_layout and res_chunks_per_leaf >= 8 and qpl >= 32 and units // res_cl >= 1536
    if resident_knob == 0:
        resident = False
    if resident_knob == 2:
        resident = res_layout
    mfma_ok = not no_threshold
    sparse = m * 128 <= ms
    mfma = "gather"
    if mfma_ok and sparse:
        mfma = "mfma32" if qpl >= 6 else "mfma16" if qpl >= 2 else "gather"
    if mfma_knob == 0:
        mfma = "gather"
    if mfma_knob == 2:
        mfma = "mfma32" if mfma_ok else "gather"
    if mfma_knob == 3:
        mfma = "mfma16" if mfma_ok else "gather"
    if mfma_ok and qpl >= 2 and n // max(1, L) >= 4096 and smfmac and mfma_knob not in (0, 3):
        mfma = "smfmac"
    if mfma == "mfma32" and smfmac:
        mfma = "smfmac"
    scan = mfma if mfma != "gather" else "resident" if resident else "gather"
    is_mfma = scan in ("mfma32", "mfma16", "smfmac")
    sp_words = (not ah) if row["SCANN_HIP_SP_WORDS"] is None else int(row["SCANN_HIP_SP_WORDS"]) != 0
    compiled = scan == "smfmac" and S <= 32 and not sp_words
    tiles32 = (quads + 7) // 8
    sp_pairs = _int(row, "SCANN_HIP_SP_PAIRS", 0)
    flat = ah and L == 1 and P == 1
    sp_pairs64 = compiled and (sp_pairs == 64 if sp_pairs else flat and (tiles32 % 2 == 0 or nq > 224))
    # the bitmap form of the 64-pair items: flat hashers, unless the knob says 0 or the bitmaps pass the byte cap
    sp_bitmap_bytes = -(-nq // 64) * 64 * -(-n // SP_RANGE64) * 128
    sp_bitmap = sp_pairs64 and flat and row["SCANN_HIP_SP_BITMAP"] is None and sp_bitmap_bytes <= SURV_BYTES_MAX
    thr_ties = row["SCANN_HIP_THR_TIES"] is None
    thr_tail = row["SCANN_HIP_THR_TAIL"] is None and not no_threshold and J <= THR_TAIL_MAX_RANK and scap > 4096
    sample_mfma = (row["SCANN_HIP_SAMPLE_MFMA"] is None and thr_tail and thr_ties and is_mfma and ah and L == 1 and
                   P == 1)
    use_i8 = m >= _int(row, "SCANN_HIP_RERANK_I8_MIN", 512) and m > 4 * k
    # the host entry keeps queries and rows in pinned memory on a non-staged pipeline, unless the call asks for stage
    # outputs or brings a filter (txh_search_host); the device entry never does
    pinned = row["entry"] == "host" and pipeline != "staged"
    return dict(pipeline=pipeline, scan=scan, pinned=pinned, no_threshold=no_threshold, cap=cap, st=st, scap=scap, J=J,
                fused=fused, thr_tail=thr_tail, sample_mfma=sample_mfma, sp_words=sp_words, sp_pairs64=sp_pairs64,
                sp_bitmap=sp_bitmap, sp_bitmap_bytes=sp_bitmap_bytes if sp_bitmap else 0,
                select_direct=row["SCANN_HIP_SELECT_DIRECT"] is None, select_regs=row["SCANN_HIP_SELECT_REGS"] is None,
                use_i8=use_i8, i8_expand=row["SCANN_HIP_RERANK_EXPAND"] is None)


def expected_kernel(row, kind, stream, leaves, P=None):
    """api_search.hip txh_kernel_name of the row's first attempt: the pinned host call of a non-staged pipeline is named by
    the pipeline's scan, every other call by the batched scan of its plan (also where a small pipeline runs it)"""
    p = expected_plan(row, kind, stream, leaves, P)
    if p["pinned"]:
        return "wide_scan_kernel" if p["pipeline"] == "wide" else "small_scan_kernel"
    return {"gather": "adc_scan_kernel", "resident": "adc_scan_res_kernel", "mfma32": "adc_mfma_kernel",
            "mfma16": "adc_mfma16_kernel", "smfmac": "adc_smfmac_kernel"}[p["scan"]]


# Calls woven into a sequence of rows: checked by their status (and, where the status is Ok, their counts) alone, and
# the rows after them must not notice them.  `status` names a constant of scann_rust_amd.hip.
#   - partitions_to_search = 5000 is clamped to the index's leaves first (plan_txh_search: P = min(P, L), as the
#     reference's tree_partitioner.rs:214 does), so on indexes of <= 4096 leaves it is a search of every leaf -- a
#     longer stream than any row's, Ok; Unimplemented needs more than 4096 leaves.
#   - the refusal a handle of these shapes can reach in plan_txh_search is pre_reorder_k above 8192: Unimplemented.
#   - a query dimensionality that is not the index's: InvalidArgument.
#   - k = 0: the candidate count resolves to 0, the rows are fill_empty's: count 0, and rows of no columns (with
#     k = 0 there is no slot to hold 0xFFFFFFFF / +inf, so the count and the shape (nq, 0) are what is checked).
DISTURBANCES = (
    dict(name="partitions-5000", nq=4, k=K, m=600, partitions_to_search=5000, q_dim=None, status="OK", count=K),
    dict(name="pre-reorder-9000", nq=4, k=K, m=9000, partitions_to_search=None, q_dim=None, status="UNIMPLEMENTED",
         count=None),
    dict(name="wrong-q-dim", nq=4, k=K, m=600, partitions_to_search=None, q_dim=-1, status="INVALID_ARGUMENT",
         count=None),
    dict(name="k-0", nq=17, k=0, m=600, partitions_to_search=None, q_dim=None, status="OK", count=0),
)


def pass1_order(rows):
    """indices of `rows` from the smallest shapes up (nq, then m): every new largest nq asks for longer per-query
    buffers (api_search.hip ensure_txh_workspace: samp, cand, queries, ... are nq x something), so the arena is rebuilt
    several times mid-sequence"""
    return sorted(range(len(rows)), key=lambda i: (rows[i]["nq"], rows[i]["m"], i))


def pass2_order(rows, seed=SEED):
    """a seeded shuffle that starts with the largest row (nq, then m; of those the first): no later call has more
    queries or candidates, so the per-query buffers are at their final size from the first call on (a later row can
    still add a buffer only its path uses, such as the prefilter's survivor list)"""
    first = max(range(len(rows)), key=lambda i: (rows[i]["nq"], rows[i]["m"], -i))
    rest = [i for i in range(len(rows)) if i != first]
    random.Random(seed + 1).shuffle(rest)
    return [first] + rest


def growth_steps(rows, order):
    """how often a call of the sequence, after the first, has more queries than every call before it"""
    steps, top = 0, None
    for i in order:
        if top is not None and rows[i]["nq"] > top:
            steps += 1
        top = rows[i]["nq"] if top is None else max(top, rows[i]["nq"])
    return steps

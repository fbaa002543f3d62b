// knobs.h -- the SCANN_HIP_* process-environment knobs, read in ONE pass over environ.
//
// None of them changes a result.  Every knob is optional; unset means the default below.
//
// knob                              values                                                        read
// --------------------------------  ------------------------------------------------------------  ---------------------
// SCANN_HIP_DEVICE_SLOTS            workspaces of the device entry points, 1..4 (default 2)        once per process
// SCANN_HIP_SEARCH_SLOTS            search slots of the host entry points, 1..64 (default 4)       once per process
// SCANN_HIP_RCCL_LIB                path of librccl tried before the default names                 once per process
// SCANN_HIP_SMFMAC                  0: no operand planes (creation) / dense 32-pair MFMA (search)  creation, every call
// SCANN_HIP_RERANK_I8               8-bit row copy of the re-rank filter: 0 never, 2 always        creation / load
// SCANN_HIP_RERANK_STORE            fp8: that copy in the reference's E4M3 codec (default int8)    creation / load
// SCANN_HIP_RERANK_UNIFORM          int8 copy: 0 a scale per row, 2 one scale (default: rows'      creation / load
//                                   magnitudes within 2 %)
// SCANN_HIP_BF_SHORTLIST_MIN_ROWS   rows from which the bf16 shortlist copy is built (65536)       creation / load
// SCANN_HIP_LOAD_PIN                0: index files skip hipHostRegister                            load
// SCANN_HIP_SMALL                   0: no small-batch / wide pipelines                             every call
// SCANN_HIP_WIDE                    0: never the wide pipeline, 2: wherever its limits allow       every call
// SCANN_HIP_RESIDENT                0: never the resident-table scan, 2: whenever codes allow      every call
// SCANN_HIP_RES_CL                  chunks per tile of the resident-table scan (>= 1)              every call
// SCANN_HIP_MFMA                    0: f32 LUT scan only, 2 / 3: 32- / 16-pair integer-MFMA        every call
//                                   prefilter whenever it applies
// SCANN_HIP_RERANK_I8_MIN           shortest candidate list the int8 filter takes (512)            every call
// SCANN_HIP_RERANK_EXPAND           0: the filter's brackets per dimension, (q - s x8)^2, finished  every call
//                                   round by round (default: one epilogue a wave; one-scale int8
//                                   store by the expanded square; per-row int8 store always as 0)
// SCANN_HIP_SP_WORDS                0 / 1: lane-walk / word-parallel survivor flush of the sparse  every call
//                                   prefilter (default: word-parallel on tree indexes)
// SCANN_HIP_SP_PAIRS                32 / 64: pairs per item of the sparse prefilter, where the     every call
//                                   64-pair form is compiled (S <= 32, lane-walk flush); default:
//                                   by the batch, flat hashers only
// SCANN_HIP_SP_BITMAP               0: 64-pair items of a flat hasher flush their survivors into   every call
//                                   lists inside the scan (default: the scan stores the survivor
//                                   bitmap and the refine walks it)
// SCANN_HIP_THR_TIES                0: filter bound on the distance alone (diagnostics)            every call
// SCANN_HIP_THR_TAIL                0: filter bound by the full histogram select                   every call
// SCANN_HIP_SAMPLE_MFMA             0: flat hashers score the bound's sample with the f32 gather   every call
//                                   (default: integer-MFMA sample, exact re-score of its low tail)
// SCANN_HIP_FUSED                   0: small batches always as three launches                      every call
// SCANN_HIP_SELECT_DIRECT           0: stage long candidate lists in LDS for the unsorted select   every call
// SCANN_HIP_SELECT_REGS             0: that select sweeps its list four times from global memory   every call
//                                   (default: one read, the list ranked in registers)
// SCANN_HIP_LOCAL_PRUNE             0: multi-GPU local stage re-ranks every candidate exactly      every call
// SCANN_HIP_COMM_FILL               multi-GPU: room in a destination block, multiple of the even   every call
//                                   share (2.5; 0 = worst case)
// SCANN_HIP_BF_SHORTLIST_TAIL       miss probability of the bf16 shortlist's bound, (0, 1) (1e-6)  every call
// SCANN_HIP_BF_SHORTLIST_MIN_QUERIES  batch size from which the bf16 shortlist is used (32)        every call
// SCANN_HIP_BF_FILTER              filtered brute force: 1 compacted id list, 2 bit test at the     every call
//                                   emit (default: by the allowed fraction, next knob)
// SCANN_HIP_BF_FILTER_COMPACT_MAX   largest allowed fraction that takes the compacted list, [0, 1]  every call
//                                   (default 1: always)
//
// "every call": one read_knobs() snapshot at the entry point, passed down.
#pragma once

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

extern char **environ;

namespace scann {

struct Knobs {
    int device_slots = 2;                 // (clamped to the slot array by its user)
    uint32_t search_slots = 4;
    const char *rccl_lib = nullptr;
    bool smfmac = true;
    int rerank_i8 = 1;
    bool rerank_fp8 = false;
    int rerank_uniform = 1;
    uint32_t bf_shortlist_min_rows = 65536;
    bool load_pin = true;
    bool small = true;
    int wide = 1;
    int resident = 1;
    uint32_t res_cl = 0;                  // 0 = from the work size
    int mfma = 1;
    uint32_t rerank_i8_min = 512;
    bool rerank_expand = true;
    int sp_words = -1;                    // -1 = by index kind
    int sp_pairs = 0;                     // 0 = by the batch (api_search.hip plan_txh_search)
    bool sp_bitmap = true;
    bool thr_ties = true;
    bool thr_tail = true;
    bool sample_mfma = true;
    bool fused = true;
    bool select_direct = true;
    bool select_regs = true;
    bool local_prune = true;
    double comm_fill = 2.5;
    double bf_shortlist_tail = 1e-6;
    uint32_t bf_shortlist_min_queries = 32;
    int bf_filter = 0;                    // 0 = by bf_filter_compact_max
    double bf_filter_compact_max = 1.0;   // (every fraction: the crossover is not measured yet)
};

// The knobs' names, in the order of the bits of read_knobs' first-occurrence mask.
constexpr const char *kKnobNames[] = {
    "SCANN_HIP_DEVICE_SLOTS", "SCANN_HIP_SEARCH_SLOTS", "SCANN_HIP_RCCL_LIB", "SCANN_HIP_SMFMAC", "SCANN_HIP_RERANK_I8",
    "SCANN_HIP_RERANK_STORE", "SCANN_HIP_RERANK_UNIFORM", "SCANN_HIP_BF_SHORTLIST_MIN_ROWS", "SCANN_HIP_LOAD_PIN",
    "SCANN_HIP_SMALL", "SCANN_HIP_WIDE", "SCANN_HIP_RESIDENT", "SCANN_HIP_RES_CL", "SCANN_HIP_MFMA",
    "SCANN_HIP_RERANK_I8_MIN", "SCANN_HIP_RERANK_EXPAND", "SCANN_HIP_SP_WORDS", "SCANN_HIP_SP_PAIRS",
    "SCANN_HIP_SP_BITMAP", "SCANN_HIP_THR_TIES", "SCANN_HIP_THR_TAIL", "SCANN_HIP_SAMPLE_MFMA", "SCANN_HIP_FUSED",
    "SCANN_HIP_SELECT_DIRECT", "SCANN_HIP_SELECT_REGS", "SCANN_HIP_LOCAL_PRUNE", "SCANN_HIP_COMM_FILL",
    "SCANN_HIP_BF_SHORTLIST_TAIL", "SCANN_HIP_BF_SHORTLIST_MIN_QUERIES", "SCANN_HIP_BF_FILTER",
    "SCANN_HIP_BF_FILTER_COMPACT_MAX"};
constexpr int kKnobCount = (int)(sizeof(kKnobNames) / sizeof(kKnobNames[0]));
static_assert(kKnobCount <= 32, "read_knobs tracks first occurrences in a 32-bit mask: one bit per name, widen `seen` first");

// The first occurrence of a name wins, as with getenv.
inline Knobs read_knobs() {
    Knobs k;
    uint32_t seen = 0;
    for (char **ep = environ; ep && *ep; ++ep) {
        const char *e = *ep;
        if (strncmp(e, "SCANN_HIP_", 10) != 0) continue;
        const char *eq = strchr(e, '=');
        if (!eq) continue;
        const size_t n = (size_t)(eq - e);
        const char *v = eq + 1;
        int id = -1;
        for (int i = 0; i < kKnobCount && id < 0; ++i)
            if (strlen(kKnobNames[i]) == n && memcmp(kKnobNames[i], e, n) == 0) id = i;
        if (id < 0 || ((seen >> id) & 1u)) continue;
        seen |= 1u << id;
        auto is = [&](const char *s) { return strcmp(kKnobNames[id], s) == 0; };
        if (is("SCANN_HIP_DEVICE_SLOTS")) k.device_slots = atoi(v);
        else if (is("SCANN_HIP_SEARCH_SLOTS")) k.search_slots = (uint32_t)std::max(1, std::min(64, atoi(v)));
        else if (is("SCANN_HIP_RCCL_LIB")) k.rccl_lib = v;
        else if (is("SCANN_HIP_SMFMAC")) k.smfmac = atoi(v) != 0;
        else if (is("SCANN_HIP_RERANK_I8")) k.rerank_i8 = atoi(v);
        else if (is("SCANN_HIP_RERANK_STORE")) k.rerank_fp8 = strcmp(v, "fp8") == 0;
        else if (is("SCANN_HIP_RERANK_UNIFORM")) k.rerank_uniform = atoi(v);
        else if (is("SCANN_HIP_BF_SHORTLIST_MIN_ROWS")) k.bf_shortlist_min_rows = (uint32_t)strtoul(v, nullptr, 10);
        else if (is("SCANN_HIP_LOAD_PIN")) k.load_pin = atoi(v) != 0;
        else if (is("SCANN_HIP_SMALL")) k.small = atoi(v) != 0;
        else if (is("SCANN_HIP_WIDE")) k.wide = atoi(v);
        else if (is("SCANN_HIP_RESIDENT")) k.resident = atoi(v);
        else if (is("SCANN_HIP_RES_CL")) k.res_cl = (uint32_t)std::max(1, atoi(v));
        else if (is("SCANN_HIP_MFMA")) k.mfma = atoi(v);
        else if (is("SCANN_HIP_RERANK_I8_MIN")) k.rerank_i8_min = (uint32_t)std::max(1, atoi(v));
        else if (is("SCANN_HIP_RERANK_EXPAND")) k.rerank_expand = atoi(v) != 0;
        else if (is("SCANN_HIP_SP_WORDS")) k.sp_words = atoi(v) != 0 ? 1 : 0;
        else if (is("SCANN_HIP_SP_PAIRS")) {
            const int n = atoi(v);
            if (n == 32 || n == 64) k.sp_pairs = n;
        } else if (is("SCANN_HIP_SP_BITMAP")) k.sp_bitmap = atoi(v) != 0;
        else if (is("SCANN_HIP_THR_TIES")) k.thr_ties = atoi(v) != 0;
        else if (is("SCANN_HIP_THR_TAIL")) k.thr_tail = atoi(v) != 0;
        else if (is("SCANN_HIP_SAMPLE_MFMA")) k.sample_mfma = atoi(v) != 0;
        else if (is("SCANN_HIP_FUSED")) k.fused = atoi(v) != 0;
        else if (is("SCANN_HIP_SELECT_DIRECT")) k.select_direct = atoi(v) != 0;
        else if (is("SCANN_HIP_SELECT_REGS")) k.select_regs = atoi(v) != 0;
        else if (is("SCANN_HIP_LOCAL_PRUNE")) k.local_prune = atoi(v) != 0;
        else if (is("SCANN_HIP_COMM_FILL")) {
            const double f = atof(v);
            k.comm_fill = f < 0.0 ? 0.0 : f;
        } else if (is("SCANN_HIP_BF_SHORTLIST_TAIL")) {
            const double t = atof(v);
            if (t > 0.0 && t < 1.0) k.bf_shortlist_tail = t;
        } else if (is("SCANN_HIP_BF_SHORTLIST_MIN_QUERIES")) k.bf_shortlist_min_queries = (uint32_t)strtoul(v, nullptr, 10);
        else if (is("SCANN_HIP_BF_FILTER")) k.bf_filter = atoi(v);
        else if (is("SCANN_HIP_BF_FILTER_COMPACT_MAX")) {
            const double f = atof(v);
            if (f >= 0.0 && f <= 1.0) k.bf_filter_compact_max = f;
        }
    }
    return k;
}

}  // namespace scann

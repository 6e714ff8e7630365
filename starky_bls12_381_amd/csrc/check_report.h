// Host half of starkhip_check_trace_report, the same for the device path (check_trace.hip: check_trace_report) and for the replay without a
// device (check_report.cpp: check_trace_report_replay): argument checks, the summary, the selection of the constraints that are
// listed, the order of the list and its truncation.  What differs is who runs the two passes (kernels_check.hip, or host loops).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "airs.h"
#include "trace_input.h"

namespace starkhip {

// THE rule for trace lengths (prove(), ctx_reserve() and the trace checkers): the built-in AIRs keep the reference's largest trace
// (8192 rows; their layouts are the reference's), a registered AIR goes up to 2^STARKHIP_MAX_LOG_ROWS.  That bound comes from the quotient kernel's 32-bit byte offsets into one LDE column
// (kernels_quotient.hip: N * 8 < 2^32 with rate_bits <= 8).
inline unsigned max_log_rows(const AirInfo& air) { return air.id >= STARKHIP_AIR_CUSTOM_BASE ? (unsigned)STARKHIP_MAX_LOG_ROWS : 13u; }
// ... and for log2(rows): true and *log_n = log2(n_rows) for a power of two from 2 on, false for every other count
inline bool log2_rows(size_t n_rows, unsigned* log_n) {
    unsigned l = 0;
    while (l < 63 && ((size_t)1 << l) < n_rows) l++;
    *log_n = l;
    return n_rows >= 2 && ((size_t)1 << l) == n_rows;
}

// What starkhip_check_trace and the report refuse with BAD_SHAPE: rows that are no power of two in 2 .. 2^max_log_rows(air), a public
// input that is not canonical.  *log_n = log2(n_rows).
int check_trace_shape(const AirInfo& air, size_t n_rows, const uint64_t* pis, unsigned* log_n);

// The rows of a mask of W words as list entries, in ascending row order: an entry is the n_lead words of `lead`, then the row, and goes
// to list[(n_lead + 1) * *listed] while *listed < cap.  Returns the popcount of the whole mask, listed or not.
inline uint64_t mask_to_list(const uint64_t* mask, size_t W, const uint64_t* lead, size_t n_lead, uint64_t* list, size_t cap, uint64_t* listed) {
    uint64_t bits = 0;
    for (size_t w = 0; w < W; w++) {
        uint64_t word = mask[w];
        bits += (uint64_t)__builtin_popcountll(word);
        for (; word && *listed < cap; word &= word - 1) {
            uint64_t* e = list + (n_lead + 1) * (*listed)++;
            for (size_t i = 0; i < n_lead; i++) e[i] = lead[i];
            e[n_lead] = w * 64 + (size_t)__builtin_ctzll(word);
        }
    }
    return bits;
}

struct CheckPasses {
    virtual ~CheckPasses() {}
    // counts[k] (zeroed, n_constraints entries) = rows on which constraint k is violated; mask (zeroed, (n + 63) / 64 words) = those rows
    virtual int count(uint32_t* counts, uint64_t* mask) = 0;
    // entries[3 * (base[k] + i)] = {k, row, value} for the counts[k] violations of every constraint with base[k] != ~0, in any order of
    // i; `total` entries in all.  `mask` is what count() gave.
    virtual int list(const uint32_t* base, const uint64_t* mask, size_t total, uint64_t* entries) = 0;
};

int check_report_run(const AirProgram& P, size_t n_rows, CheckPasses& passes, uint32_t* per_constraint, uint64_t* row_mask, uint64_t* list,
                     size_t cap, starkhip_check_report_t* out);

int check_trace_report_replay(const AirInfo& air, const TraceInput& in, const uint64_t* pis, uint32_t* per_constraint, uint64_t* row_mask,
                              uint64_t* list, size_t cap, starkhip_check_report_t* out);

// The check blob a prove() with "check_trace" hands back for a violating trace (starkhip.h has the table): CHECK_BLOB_HEADER words
// {magic, AIR id, n_rows, violations, constraints_violated, rows_violated, listed, 0}, then the report's list.  From malloc, never
// from the proof arena: starkhip_free releases it like a proof.  nullptr: out of memory.
static const size_t CHECK_BLOB_HEADER = 8;
uint64_t* check_blob_make(int air, size_t n_rows, const starkhip_check_report_t& rep, const uint64_t* list, size_t* words);
// *list points into the blob; false for anything that is not exactly one check blob
bool check_blob_read(const uint64_t* blob, size_t words, starkhip_check_report_t* out, const uint64_t** list);
// what prove() must hand back for this trace with "check_trace_list" = cap, without a device: STARKHIP_OK and no blob, or
// STARKHIP_ERR_TRACE and the blob (check_trace_report_replay underneath)
int check_blob_replay(const AirInfo& air, const TraceInput& in, const uint64_t* pis, size_t cap, uint64_t** blob, size_t* words);

}  // namespace starkhip

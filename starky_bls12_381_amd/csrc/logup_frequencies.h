// Host half of starkhip_logup_frequencies (starkhip.h has the rule), the same for the device path (logup_frequencies.hip over
// kernels_multiset.hip and kernels_logup_freq.hip) and for the replay without a device (logup_frequencies.cpp): the plan of an AIR's
// lookups, the fillable test, the argument checks, the loop over the batches, the counts, the list from the masks in its fixed order
// and the report.  What differs is who runs one batch: device steps, or host loops.
//
// The rule, for one lookup over n rows with m looked-up columns, t = its table column and f = its frequencies column, cells read mod p:
//   row r of t is a FIRST when no row r' < r has t[r'] = t[r]; a looked-up cell is MISSING when its value occurs nowhere in t.  When
//   no cell is missing, f[r] = the number of the m n looked-up cells equal to t[r] on a first and 0 elsewhere.  Otherwise f stays as it
//   was, and the rows with a missing cell are the lookup's missing rows.
//
// A lookup over Columns and Filters (logup.h) follows the same rule with values for cells: the keys of a table are its Column's values,
// and a looked-up cell (c, r) is SKIPPED when its filter phi_c(r) is 0, looked up and counted when phi_c(r) is 1, and FLAGGED when
// phi_c(r) is anything else -- the fill needs a multiplicity, and the argument would need phi as one.  Flagged cells count as missing,
// in the same masks, counters, list and LogUp blob, whose layouts do not change.
//
// The lookups of a call run in BATCHES of G consecutive lookups (logup_freq_batch_size): one set of launches and one wait for the
// missing counts on the device.  The same file has the LogUp blob a prove() with "fill_frequencies" hands back for a trace some lookup
// of which fails.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/starkhip.h"
#include "trace_input.h"

namespace starkhip {

// An AIR is FILLABLE when every frequencies Column is one plain local column (coefficient 1, constant 0) that no Column or Filter of
// any lookup reads and that is no other lookup's frequencies column: then the order of the lookups does not matter.  `why` (may be null) gets the reason of a refusal.
bool logup_fillable(const AirProgram& P, std::string* why);

// The lookups of a fillable program as the steps want them.  The looked-up values of all lookups are numbered back to back in
// declaration order (sum m), those of lookup q from col_off[q] to col_off[q + 1]; freq: the frequencies columns; table_of[q]: the
// first lookup with the same table Column (compared structurally: the distinct tables of a batch); named: the distinct columns a fill
// READS, ascending.  A program of plain lookups (general == false) also has cols and table, the looked-up and the table columns, and
// runs the kernels over columns; any other runs the ones that evaluate Columns and Filters.  `prog` must outlive the plan.
struct LogupFreqPlan {
    size_t L = 0;
    const AirProgram* prog = nullptr;
    bool general = false;
    size_t desc_words = 0;  // what one batch's descriptor takes at most
    std::vector<uint32_t> cols, col_off, table, table_of, freq, named;
    explicit LogupFreqPlan(const AirProgram& P);
    size_t n_values() const { return col_off.back(); }
    size_t m(size_t q) const { return col_off[q + 1] - col_off[q]; }
};

// Table rows (n per distinct table of a batch) whose sorted items one context keeps: a memory choice, as LOOKUP_ITEM_BUDGET
static const size_t LOGUP_FREQ_ITEM_BUDGET = (size_t)1 << 22;
// G: the lookups of one batch -- all of them where they fit the budget, never fewer than one
inline size_t logup_freq_batch_size(size_t n_rows, size_t n_lookups) {
    return std::max<size_t>(1, std::min(n_lookups, LOGUP_FREQ_ITEM_BUDGET / std::max<size_t>(1, n_rows)));
}

// BAD_SHAPE for what the entries refuse of their arguments (the AIR is the caller's to judge: BAD_AIR comes first)
int logup_freq_args(const AirInfo& air, const TraceInput& in, const uint64_t* list, size_t cap, const void* out);

struct LogupFreqSteps {
    virtual ~LogupFreqSteps() {}
    // the g lookups from q0 on as one batch: col_missing[k] = the missing cells of looked-up column col_off[q0] + k; the frequencies
    // column of a lookup is written when it has none and, where the trace is the caller's, only then
    virtual int run(size_t q0, size_t g, uint32_t* col_missing) = 0;
    // the mask of lookup i of the last batch: (n + 63) / 64 words
    virtual int mask(size_t i, uint64_t* out) = 0;
};

// per_lookup [L], per_column [sum m], masks [L][(n + 63) / 64], list [cap][2]: each may be null (list only with cap == 0)
int logup_freq_run(size_t n_rows, const LogupFreqPlan& plan, size_t batch, LogupFreqSteps& steps, uint32_t* per_lookup, uint32_t* per_column, uint64_t* masks,
                   uint64_t* list, size_t cap, starkhip_logup_report_t* out);

int logup_frequencies_replay(const AirInfo& air, const TraceInput& in, uint64_t* words, uint32_t* per_lookup, uint32_t* per_column, uint64_t* masks, uint64_t* list,
                             size_t cap, starkhip_logup_report_t* out);

// The LogUp blob (starkhip.h has the table): LOGUP_BLOB_HEADER words {magic, AIR id, n_rows, lookups, lookups_failed, missing_rows,
// listed, missing_cells}, then listed x {lookup, row}.  From malloc like a check blob: starkhip_free releases it.  nullptr: out of memory.
static const size_t LOGUP_BLOB_HEADER = 8;
uint64_t* logup_blob_make(int air, size_t n_rows, const starkhip_logup_report_t& rep, const uint64_t* list, size_t* words);
// *list points into the blob; false for anything that is not exactly one LogUp blob
bool logup_blob_read(const uint64_t* blob, size_t words, starkhip_logup_report_t* out, const uint64_t** list);
// what a prove() with "fill_frequencies" and "check_trace_list" = cap must hand back for this trace of a fillable AIR with LogUp
// lookups, without a device: STARKHIP_OK and no blob, or STARKHIP_ERR_TRACE and the blob (the replay on a copy of the trace)
int logup_blob_replay(const AirInfo& air, const TraceInput& in, size_t cap, uint64_t** blob, size_t* words);

}  // namespace starkhip

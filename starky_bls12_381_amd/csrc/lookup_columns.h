// Host half of starkhip_lookup_columns (starkhip.h has the rule), the same for the device path (lookup_columns.hip over
// kernels_multiset.hip and kernels_lookup.hip) and for the replay without a device (lookup_columns.cpp): the argument checks, the loop
// over the lookups, the counts, the list from the masks in its fixed order and the report.  What differs is who runs one lookup:
// device steps, or host loops.
//
// The rule, for one lookup over n rows with a = its input column and t = its table column, cells read mod p:
//   A = a sorted ascending, T = t sorted ascending; permuted_input = A.  Position i of A is a HEAD when i = 0 or A[i] != A[i - 1];
//   position j of T is USED when it is the first of T holding its value and that value occurs in a.  When every value of a occurs in
//   t, permuted_table[i] = A[i] on every head, and the k-th non-head position of A takes the k-th unused entry of T.  Otherwise the
//   input rows whose value t does not hold are the lookup's MISSING rows and its two output columns stay as they were.
//
// The lookups of a call run in BATCHES of G (lookup_batch_size): one set of launches and one wait for the G missing counts on the
// device, G runs of the host loops in the replay.  The same file has what an AIR registered with its lookups needs (starkhip.h:
// starkhip_air_register_lookups): the check of a list against a program, and the lookup blob a prove() with "fill_lookups" hands back
// for a trace some lookup of which fails.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "../../include/starkhip.h"
#include "trace_input.h"

namespace starkhip {

// The caller's trace is dense and written in place: `in` is the view of it every trace entry gets, `words` the same memory, writable
// (host memory, or device memory when in.on_device).
// BAD_SHAPE for what the entries refuse of their arguments
int lookup_args(const TraceInput& in, const starkhip_lookup_t* lookups, size_t n_lookups, const uint64_t* list, size_t cap, const void* out);

// The rule lookup_args applies to the columns of a list, with a reason: every column inside n_cols, the two outputs of a lookup
// distinct, an output column no lookup's input or table and nobody else's output; 1 .. STARKHIP_LOOKUPS_MAX lookups
bool lookup_list_ok(size_t n_cols, const starkhip_lookup_t* lookups, size_t n_lookups, std::string* why);
// ... and what starkhip_air_check_lookups adds for a program: it declares the pairs [(input, permuted_input)] and [(table,
// permuted_table)] of every lookup, or the fill would write columns that the proof does not bind
bool air_lookups_ok(const AirProgram& P, const starkhip_lookup_t* lookups, size_t n_lookups, std::string* why);

// Items (2 n per lookup) whose buffers one context keeps for a batch: DESIGN.md 13c has the reason -- a memory choice.  One lookup of
// the longest trace (2^20 rows) is half of it.
static const size_t LOOKUP_ITEM_BUDGET = (size_t)1 << 22;
// G: the lookups of one batch -- all of them where they fit the budget, never fewer than one, at most `limit` when that is not 0
// ("lookup_batch")
inline size_t lookup_batch_size(size_t n_rows, size_t n_lookups, size_t limit) {
    size_t g = std::min(n_lookups, std::max<size_t>(1, LOOKUP_ITEM_BUDGET / (2 * n_rows)));
    if (limit) g = std::min(g, limit);
    return std::max<size_t>(1, g);
}

struct LookupSteps {
    virtual ~LookupSteps() {}
    // the g lookups from q0 on as one batch: missing[i] = the missing rows of lookup q0 + i; its two output columns are written when
    // that is 0 and, where the trace is the caller's, only then
    virtual int run(size_t q0, const starkhip_lookup_t* lks, size_t g, uint64_t* missing) = 0;
    // the mask of lookup i of the last batch: (n + 63) / 64 words
    virtual int mask(size_t i, uint64_t* out) = 0;
};

// batch: G.  The counts, the list and the report do not depend on it.
int lookup_run(size_t n_rows, const starkhip_lookup_t* lookups, size_t n_lookups, size_t batch, LookupSteps& steps, uint32_t* per_lookup, uint64_t* masks,
               uint64_t* list, size_t cap, starkhip_lookup_report_t* out);

int lookup_columns_replay(const TraceInput& in, uint64_t* words, const starkhip_lookup_t* lookups, size_t n_lookups, uint32_t* per_lookup, uint64_t* masks,
                          uint64_t* list, size_t cap, starkhip_lookup_report_t* out, size_t batch = 0);

// The lookup blob (starkhip.h has the table): LOOKUP_BLOB_HEADER words {magic, AIR id, n_rows, lookups, lookups_failed, missing_rows,
// listed, 0}, then listed x {lookup, row}.  From malloc like a check blob: starkhip_free releases it.  nullptr: out of memory.
static const size_t LOOKUP_BLOB_HEADER = 8;
uint64_t* lookup_blob_make(int air, size_t n_rows, const starkhip_lookup_report_t& rep, const uint64_t* list, size_t* words);
// *list points into the blob; false for anything that is not exactly one lookup blob
bool lookup_blob_read(const uint64_t* blob, size_t words, starkhip_lookup_report_t* out, const uint64_t** list);
// what a prove() with "fill_lookups" and "check_trace_list" = cap must hand back for this trace of an AIR registered with lookups,
// without a device: STARKHIP_OK and no blob, or STARKHIP_ERR_TRACE and the blob (lookup_columns_replay on a copy of the trace)
int lookup_blob_replay(const AirInfo& air, const TraceInput& in, size_t cap, uint64_t** blob, size_t* words);

}  // namespace starkhip

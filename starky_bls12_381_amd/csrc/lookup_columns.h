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
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/starkhip.h"
#include "trace_input.h"

namespace starkhip {

// The caller's trace is dense and written in place: `in` is the view of it every trace entry gets, `words` the same memory, writable
// (host memory, or device memory when in.on_device).
// BAD_SHAPE for what the entries refuse of their arguments
int lookup_args(const TraceInput& in, const starkhip_lookup_t* lookups, size_t n_lookups, const uint64_t* list, size_t cap, const void* out);

struct LookupSteps {
    virtual ~LookupSteps() {}
    // lookup q: *missing = its missing rows; the two output columns are written when, and only when, that is 0
    virtual int run(size_t q, const starkhip_lookup_t& lk, uint64_t* missing) = 0;
    // the mask of the last run: (n + 63) / 64 words
    virtual int mask(uint64_t* out) = 0;
};

int lookup_run(size_t n_rows, const starkhip_lookup_t* lookups, size_t n_lookups, LookupSteps& steps, uint32_t* per_lookup, uint64_t* masks,
               uint64_t* list, size_t cap, starkhip_lookup_report_t* out);

int lookup_columns_replay(const TraceInput& in, uint64_t* words, const starkhip_lookup_t* lookups, size_t n_lookups, uint32_t* per_lookup, uint64_t* masks,
                          uint64_t* list, size_t cap, starkhip_lookup_report_t* out);

}  // namespace starkhip

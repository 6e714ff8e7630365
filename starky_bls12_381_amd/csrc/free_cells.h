// starkhip_check_trace_free_cell_classes and starkhip_check_trace_free_cells: which cells of a trace could change by delta without any
// constraint noticing, and why not.  What the device path (check_trace.hip: free_cell_classes_run, kernels_free_classes.hip) and the
// replay without a device (free_cells.cpp) share: the compiled form of an AIR the kernel walks, the summaries of the per-column
// counts, and the projection that makes the audit's result out of the classes'.
//
// The rule.  An OCCURRENCE is constraint k reading column c as a local or as a next cell: a pivot of compile_free_cells.  It puts
// cell (r, c) in a frame -- a read as a local cell in frame r, a read as a next cell in frame (r - 1) mod n -- and COUNTS when k
// applies to that frame (constraint_applies, air_ir.h).  On that frame, with this one cell replaced by cell + delta (only this
// occurrence's read changed), G' is the product of the group's gates (1 without gates) and body' the constraint's body.  Three bits
// per cell, over its counting occurrences:
//   read: there is one;  open: some has G' != 0;  caught: some has G' * body' != 0.
// read contains open contains caught.  CAUGHT = caught, SILENT = open and not caught, GATED = read and not open, UNREAD = not read.
// G' is taken AFTER the change: a pivot that is itself a gate opens or closes its own gate.  Per constraint k and on the UNCHANGED
// trace, open_rows[k] is the number of frames r that k applies to with G(frame r) != 0.
//
// The audit (starkhip_check_trace_free_cells) asks for less: cell (r, c) is caught when some constraint that reads column c is nonzero
// on the frame that read puts the cell in, with this one cell replaced by cell + delta -- the caught bit above -- and every other
// cell is FREE: the silent, gated and unread ones together.  free_cells_from_classes is that projection.
//
// Cells are read mod p; the trace need not satisfy the AIR; the result is a pure function of the arguments.  Two limits: one cell at
// a time (necessary, not sufficient), and probabilistic in delta (per occurrence, at most `degree` values of delta turn a caught cell
// silent or an open one gated).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "airs.h"
#include "gl.h"
#include "trace_input.h"
#include "quotient_ops.h"

namespace starkhip {

// One constraint of the op stream of compile_quotient_ops, as the free-cell kernel re-walks it: the ops of its group's GROUP + GATE
// ops, the ops of its own terms (the last one carries QOP_FOLD), and its pivots -- the distinct (column | REF_NEXT) references
// among those gates and its factors.  32 bytes: one scalar fetch.
struct FreeCon {
    uint32_t g0, g1;      // [g0, g1) the GROUP op and the group's gates
    uint32_t t0, t1;      // [t0, t1) the constraint's FACTOR / TERM ops
    uint32_t piv0, piv1;  // [piv0, piv1) its pivots in FreeProgram::pivots
    uint32_t kind, pad;   // KIND_*
};
static_assert(sizeof(FreeCon) == 32, "FreeCon is fetched as 8 dwords");

struct FreeProgram {
    std::vector<FreeCon> cons;     // [n_constraints], op indices into Q.ops
    std::vector<uint32_t> pivots;  // column | REF_NEXT
};
FreeProgram compile_free_cells(const QProgram& Q);

// what both entries refuse of their delta, at the C entries, on the device path and in the replay
inline bool free_cells_bad_delta(uint64_t delta) { return delta == 0 || delta >= GL_P; }

// The classes: per_column is [n_cols][3] (silent, gated, unread rows of each column), planes [3][n_cols][(n_rows + 63) / 64] (read, open,
// caught), open_rows [n_constraints].  The summary from the first and the last:
starkhip_free_cell_classes_t free_cell_classes_summary(const uint32_t* per_column, const uint32_t* open_rows, size_t n_rows, size_t n_cols,
                                                       size_t n_constraints);
// and the rule as host loops over air_constraint_parts_at on changed frames, one thread: for tests at small shapes.
int check_trace_free_cell_classes_replay(const AirInfo& air, const TraceInput& in, const uint64_t* pis, uint64_t delta, uint32_t* per_column,
                                         uint64_t* planes, uint32_t* open_rows, starkhip_free_cell_classes_t* out);

// The audit from the classes.  cells, free cells, wholly and partly free columns from the free rows of each column:
starkhip_free_cells_t free_cells_summary(const uint32_t* per_column, size_t n_rows, size_t n_cols);
// The projection, for the device path and the replay alike: per_column[c] (may be NULL) = silent + gated + unread of column c; `mask`
// (may be NULL) holds the caught plane [n_cols][(n_rows + 63) / 64] and is complemented in place on the live rows, so that bits at
// or beyond n_rows stay zero; the summary of the free rows is returned.
starkhip_free_cells_t free_cells_from_classes(const uint32_t* class_per_column, size_t n_rows, size_t n_cols, uint32_t* per_column, uint64_t* mask);
// check_trace_free_cell_classes_replay and that projection.
int check_trace_free_cells_replay(const AirInfo& air, const TraceInput& in, const uint64_t* pis, uint64_t delta, uint32_t* per_column,
                                  uint64_t* free_mask, starkhip_free_cells_t* out);

}  // namespace starkhip

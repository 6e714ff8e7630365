// starkhip_check_trace_free_cells: which cells of a trace could change by delta without any constraint noticing.  What the device
// path (check_trace.hip: check_trace_free_cells, kernels_free_cells.hip) and the replay without a device (free_cells.cpp) share: the
// compiled form of an AIR the kernel walks, and the summary of the per-column counts.
//
// The rule.  Cell (r, c) is CAUGHT when some constraint k reads column c and is nonzero on the frame that read puts the cell in,
// with this one cell replaced by cell + delta: a read as a local cell tests frame r, a read as a next cell frame (r - 1) mod n, and
// k has to apply to that frame (constraint_applies, air_ir.h).  Every other cell is FREE.
//
// starkhip_check_trace_free_cell_classes (check_trace_free_cell_classes, kernels_free_classes.hip, and its replay here) tells the free
// cells apart.  An OCCURRENCE is constraint k reading column c as a local or as a next cell: a pivot of compile_free_cells.  It puts
// cell (r, c) in frame r or (r - 1) mod n as above and COUNTS when k applies to that frame.  On that frame, with this one cell replaced
// by cell + delta (only this occurrence's read changed), G' is the product of the group's gates (1 without gates) and body' the
// constraint's body.  Three bits per cell, over its counting occurrences:
//   read: there is one;  open: some has G' != 0;  caught: some has G' * body' != 0, the rule above bit for bit.
// read contains open contains caught.  CAUGHT = caught, SILENT = open and not caught, GATED = read and not open, UNREAD = not read;
// the last three partition the FREE cells.  G' is taken AFTER the change: a pivot that is itself a gate opens or closes its own gate.
// Per constraint k and on the UNCHANGED trace, open_rows[k] is the number of frames r that k applies to with G(frame r) != 0.
// Cells are read mod p; the trace need not satisfy the AIR; the result is a pure function of the arguments.  Two limits, the
// audit's: one cell at a time (necessary, not sufficient), and probabilistic in delta (per occurrence, at most `degree` values of
// delta turn a caught cell silent or an open one gated).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "airs.h"
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

// cells, free cells, wholly and partly free columns from the free rows of each column
starkhip_free_cells_t free_cells_summary(const uint32_t* per_column, size_t n_rows, size_t n_cols);

// The rule above as host loops over air_constraint_value_at on changed frames, one thread: for tests at small shapes.
int check_trace_free_cells_replay(const AirInfo& air, const TraceInput& in, const uint64_t* pis, uint64_t delta, uint32_t* per_column,
                                  uint64_t* free_mask, starkhip_free_cells_t* out);

// The classes: per_column is [n_cols][3] (silent, gated, unread rows of each column), planes [3][n_cols][(n_rows + 63) / 64] (read, open,
// caught), open_rows [n_constraints].  The summary from the first and the last:
starkhip_free_cell_classes_t free_cell_classes_summary(const uint32_t* per_column, const uint32_t* open_rows, size_t n_rows, size_t n_cols,
                                                       size_t n_constraints);
// and the rule as host loops over air_constraint_parts_at on changed frames, one thread: for tests at small shapes.
int check_trace_free_cell_classes_replay(const AirInfo& air, const TraceInput& in, const uint64_t* pis, uint64_t delta, uint32_t* per_column,
                                         uint64_t* planes, uint32_t* open_rows, starkhip_free_cell_classes_t* out);

}  // namespace starkhip

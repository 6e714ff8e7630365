// Validator of a caller's serialised constraint program (air_ir.h, magic SAIR_IR1) and the per-constraint host evaluator the
// trace checker reports with.
//
// A registered program goes straight into the quotient kernels, the plan builder and the verifiers, which index the LDE and the
// opened rows by its cell references without further checks.  air_parse_checked() is the one gate in front of them: what it
// accepts parses exactly by the grammar of air_ir.h, every reference is inside the declared columns, public inputs and const
// table, and the declared degree covers every constraint by AirBuilder::emit's rule.  The limits (STARKHIP_AIR_MAX_*) are in
// include/starkhip.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <functional>
#include <string>

#include "../../include/starkhip.h"
#include "air_ir.h"
#include "ctl.h"

namespace starkhip {

// The reason of a refusal goes to *why (may be NULL).  On success *out holds the program, group tables included.
bool air_parse_checked(const uint64_t* blob, size_t words, AirProgram* out, std::string* why);

// The same gate for a system blob (ctl.h; cross-table lookups, COMPAT.md 2d).  air_of(id): the program of a registered AIR, or null.
// Refused with a reason: a table id that is no registered AIR, a table with permutation pairs or of degree 1, an endpoint whose table is
// out of range, a width mismatch between a CTL's endpoints, a column outside its table's n_cols, a Column or Filter beyond the LogUp
// term limits, nA + nC above STARKHIP_AIR_MAX_LOGUP_POLYS for some table, a blob that ends early or late.
bool system_parse_checked(const uint64_t* blob, size_t words, const std::function<const AirProgram*(int)>& air_of, SystemProgram* out, std::string* why);

// mask-free value G * body of constraint k (0 <= k < n_constraints) on one frame: what oracle_check_trace compares with zero
gl_t air_constraint_value(const AirProgram& P, uint32_t k, const gl_t* local, const gl_t* next, const gl_t* pis);
// the same for a caller that knows where the constraint is: the code words of its group and of its own first term
gl_t air_constraint_value_at(const AirProgram& P, uint32_t group_word, uint32_t term_word, const gl_t* local, const gl_t* next, const gl_t* pis);
// the two factors of that value apart: *G the product of the group's gates (1 for a group without gates), *body the constraint's
// body, both canonical.  What the free-cell classes ask (free_cells.h): was the gate open, and did the body notice?
void air_constraint_parts_at(const AirProgram& P, uint32_t group_word, uint32_t term_word, const gl_t* local, const gl_t* next, const gl_t* pis,
                             gl_t* G, gl_t* body);

}  // namespace starkhip

// Host half of starkhip_check_trace_permutations (starkhip.h has the rule), the same for the device path (permutation_check.hip
// over kernels_multiset.hip) and for the replay without a device (permutation_check.cpp): the argument checks,
// the seed sequence, the rerun of a pair whose keys collided, undecided pairs, the counts, the list from the masks in its fixed order
// and the summary.  What differs is who runs one pair under one seed: three device steps, or host loops.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "airs.h"
#include "gl.h"
#include "trace_input.h"

namespace starkhip {

inline bool perm_check_bad_seed(uint64_t seed) { return seed < 2 || seed >= GL_P; }
// the seed after s: 7 s + 1 mod p, again while that is below 2
inline gl_t perm_check_next_seed(gl_t s) {
    do s = gl_add(gl_mul(7, s), 1);
    while (s < 2);
    return s;
}
inline void perm_check_seeds(uint64_t seed, uint64_t out[STARKHIP_PERM_CHECK_ATTEMPTS]) {
    for (int k = 0; k < STARKHIP_PERM_CHECK_ATTEMPTS; k++, seed = perm_check_next_seed(seed)) out[k] = seed;
}

// BAD_AIR for an AIR without pairs, BAD_SHAPE for what the entry refuses of its arguments after TraceInput::check
int perm_check_args(const AirInfo* air, const TraceInput& in, uint64_t seed, const uint64_t* list, size_t cap, const void* out);

struct PermCheckSteps {
    virtual ~PermCheckSteps() {}
    // pair q under `seed`: counts = {items whose key equals their predecessor's while their tuple differs, unmatched lhs rows, unmatched
    // rhs rows}; the last two mean something only when the first is 0
    virtual int run(size_t q, gl_t seed, uint64_t counts[3]) = 0;
    // the masks of the last run: [2][(n + 63) / 64]
    virtual int masks(uint64_t* out) = 0;
};

int perm_check_run(const AirProgram& P, size_t n_rows, PermCheckSteps& steps, uint64_t seed, uint32_t* per_pair, uint64_t* masks, uint64_t* list,
                   size_t cap, starkhip_perm_check_t* out);

int check_trace_permutations_replay(const AirInfo& air, const TraceInput& in, uint64_t seed, uint32_t* per_pair, uint64_t* masks, uint64_t* list,
                                    size_t cap, starkhip_perm_check_t* out);

}  // namespace starkhip

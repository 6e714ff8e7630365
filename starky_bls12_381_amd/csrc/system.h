// Systems of tables tied by cross-table lookups (ctl.h; COMPAT.md 2d): the registry, and what the system prover (system.cpp) and the
// system verifier (verifier_system.cpp) share.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/starkhip.h"
#include "ctl.h"

namespace starkhip {

struct SystemInfo {
    int id;
    SystemProgram prog;
    std::vector<CtlTable> tables;  // prog.table(t), built once
    std::vector<uint64_t> blob;
};
// nullptr for an unknown id; registered systems live for the process lifetime
const SystemInfo* system_get(int id);
// the configs of a system's tables may differ in rate_bits only
inline bool system_configs_ok(const starkhip_config_t* cfgs, size_t T) {
    if (!cfgs) return false;
    for (size_t t = 1; t < T; t++) {
        starkhip_config_t a = cfgs[0], b = cfgs[t];
        a.rate_bits = b.rate_bits = 0;
        if (a.security_bits != b.security_bits || a.num_challenges != b.num_challenges || a.cap_height != b.cap_height || a.proof_of_work_bits != b.proof_of_work_bits ||
            a.arity_bits != b.arity_bits || a.final_poly_bits != b.final_poly_bits || a.num_query_rounds != b.num_query_rounds)
            return false;
    }
    return true;
}
// the T + 1 offsets of a system proof blob, checked against its length
bool system_proof_offsets(const uint64_t* blob, size_t words, std::vector<size_t>* off);

}  // namespace starkhip

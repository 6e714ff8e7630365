// Registry of the AIRs this library can prove (one per `impl Stark for ...` in the reference).
#pragma once
#include <vector>

#include "../../include/starkhip.h"
#include "air_ir.h"

namespace starkhip {

struct AirInfo {
    int id;
    const char* name;
    uint32_t cols, pis, degree, default_rows;
    AirProgram prog;
    std::vector<uint64_t> blob;  // prog.serialize()
    // the lookups a registration named (starkhip_air_register_lookups): whose permuted columns "fill_lookups" fills.  Witness
    // information: no verifier reads it and it is no part of the blob.  Empty for built-in AIRs and plain registrations.
    std::vector<starkhip_lookup_t> lookups;
    std::vector<uint64_t> key;   // registered AIRs: what the registry tells them apart by -- the blob's length, the blob, the list
};

// nullptr for an unknown id.  Programs are built on first use and cached for the process lifetime.  Registered AIRs (ids from
// STARKHIP_AIR_CUSTOM_BASE on) are looked up without a lock, so air_get is safe beside a registration on another thread.
const AirInfo* air_get(int id);

// Registers a program that passed air_parse_checked (starkhip_air_register): STARKHIP_OK and *id, or STARKHIP_ERR_BAD_AIR when the
// registry is full.  The key is (blob, lookups): the same two again return their first id, and the same blob with another list --
// or with none -- is another AIR with an id of its own.  `lookups` passed air_lookups_ok (lookup_columns.h) or is empty.
int air_register(AirProgram&& prog, const std::vector<uint64_t>& blob, const char* name, uint32_t default_rows, int* id,
                 const std::vector<starkhip_lookup_t>& lookups = {});

// builders (air_*.cpp)
AirProgram build_air_fibonacci();
AirProgram build_air_fp12_mul();
AirProgram build_air_final_exp();
AirProgram build_air_miller_loop();
AirProgram build_air_pairing_precomp();
AirProgram build_air_ecc_aggregate();

}  // namespace starkhip

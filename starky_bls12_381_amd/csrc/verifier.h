// The verifier's two halves (verifier.cpp, verifier_device.cpp): the prelude every path shares -- shape checks, the
// Fiat-Shamir replay, proof of work, query indices and the quotient identity at zeta -- and the query phase, which the CPU
// verifier runs on host threads and the device verifier on the GPU (verify_query.h).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "airs.h"
#include "proof.h"

namespace starkhip {

struct Ctx;

// What the query phase takes from the transcript
struct VerifyPrelude {
    ProofLayout pl;
    FriGeometry geo;
    gl2_t zeta, gzeta, fri_alpha;
    gl2_t red[2];         // the reduced openings: sum_j alpha^j open_j at zeta (trace, [Zs,] then quotient) and at g zeta (trace [, Zs])
    gl2_t alpha_pow_C;    // alpha^(C + nZ): the length of the g zeta batch
    std::vector<gl2_t> betas;
    std::vector<size_t> indices;
};

// STARKHIP_OK: the queries decide; STARKHIP_ERR_BAD_SHAPE / STARKHIP_ERR_VERIFY: the proof's result, except that with
// check_query_words = false the words of the query section are not range-checked here, and a word >= p there must still turn a
// VERIFY into BAD_SHAPE (the CPU verifier checks every word before it looks at any).  `out->pl` is valid unless BAD_SHAPE.
// `ctl`: the proof is a table's of a system (verifier_system.cpp; COMPAT.md C7) -- its endpoints, the challenger after the system
// transcript, from which the table's transcript starts without observing its trace cap again, and the CTL challenges.  Null: a proof on
// its own, and one whose header names CTL polynomials is BAD_SHAPE.
struct CtlTable;
struct Challenger;
struct CtlVerify {
    const CtlTable* table;
    const Challenger* initial;
    gl_t challenges[4];
};
int verify_prelude(const AirInfo& air, const starkhip_config_t& cfg, const uint64_t* proof, size_t words, bool check_query_words,
                   VerifyPrelude* out, const CtlVerify* ctl = nullptr);
// the CPU verifier of one proof (verifier.cpp): the prelude, then the query rounds on host threads
int verify_proof(const AirInfo& air, const starkhip_config_t& cfg, const uint64_t* proof, size_t words, const CtlVerify* ctl);
// the system verifier (verifier_system.cpp): the system transcript replayed from the table proofs' trace caps, every table proof from the
// copied state, every CTL's sum equation under both challenges; one verdict
struct SystemProgram;
int verify_system_proof(const SystemProgram& sys, const starkhip_config_t* cfgs, const uint64_t* blob, size_t words);

// starkhip_verify_batch: results[i] = starkhip_verify's code for proof i; the return value describes the call
int verify_batch_device(Ctx* c, size_t n, const starkhip_air_t* airs, const starkhip_config_t* cfgs, const uint64_t* const* proofs,
                        const size_t* proof_words, int* results);
// the same host side with the query phase replayed on the CPU through verify_query.h (tests)
int verify_batch_replay(size_t n, const starkhip_air_t* airs, const starkhip_config_t* cfgs, const uint64_t* const* proofs,
                        const size_t* proof_words, int* results);

// per context (ctx.hip): the device-memory cap of one chunk of a batch ("verify_chunk_mb") and the last batch's timings
// [host prelude ms, upload ms, device ms, host CPU seconds]
long ctx_verify_chunk_mb(Ctx* c);
double* ctx_verify_timings(Ctx* c);
int ctx_device(Ctx* c);

}  // namespace starkhip

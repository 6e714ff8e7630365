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
int verify_prelude(const AirInfo& air, const starkhip_config_t& cfg, const uint64_t* proof, size_t words, bool check_query_words,
                   VerifyPrelude* out);

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

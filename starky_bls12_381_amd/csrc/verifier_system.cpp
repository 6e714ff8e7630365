// CPU verifier of a system proof (cross-table lookups; COMPAT.md C1 - C8), written from the verifier's equations: the system transcript
// replayed from the table proofs' trace caps, every table proof checked by verify_proof from a copy of that state -- the four CTL
// constraints at zeta go through ctl_eval_folded with the sums the proof carries --, then every CTL's sum equation under both challenges.
#include <vector>

#include "airs.h"
#include "ctl.h"
#include "poseidon.h"
#include "proof.h"
#include "system.h"
#include "verifier.h"

namespace starkhip {

bool system_proof_offsets(const uint64_t* blob, size_t words, std::vector<size_t>* off) {
    if (!blob || words < 3 || blob[0] != STARKHIP_SYSTEM_PROOF_MAGIC) return false;
    const uint64_t T = blob[1];
    if (T < 2 || T > SYSTEM_MAX_TABLES || words < 3 + T) return false;
    off->assign(blob + 2, blob + 3 + T);
    if ((*off)[0] != 3 + T || (*off)[T] != words) return false;
    for (size_t t = 0; t < T; t++)
        if ((*off)[t + 1] < (*off)[t] + 16 || (*off)[t + 1] > words) return false;
    return true;
}

int verify_system_proof(const SystemProgram& sys, const starkhip_config_t* cfgs, const uint64_t* blob, size_t words) {
    const size_t T = sys.airs.size();
    std::vector<size_t> off;
    if (!system_proof_offsets(blob, words, &off) || off.size() != T + 1 || !system_configs_ok(cfgs, T)) return STARKHIP_ERR_BAD_SHAPE;
    // C1: a fresh challenger under the proofs' hasher observes the trace cap of table 0, 1, .. and draws beta_0, gamma_0, beta_1, gamma_1
    std::vector<ProofLayout> pls(T);
    for (size_t t = 0; t < T; t++) {
        if (!pls[t].read_header(blob + off[t], off[t + 1] - off[t])) return STARKHIP_ERR_BAD_SHAPE;
        if (pls[t].hasher != pls[0].hasher) return STARKHIP_ERR_BAD_SHAPE;  // every table under the same hasher
        for (size_t i = 0; i < 4 * pls[t].ncap; i++)
            if (blob[off[t] + pls[t].mat[0].off_cap + i] >= GL_P) return STARKHIP_ERR_BAD_SHAPE;
    }
    Challenger ch((int)pls[0].hasher);
    for (size_t t = 0; t < T; t++) ch.observe_many(blob + off[t] + pls[t].mat[0].off_cap, 4 * pls[t].ncap);
    CtlVerify cv;
    for (gl_t& x : cv.challenges) x = ch.get();
    cv.initial = &ch;
    // C7: every table proof from the copied state
    std::vector<std::vector<gl_t>> sums_of(T);
    for (size_t t = 0; t < T; t++) {
        const AirInfo* a = air_get(sys.airs[t]);
        if (!a) return STARKHIP_ERR_BAD_AIR;
        const CtlTable table = sys.table((uint32_t)t);
        cv.table = &table;
        if (int rc = verify_proof(*a, cfgs[t], blob + off[t], off[t + 1] - off[t], &cv); rc != STARKHIP_OK) return rc;
        sums_of[t].assign(blob + off[t] + pls[t].off_sums, blob + off[t] + pls[t].off_sums + pls[t].nC / 2);
    }
    // ... and every CTL's sums: looking = looked, under both challenges
    return ctl_first_unbalanced(sys, sums_of) < 0 ? STARKHIP_OK : STARKHIP_ERR_VERIFY;
}

}  // namespace starkhip

// What the device verifier's two users share (verifier_device.cpp): starkhip_verify_batch, one call at a time, and a pool's
// VerifyService (verify_service.cpp), which packs proofs into a persistent arena as their preludes finish.  Both build the same
// descriptors (a chunk), enqueue the same launch sequence and decode the results the same way.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "verifier.h"
#include "verify_query.h"

namespace starkhip {

struct VerifyItem {
    int code = STARKHIP_OK;
    bool queries = false;  // the prelude passed: the query rounds decide
    VerifyPrelude pre;
};

// one proof's prelude with verify_batch's rules (BAD_AIR for an unknown id, BAD_SHAPE for a NULL proof, a VERIFY from the prelude
// turned into BAD_SHAPE when a query word is >= p)
void verify_prelude_item(int air, const starkhip_config_t& cfg, const uint64_t* proof, size_t words, VerifyItem* it);

// device bytes of one proof in a chunk (its region, powers of alpha, digests, sums, descriptors and results)
size_t verify_device_bytes(const ProofLayout& pl);

struct VerifyChunk {
    std::vector<size_t> ids;  // the caller's indices of its proofs
    std::vector<VQProof> proofs;
    std::vector<VQLeaf> leaves;
    std::vector<uint32_t> query_proof;
    std::vector<uint64_t> x_index;
    std::vector<gl2_t> alphas;  // per proof: the FRI alpha
    size_t words = 0, apow = 0, digests = 0, bytes = 0;
    unsigned hashers = 0;  // bit h: the chunk holds a proof of hasher h (which leaf-digest kernels run)
};
void verify_chunk_add(VerifyChunk& ch, size_t id, const VerifyPrelude& pre);
void verify_chunk_seal(VerifyChunk& ch);  // the leaves longest first

// the chunk's device buffers
struct VerifyDevBufs {
    gl_t *words = nullptr, *dig = nullptr;
    gl2_t *apow = nullptr, *sums = nullptr;
    VQProof* proofs = nullptr;
    VQLeaf* leaves = nullptr;
    uint32_t *qproof = nullptr, *status = nullptr, *bad = nullptr;
    uint64_t* xidx = nullptr;
};
// carve the buffers of `ch` out of `cap` bytes at `base` (each 256-byte aligned); false if they do not fit
bool verify_bufs_carve(const VerifyChunk& ch, void* base, size_t cap, VerifyDevBufs* out);
const size_t VERIFY_CARVE_SLACK = 10 * 256;  // what the alignment of the ten buffers may add to verify_device_bytes

// the two pieces of proof k's region: (source, words, destination word)
struct VerifyPiece {
    const uint64_t* src;
    size_t words, dst;
};
void verify_pieces(const VerifyChunk& ch, size_t k, const uint64_t* proof, const ProofLayout& pl, VerifyPiece out[2]);

// host -> device copies of proof regions: page-locked sources directly, anything else through two page-locked staging halves
// (allocated at the first pageable copy when `staging` is NULL and `lazy`)
struct VerifyStaging {
    void* mem = nullptr;
    hipEvent_t sev[2] = {nullptr, nullptr};
    bool used[2] = {false, false};
    unsigned half = 0;
    bool lazy = true;
    hipError_t copy(gl_t* dst, const uint64_t* src, size_t words, bool pinned, hipStream_t st);
};
extern const size_t VERIFY_STAGING_HALF;  // bytes per staging half

// descriptors up, range flags cleared: everything but the proof regions
hipError_t verify_chunk_upload_descriptors(const VerifyChunk& ch, const VerifyDevBufs& b, hipStream_t st);
// the kernel chain: powers of alpha, range check, leaf digests, fri_combine_initial's sums, the per-query checks
hipError_t verify_chunk_launch(const VerifyChunk& ch, const VerifyDevBufs& b, hipStream_t st);
// per proof of the chunk: BAD_SHAPE if its range flag is set, VERIFY if any query failed, else OK
void verify_chunk_codes(const VerifyChunk& ch, const uint32_t* status, const uint32_t* bad, const size_t* n_queries, int* codes);

// the device's part on the host (the replay, and the stand-in device of the sanitizer builds): range flags, powers of alpha, leaf
// digests through the host permutation, the sums and verify_query.h per query, on buffers laid out as on the device
void verify_host_range(const gl_t* words, const VQProof* proofs, size_t n, uint32_t* bad);
void verify_host_ext_powers(gl2_t* out, gl2_t alpha, size_t n);
void verify_host_leaf_digests(const gl_t* words, const VQLeaf* leaves, size_t n, gl_t* digests);
void verify_host_combine(const gl_t* words, const VQProof* proofs, const uint32_t* query_proof, size_t n_queries, const gl2_t* apow, gl2_t* sums);
void verify_host_queries(const gl_t* words, const VQProof* proofs, const uint32_t* query_proof, const uint64_t* x_index, size_t n_queries,
                         const gl_t* digests, const gl2_t* sums, uint32_t* status);

}  // namespace starkhip

// Device verifier: starkhip_verify_batch (and its CPU replay, starkhip_verify_batch_replay).  Per proof, the host runs the
// prelude the CPU verifier runs (verify_prelude: shapes, the Fiat-Shamir replay, proof of work, the quotient identity at zeta) on
// a bounded set of threads; the query rounds -- a leaf re-hash of C / 8 permutations per query and a dot product of C terms, the
// verifier's bulk -- go to the GPU in chunks of proofs whose device footprint stays under the context's "verify_chunk_mb":
//   upload   each proof's caps, FRI caps, query rounds and final polynomial (page-locked pool blobs directly, anything else through
//            two page-locked staging halves)
//   kernels  range check of the query sections, the row-form digests of every opened leaf (longest first), powers of the FRI
//            alpha and fri_combine_initial's sums, then one lane per query for the Merkle paths and the FRI layers (verify_query.h)
//   result   one status word per query and one range flag per proof; BAD_SHAPE wins over VERIFY, as on the CPU.
#include <hip/hip_runtime.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>
#include <type_traits>
#include <vector>

#include "airs.h"
#include "blob_arena.h"
#include "kernels.h"
#include "poseidon.h"
#include "proof.h"
#include "prover.h"
#include "scheduler.h"
#include "verifier.h"
#include "verify_chunk.h"
#include "verify_query.h"

namespace starkhip {

const size_t VERIFY_STAGING_HALF = (size_t)32 << 20;  // bytes per page-locked staging half

namespace {

bool query_words_in_range(const uint64_t* proof, const ProofLayout& pl) {
    for (size_t i = pl.off_queries; i < pl.off_final; i++)
        if (proof[i] >= GL_P) return false;
    return true;
}

// A proof's words in the chunk's buffer: [trace cap | (Z cap) | quotient cap] then [FRI caps .. final polynomial] of the blob
size_t head_words(const ProofLayout& pl) { return pl.quotient().off_cap + 4 * pl.ncap - pl.mat[0].off_cap; }  // from the first matrix's cap through the last's
size_t region_words(const ProofLayout& pl) { return head_words(pl) + (pl.off_pow - pl.off_fri_caps); }

}  // namespace

void verify_prelude_item(int id, const starkhip_config_t& cfg, const uint64_t* proof, size_t words, VerifyItem* it) {
    const AirInfo* a = air_get(id);
    if (!a) {
        it->code = STARKHIP_ERR_BAD_AIR;
        return;
    }
    if (!proof) {
        it->code = STARKHIP_ERR_BAD_SHAPE;
        return;
    }
    const int rc = verify_prelude(*a, cfg, proof, words, false, &it->pre);
    if (rc == STARKHIP_OK) it->queries = true;
    else if (rc == STARKHIP_ERR_VERIFY) it->code = query_words_in_range(proof, it->pre.pl) ? STARKHIP_ERR_VERIFY : STARKHIP_ERR_BAD_SHAPE;
    else it->code = rc;
}

size_t verify_device_bytes(const ProofLayout& pl) {
    const size_t per_query = (pl.n_mats + pl.L) * (4 * 8 + sizeof(VQLeaf)) + 2 * sizeof(gl2_t) + 8 + 4 + 4;
    return 8 * region_words(pl) + sizeof(gl2_t) * pl.batch_cols[0] + pl.n_queries * per_query + sizeof(VQProof) + 4;
}

void verify_chunk_add(VerifyChunk& ch, size_t id, const VerifyPrelude& pre) {
    const ProofLayout& pl = pre.pl;
    VQProof P;
    memset(&P, 0, sizeof P);
    const size_t h = head_words(pl);
    P.base = ch.words;
    P.query_words = pl.query_words;
    P.off_quot_cap = pl.quotient().off_cap - pl.mat[0].off_cap;
    P.off_zs_cap = 4 * pl.ncap;
    P.nZ = (uint32_t)pl.middle();  // the middle matrix, whichever kind
    P.off_fri_caps = h;
    P.off_queries = h + (pl.off_queries - pl.off_fri_caps);
    P.off_final = h + (pl.off_final - pl.off_fri_caps);
    P.apow = ch.apow;
    P.C = (uint32_t)pl.C;
    P.Q = (uint32_t)pl.Q;
    P.L = (uint32_t)pl.L;
    P.log_N = (uint32_t)pl.log_N;
    P.cap_h = (uint32_t)pl.cap_h;
    P.final_len = (uint32_t)pl.final_len;
    P.first_query = (uint32_t)ch.query_proof.size();
    P.first_digest = (uint32_t)ch.digests;
    P.hasher = (uint32_t)pl.hasher;
    ch.hashers |= 1u << P.hasher;
    for (size_t l = 0; l < pl.L; l++) {
        P.arity_bits[l] = pre.geo.arities[l];
        P.layer_depth[l] = (uint32_t)pl.layer_depth[l];
        P.betas[l] = pre.betas[l];
    }
    P.zeta = pre.zeta;
    P.gzeta = pre.gzeta;
    P.red0 = pre.red[0];
    P.red1 = pre.red[1];
    P.alpha_pow_C = pre.alpha_pow_C;
    const size_t d0 = pl.log_N - pl.cap_h, per_q = vq_slots(P);
    for (size_t q = 0; q < pl.n_queries; q++) {
        const uint32_t slot = (uint32_t)(ch.digests + q * per_q);
        size_t o = P.base + P.off_queries + q * pl.query_words;
        for (size_t k = 0; k < pl.n_mats; k++) {  // digest slots (verify_query.h): 0 trace, 1 quotient, 2 + l the layers, 2 + L the Zs
            const uint32_t at = k == 0 ? 0 : k + 1 == pl.n_mats ? 1 : (uint32_t)(2 + pl.L);
            ch.leaves.push_back(VQLeaf{o + pl.mat[k].q_leaf, (uint32_t)pl.mat[k].cols, slot + at, P.hasher, 0});
        }
        o += pl.quotient().q_sib + 4 * d0;
        for (size_t l = 0; l < pl.L; l++) {
            const size_t arity = (size_t)1 << pre.geo.arities[l];
            ch.leaves.push_back(VQLeaf{o, (uint32_t)(2 * arity), (uint32_t)(slot + 2 + l), P.hasher, 0});
            o += 2 * arity + 4 * pl.layer_depth[l];
        }
        ch.query_proof.push_back((uint32_t)ch.proofs.size());
        ch.x_index.push_back(pre.indices[q]);
    }
    ch.proofs.push_back(P);
    ch.ids.push_back(id);
    ch.alphas.push_back(pre.fri_alpha);
    ch.words += region_words(pl);
    ch.apow += pl.batch_cols[0];
    ch.digests += pl.n_queries * per_q;
    ch.bytes += verify_device_bytes(pl);
}

void verify_chunk_seal(VerifyChunk& ch) {
    std::stable_sort(ch.leaves.begin(), ch.leaves.end(), [](const VQLeaf& a, const VQLeaf& b) { return a.len > b.len; });
}

bool verify_bufs_carve(const VerifyChunk& ch, void* base, size_t cap, VerifyDevBufs* b) {
    size_t at = 0;
    bool ok = true;
    auto take = [&](auto** p, size_t count) {
        using T = std::remove_reference_t<decltype(**p)>;
        at = (at + 255) & ~(size_t)255;
        *p = (T*)((char*)base + at);
        at += std::max<size_t>(count, 1) * sizeof(T);
        ok = ok && at <= cap;
    };
    const size_t nq = ch.query_proof.size(), np = ch.proofs.size();
    take(&b->words, ch.words);
    take(&b->apow, ch.apow);
    take(&b->dig, 4 * ch.digests);
    take(&b->sums, 2 * nq);
    take(&b->proofs, np);
    take(&b->leaves, ch.leaves.size());
    take(&b->qproof, nq);
    take(&b->xidx, nq);
    take(&b->status, nq);
    take(&b->bad, np);
    return ok;
}

void verify_pieces(const VerifyChunk& ch, size_t k, const uint64_t* proof, const ProofLayout& pl, VerifyPiece out[2]) {
    const size_t base = ch.proofs[k].base;
    out[0] = VerifyPiece{proof + pl.mat[0].off_cap, head_words(pl), base};
    out[1] = VerifyPiece{proof + pl.off_fri_caps, pl.off_pow - pl.off_fri_caps, base + head_words(pl)};
}

hipError_t VerifyStaging::copy(gl_t* dst, const uint64_t* src, size_t words, bool pinned, hipStream_t st) {
    if (pinned) return hipMemcpyAsync(dst, src, words * 8, hipMemcpyHostToDevice, st);
    if (!mem) {
        if (!lazy) return hipErrorInvalidValue;
        const hipError_t e = hipHostMalloc(&mem, 2 * VERIFY_STAGING_HALF, hipHostMallocDefault);
        if (e != hipSuccess) {
            mem = nullptr;
            return e;
        }
    }
    for (size_t done = 0; done < words;) {  // pageable: through the two staging halves in turn
        const size_t w = std::min(words - done, VERIFY_STAGING_HALF / 8);
        if (used[half]) {
            const hipError_t e = event_wait_sleeping(sev[half]);  // the copy that last read this half has run
            if (e != hipSuccess) return e;
        }
        uint64_t* s = (uint64_t*)mem + half * (VERIFY_STAGING_HALF / 8);
        memcpy(s, src + done, w * 8);
        hipError_t e = hipMemcpyAsync(dst + done, s, w * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipEventRecord(sev[half], st);
        if (e != hipSuccess) return e;
        used[half] = true;
        half ^= 1;
        done += w;
    }
    return hipSuccess;
}

hipError_t verify_chunk_upload_descriptors(const VerifyChunk& ch, const VerifyDevBufs& b, hipStream_t st) {
    hipError_t e = hipMemcpyAsync(b.proofs, ch.proofs.data(), ch.proofs.size() * sizeof(VQProof), hipMemcpyHostToDevice, st);
    if (ch.query_proof.empty()) return e == hipSuccess ? hipMemsetAsync(b.bad, 0, ch.proofs.size() * 4, st) : e;  // num_query_rounds = 0
    if (e == hipSuccess) e = hipMemcpyAsync(b.leaves, ch.leaves.data(), ch.leaves.size() * sizeof(VQLeaf), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(b.qproof, ch.query_proof.data(), ch.query_proof.size() * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(b.xidx, ch.x_index.data(), ch.x_index.size() * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(b.bad, 0, ch.proofs.size() * 4, st);
    return e;
}

hipError_t verify_chunk_launch(const VerifyChunk& ch, const VerifyDevBufs& b, hipStream_t st) {
    hipError_t e = hipSuccess;
    for (size_t k = 0; k < ch.proofs.size() && e == hipSuccess; k++) {
        const VQProof& P = ch.proofs[k];
        e = launch_ext_powers(b.apow + P.apow, ch.alphas[k], P.C + P.nZ + P.Q, st);
    }
    if (e == hipSuccess) e = launch_verify_range(b.words, b.proofs, ch.proofs.size(), b.bad, st);
    if (e == hipSuccess) e = launch_verify_leaf_digests(b.words, b.leaves, ch.leaves.size(), b.dig, ch.hashers, st);
    if (e == hipSuccess) e = launch_verify_combine(b.words, b.proofs, b.qproof, ch.query_proof.size(), b.apow, b.sums, st);
    if (e == hipSuccess) e = launch_verify_queries(b.words, b.proofs, b.qproof, b.xidx, ch.query_proof.size(), b.dig, b.sums, b.status, st);
    return e;
}

void verify_chunk_codes(const VerifyChunk& ch, const uint32_t* status, const uint32_t* bad, const size_t* n_queries, int* codes) {
    for (size_t k = 0; k < ch.ids.size(); k++) {
        const VQProof& P = ch.proofs[k];
        uint32_t any = 0;
        for (size_t q = 0; q < n_queries[k]; q++) any |= status[P.first_query + q];
        codes[k] = bad[k] ? STARKHIP_ERR_BAD_SHAPE : any ? STARKHIP_ERR_VERIFY : STARKHIP_OK;
    }
}

void verify_host_range(const gl_t* W, const VQProof* proofs, size_t n, uint32_t* bad) {
    for (size_t k = 0; k < n; k++) {
        const VQProof& P = proofs[k];
        for (uint64_t i = P.base + P.off_queries; i < P.base + P.off_final; i++) bad[k] |= W[i] >= GL_P;
    }
}

void verify_host_ext_powers(gl2_t* out, gl2_t alpha, size_t n) {
    gl2_t a = gl2_one();
    for (size_t i = 0; i < n; i++, a = gl2_mul(a, alpha)) out[i] = a;
}

void verify_host_leaf_digests(const gl_t* W, const VQLeaf* leaves, size_t n, gl_t* dig) {
    for (size_t k = 0; k < n; k++) {  // hash_or_noop
        const VQLeaf& lf = leaves[k];
        gl_t* out = dig + 4 * (size_t)lf.slot;
        const gl_t* in = W + lf.off;
        if (lf.hasher == STARKHIP_HASHER_KECCAK) {
            keccak_hash_or_noop(in, lf.len, 1, out);
            continue;
        }
        if (lf.len <= 4) {
            for (uint32_t i = 0; i < 4; i++) out[i] = i < lf.len ? in[i] : 0;
            continue;
        }
        gl_t s[12] = {0};
        for (uint32_t off = 0; off < lf.len; off += 8) {
            for (uint32_t i = 0; i < 8 && off + i < lf.len; i++) s[i] = in[off + i];
            poseidon_permute_host(s);
        }
        for (int i = 0; i < 4; i++) out[i] = s[i];
    }
}

void verify_host_combine(const gl_t* W, const VQProof* proofs, const uint32_t* query_proof, size_t n_queries, const gl2_t* apow, gl2_t* sums) {
    for (size_t g = 0; g < n_queries; g++) {
        const VQProof& P = proofs[query_proof[g]];
        const uint32_t qi = (uint32_t)g - P.first_query;
        const gl_t* tleaf = W + P.base + P.off_queries + (uint64_t)qi * P.query_words;
        const gl_t* zleaf = tleaf + P.C + 4 * (P.log_N - P.cap_h);
        const gl_t* qleaf = tleaf + vq_quot_leaf_off(P);
        gl2_t st = gl2_zero(), sq = gl2_zero();
        for (uint32_t c = 0; c < P.C; c++) st = gl2_add(st, gl2_mul_base(apow[P.apow + c], tleaf[c]));
        for (uint32_t z = 0; z < P.nZ; z++) st = gl2_add(st, gl2_mul_base(apow[P.apow + P.C + z], zleaf[z]));
        for (uint32_t q = 0; q < P.Q; q++) sq = gl2_add(sq, gl2_mul_base(apow[P.apow + P.C + P.nZ + q], qleaf[q]));
        sums[2 * g] = gl2_add(st, sq);
        sums[2 * g + 1] = st;
    }
}

void verify_host_queries(const gl_t* W, const VQProof* proofs, const uint32_t* query_proof, const uint64_t* x_index, size_t n_queries,
                         const gl_t* dig, const gl2_t* sums, uint32_t* status) {
    for (size_t g = 0; g < n_queries; g++) {
        const VQProof& P = proofs[query_proof[g]];
        const uint32_t qi = (uint32_t)g - P.first_query;
        status[g] = vq_check_query(P, W + P.base, dig + 4 * ((size_t)P.first_digest + (size_t)qi * vq_slots(P)), sums[2 * g], sums[2 * g + 1],
                                   x_index[g], qi);
    }
}

namespace {

// the preludes of a batch on at most 16 host threads (cpu_budget(): the CPUs this process may use)
void run_preludes(size_t n, const starkhip_air_t* airs, const starkhip_config_t* cfgs, const uint64_t* const* proofs, const size_t* words,
                  std::vector<VerifyItem>& items) {
    items.assign(n, VerifyItem());
    std::atomic<size_t> next(0);
    auto worker = [&]() {
        for (size_t i; (i = next.fetch_add(1)) < n;) {
            int id;  // read as an int: a caller's id need not be one of the enum's values
            memcpy(&id, &airs[i], sizeof id);
            verify_prelude_item(id, cfgs[i], proofs[i], words[i], &items[i]);
        }
    };
    const size_t n_threads = std::min<size_t>({(size_t)16, (size_t)std::max(1u, cpu_budget()), n});
    std::vector<std::thread> pool;
    for (size_t t = 1; t < n_threads; t++) pool.emplace_back(worker);
    worker();
    for (auto& t : pool) t.join();
}

// proofs in batch order, a new chunk whenever the next proof would take the current one past `cap` bytes (a proof bigger than
// the cap gets a chunk of its own); the leaves of a chunk longest first
std::vector<VerifyChunk> make_chunks(const std::vector<VerifyItem>& items, size_t cap) {
    std::vector<VerifyChunk> out;
    for (size_t i = 0; i < items.size(); i++) {
        if (!items[i].queries) continue;
        if (out.empty() || (!out.back().ids.empty() && out.back().bytes + verify_device_bytes(items[i].pre.pl) > cap)) out.emplace_back();
        verify_chunk_add(out.back(), i, items[i].pre);
    }
    for (VerifyChunk& ch : out) verify_chunk_seal(ch);
    return out;
}

// the per-proof results of a chunk from its query statuses and range flags
void chunk_results(const VerifyChunk& ch, const std::vector<uint32_t>& status, const std::vector<uint32_t>& bad, std::vector<VerifyItem>& items) {
    std::vector<size_t> nq(ch.ids.size());
    std::vector<int> codes(ch.ids.size());
    for (size_t k = 0; k < ch.ids.size(); k++) nq[k] = items[ch.ids[k]].pre.pl.n_queries;
    verify_chunk_codes(ch, status.data(), bad.data(), nq.data(), codes.data());
    for (size_t k = 0; k < ch.ids.size(); k++) items[ch.ids[k]].code = codes[k];
}

double process_cpu_s() {
    timespec ts;
    if (clock_gettime(CLOCK_PROCESS_CPUTIME_ID, &ts) != 0) return 0;
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

bool call_args_ok(size_t n, const starkhip_air_t* airs, const starkhip_config_t* cfgs, const uint64_t* const* proofs, const size_t* words,
                  const int* results) {
    return n == 0 || (airs && cfgs && proofs && words && results);
}

// ---- device memory of one call, released on every way out
struct DevMem {
    std::vector<void*> bufs;
    VerifyStaging staging;
    hipStream_t st = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    ~DevMem() {
        if (st) (void)hipStreamSynchronize(st);
        for (void* b : bufs) (void)hipFree(b);
        if (staging.mem) (void)hipHostFree(staging.mem);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : staging.sev)
            if (e) (void)hipEventDestroy(e);
        if (st) (void)hipStreamDestroy(st);
    }
    template <class T>
    hipError_t alloc(T** p, size_t count) {
        void* v = nullptr;
        const hipError_t e = hipMalloc(&v, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) bufs.push_back(v);
        *p = (T*)v;
        return e;
    }
};

}  // namespace

#define VHIP(x)                                                                          \
    do {                                                                                 \
        const hipError_t e_ = (x);                                                       \
        if (e_ != hipSuccess) {                                                          \
            (void)hipGetLastError();                                                     \
            return e_ == hipErrorOutOfMemory ? STARKHIP_ERR_OOM : STARKHIP_ERR_HIP;      \
        }                                                                                \
    } while (0)

int verify_batch_device(Ctx* c, size_t n, const starkhip_air_t* airs, const starkhip_config_t* cfgs, const uint64_t* const* proofs,
                        const size_t* proof_words, int* results) {
    if (!c) return STARKHIP_ERR_NO_DEVICE;
    if (!call_args_ok(n, airs, cfgs, proofs, proof_words, results)) return STARKHIP_ERR_BAD_SHAPE;
    double* tm = ctx_verify_timings(c);
    for (int i = 0; i < 4; i++) tm[i] = 0;
    const double cpu0 = process_cpu_s(), t0 = wall_ms();
    std::vector<VerifyItem> items;
    run_preludes(n, airs, cfgs, proofs, proof_words, items);
    tm[0] = wall_ms() - t0;
    const std::vector<VerifyChunk> chunks = make_chunks(items, (size_t)ctx_verify_chunk_mb(c) << 20);
    if (!chunks.empty()) {
        VHIP(hipSetDevice(ctx_device(c)));
        size_t max_words = 0, max_apow = 0, max_dig = 0, max_q = 0, max_p = 0, max_leaves = 0;
        for (const VerifyChunk& ch : chunks) {
            max_words = std::max(max_words, ch.words);
            max_apow = std::max(max_apow, ch.apow);
            max_dig = std::max(max_dig, ch.digests);
            max_q = std::max(max_q, ch.query_proof.size());
            max_p = std::max(max_p, ch.proofs.size());
            max_leaves = std::max(max_leaves, ch.leaves.size());
        }
        DevMem m;
        VerifyDevBufs b;
        VHIP(m.alloc(&b.words, max_words));
        VHIP(m.alloc(&b.apow, max_apow));
        VHIP(m.alloc(&b.dig, 4 * max_dig));
        VHIP(m.alloc(&b.sums, 2 * max_q));
        VHIP(m.alloc(&b.proofs, max_p));
        VHIP(m.alloc(&b.leaves, max_leaves));
        VHIP(m.alloc(&b.qproof, max_q));
        VHIP(m.alloc(&b.xidx, max_q));
        VHIP(m.alloc(&b.status, max_q));
        VHIP(m.alloc(&b.bad, max_p));
        VHIP(hipStreamCreateWithFlags(&m.st, hipStreamNonBlocking));
        for (hipEvent_t& e : m.ev) VHIP(hipEventCreate(&e));
        for (hipEvent_t& e : m.staging.sev) VHIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        std::vector<uint32_t> status, bad;
        for (const VerifyChunk& ch : chunks) {
            VHIP(hipEventRecord(m.ev[0], m.st));
            VHIP(verify_chunk_upload_descriptors(ch, b, m.st));
            for (size_t k = 0; k < ch.ids.size(); k++) {
                const size_t id = ch.ids[k];
                VerifyPiece pc[2];
                verify_pieces(ch, k, proofs[id], items[id].pre.pl, pc);
                const bool pinned = blob_is_pinned(proofs[id], proof_words[id] * 8);
                for (const VerifyPiece& p : pc) VHIP(m.staging.copy(b.words + p.dst, p.src, p.words, pinned, m.st));
            }
            VHIP(hipEventRecord(m.ev[1], m.st));
            VHIP(verify_chunk_launch(ch, b, m.st));
            VHIP(hipEventRecord(m.ev[2], m.st));
            VHIP(event_wait_sleeping(m.ev[2]));
            status.resize(ch.query_proof.size());
            bad.resize(ch.proofs.size());
            if (!status.empty()) VHIP(hipMemcpy(status.data(), b.status, status.size() * 4, hipMemcpyDeviceToHost));
            VHIP(hipMemcpy(bad.data(), b.bad, bad.size() * 4, hipMemcpyDeviceToHost));
            float up = 0, dev = 0;
            VHIP(hipEventElapsedTime(&up, m.ev[0], m.ev[1]));
            VHIP(hipEventElapsedTime(&dev, m.ev[1], m.ev[2]));
            tm[1] += up;
            tm[2] += dev;
            chunk_results(ch, status, bad, items);
        }
    }
    for (size_t i = 0; i < n; i++) results[i] = items[i].code;
    tm[3] = process_cpu_s() - cpu0;
    return STARKHIP_OK;
}

// The same host side, with the device's work done on the CPU: the region copies into one buffer, the range check, every leaf
// digest through the host permutation, the sums as dot products with the powers of alpha, and verify_query.h per query.
int verify_batch_replay(size_t n, const starkhip_air_t* airs, const starkhip_config_t* cfgs, const uint64_t* const* proofs,
                        const size_t* proof_words, int* results) {
    if (!call_args_ok(n, airs, cfgs, proofs, proof_words, results)) return STARKHIP_ERR_BAD_SHAPE;
    std::vector<VerifyItem> items;
    run_preludes(n, airs, cfgs, proofs, proof_words, items);
    for (const VerifyChunk& ch : make_chunks(items, (size_t)1024 << 20)) {
        std::vector<gl_t> W(ch.words);
        std::vector<uint32_t> bad(ch.proofs.size(), 0), status(ch.query_proof.size(), 0);
        std::vector<gl2_t> apow(ch.apow), sums(2 * ch.query_proof.size());
        std::vector<gl_t> dig(4 * ch.digests);
        for (size_t k = 0; k < ch.ids.size(); k++) {
            const size_t id = ch.ids[k];
            VerifyPiece pc[2];
            verify_pieces(ch, k, proofs[id], items[id].pre.pl, pc);
            for (const VerifyPiece& p : pc) memcpy(W.data() + p.dst, p.src, p.words * 8);
            verify_host_ext_powers(apow.data() + ch.proofs[k].apow, ch.alphas[k], (size_t)ch.proofs[k].C + ch.proofs[k].nZ + ch.proofs[k].Q);
        }
        verify_host_range(W.data(), ch.proofs.data(), ch.proofs.size(), bad.data());
        verify_host_leaf_digests(W.data(), ch.leaves.data(), ch.leaves.size(), dig.data());
        verify_host_combine(W.data(), ch.proofs.data(), ch.query_proof.data(), ch.query_proof.size(), apow.data(), sums.data());
        verify_host_queries(W.data(), ch.proofs.data(), ch.query_proof.data(), ch.x_index.data(), ch.query_proof.size(), dig.data(), sums.data(),
                            status.data());
        chunk_results(ch, status, bad, items);
    }
    for (size_t i = 0; i < n; i++) results[i] = items[i].code;
    return STARKHIP_OK;
}

}  // namespace starkhip

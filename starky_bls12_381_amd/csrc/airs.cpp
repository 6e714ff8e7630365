// AIR registry: builds each built-in constraint program once, on first use, and holds the programs registered at run time.
#include "airs.h"

#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>

namespace starkhip {

namespace {
struct Slot {
    int id;
    const char* name;
    uint32_t default_rows;
    AirProgram (*build)();
    std::once_flag once;
    AirInfo info;
    bool ok = false;
};

// default_rows: the sizes the reference instantiates, /root/reference/src/aggregate_proof.rs:34,77,123,157
Slot g_slots[] = {
    {STARKHIP_AIR_FP12_MUL, "FP12MulStark", 16, build_air_fp12_mul},
    {STARKHIP_AIR_PAIRING_PRECOMP, "PairingPrecompStark", 1024, build_air_pairing_precomp},
    {STARKHIP_AIR_MILLER_LOOP, "MillerLoopStark", 1024, build_air_miller_loop},
    {STARKHIP_AIR_FINAL_EXP, "FinalExponentiateStark", 8192, build_air_final_exp},
    {STARKHIP_AIR_ECC_AGGREGATE, "ECCAggStark", 8192, build_air_ecc_aggregate},  // src/aggregate_proof.rs:188-189
    {STARKHIP_AIR_TEST_FIBONACCI, "TestFibonacci", 64, build_air_fibonacci},
};
// Registered AIRs: entries are published once, with release order, and never change or move afterwards, so a reader needs no lock;
// the registry's mutex orders registrations among themselves.
struct Custom {
    AirInfo info;
    std::string name;
};
std::atomic<Custom*> g_custom[STARKHIP_AIR_CUSTOM_CAPACITY];
std::mutex g_custom_mu;
int g_custom_count = 0;                            // under g_custom_mu
struct BlobLess {
    bool operator()(const std::vector<uint64_t>* a, const std::vector<uint64_t>* b) const { return *a < *b; }
};
std::map<const std::vector<uint64_t>*, int, BlobLess> g_custom_ids;  // registered key (the entry's own copy: AirInfo::key) -> id, under g_custom_mu
}  // namespace

int air_register(AirProgram&& prog, const std::vector<uint64_t>& blob, const char* name, uint32_t default_rows, int* id,
                 const std::vector<starkhip_lookup_t>& lookups) {
    std::vector<uint64_t> key = {blob.size()};  // the length first: a blob followed by a list is no other blob
    key.insert(key.end(), blob.begin(), blob.end());
    for (const starkhip_lookup_t& lk : lookups) {
        key.push_back((uint64_t)lk.input | ((uint64_t)lk.table << 32));
        key.push_back((uint64_t)lk.permuted_input | ((uint64_t)lk.permuted_table << 32));
    }
    std::lock_guard<std::mutex> g(g_custom_mu);
    auto it = g_custom_ids.find(&key);
    if (it != g_custom_ids.end()) {
        *id = it->second;
        return STARKHIP_OK;
    }
    if (g_custom_count >= STARKHIP_AIR_CUSTOM_CAPACITY) return STARKHIP_ERR_BAD_AIR;
    const int new_id = STARKHIP_AIR_CUSTOM_BASE + g_custom_count;
    std::unique_ptr<Custom> c(new Custom());
    c->name = name ? std::string(name) : "CustomAir" + std::to_string(new_id);
    c->info.prog = std::move(prog);
    c->info.id = new_id;
    c->info.name = c->name.c_str();
    c->info.cols = c->info.prog.n_cols;
    c->info.pis = c->info.prog.n_pis;
    c->info.degree = c->info.prog.degree;
    c->info.default_rows = default_rows;
    c->info.blob = blob;
    c->info.lookups = lookups;
    c->info.key = std::move(key);
    g_custom_ids.emplace(&c->info.key, new_id);
    g_custom[g_custom_count++].store(c.release(), std::memory_order_release);  // lives as long as the process
    *id = new_id;
    return STARKHIP_OK;
}

const AirInfo* air_get(int id) {
    if (id >= STARKHIP_AIR_CUSTOM_BASE && id < STARKHIP_AIR_CUSTOM_BASE + STARKHIP_AIR_CUSTOM_CAPACITY) {
        const Custom* c = g_custom[id - STARKHIP_AIR_CUSTOM_BASE].load(std::memory_order_acquire);
        return c ? &c->info : nullptr;
    }
    for (auto& s : g_slots) {
        if (s.id != id) continue;
        std::call_once(s.once, [&s]() {
            try {
                s.info.prog = s.build();
                s.info.id = s.id;
                s.info.name = s.name;
                s.info.cols = s.info.prog.n_cols;
                s.info.pis = s.info.prog.n_pis;
                s.info.degree = s.info.prog.degree;
                s.info.default_rows = s.default_rows;
                s.info.blob = s.info.prog.serialize();
                s.ok = s.info.prog.n_constraints > 0;
            } catch (const std::exception& e) {
                fprintf(stderr, "starkhip: building AIR %s failed: %s\n", s.name, e.what());
                s.ok = false;
            }
        });
        return s.ok ? &s.info : nullptr;
    }
    return nullptr;
}

}  // namespace starkhip

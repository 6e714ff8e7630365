// Internal interface between the C ABI (capi.cpp) and the GPU prover driver: the context (ctx.hip), the proof (prover.hip), the trace checkers
// (check_trace.hip), the check of the permutation pairs (permutation_check.hip), the fill of a lookup's permuted columns (lookup_columns.hip)
// and the kernel-level entries of the tests (kernel_entries.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "airs.h"
#include "trace_input.h"

namespace starkhip {

struct Ctx;
int ctx_create(int device, Ctx** out, int priority = 0);
void ctx_destroy(Ctx* c);
const float* ctx_timings(Ctx* c);
const float* ctx_kernel_timings(Ctx* c);
const float* ctx_host_timings(Ctx* c);
void ctx_commit_info(Ctx* c, int* form, unsigned* group);  // how the last proof's trace commitment went out (HashService::Timing)
int ctx_set_option(Ctx* c, const char* name, long value);
class HashService;  // scheduler.h
void ctx_attach_hash_service(Ctx* c, HashService* hs);  // trace commitments of this context go through the pool's scheduler
bool ctx_has_hash_service(Ctx* c);
int ctx_set_urgent(Ctx* c, bool urgent);
// "check_trace" and "check_trace_list" of the context's next proofs, as a pool sets them per job; {traces checked, traces rejected} so far
void ctx_set_check_trace(Ctx* c, bool on, size_t list_cap);
// "fill_lookups" of the context's next proofs, as a pool sets it per job
void ctx_set_fill_lookups(Ctx* c, bool on);
// "fill_frequencies" likewise
void ctx_set_fill_frequencies(Ctx* c, bool on);
void ctx_set_hasher(Ctx* c, int hasher);  // the "hasher" option of the context's next proofs, as a pool sets it per job
void ctx_check_stats(Ctx* c, uint64_t out[2]);
// tables, plan, work buffers, upload staging and `proof_blobs` page-locked proof blobs (blob_arena.h) for proofs of `air`,
// allocated now (a pool's warm-up)
int ctx_reserve(Ctx* c, const AirInfo& air, const starkhip_config_t& cfg, size_t log_bytes, unsigned proof_blobs = 0, bool device_traces = false);
void ctx_hash_request_reset(Ctx* c);
bool ctx_hash_requested(Ctx* c);  // the current / last prove() reached its trace commitment

struct Pool;
int pool_create(const starkhip_pool_config_t& cfg, Pool** out, unsigned cpu_share = 1);  // cpu_share: pools that split this process's CPUs
void pool_destroy(Pool* p);
int pool_submit(Pool* p, int air, const starkhip_config_t* cfg, const TraceInput& in, const uint64_t* pis, size_t n_pis, uint64_t pow, uint64_t* ticket);
int pool_submit_witness(Pool* p, int air, const starkhip_config_t* cfg, const uint32_t* operands, size_t n_limbs, uint64_t pow, uint64_t* ticket);
int pool_wait(Pool* p, uint64_t ticket, uint64_t** proof, size_t* words, starkhip_ticket_info_t* info);
int pool_stats(Pool* p, starkhip_pool_stats_t* out);
int pool_reservation(Pool* p, starkhip_pool_reservation_t* out);
int pool_host_info(Pool* p, starkhip_pool_host_info_t* out);
int pool_set_option(Pool* p, const char* name, long value);
int pool_submit_verify(Pool* p, int air, const starkhip_config_t* cfg, const uint64_t* proof, size_t words, uint64_t* ticket);
int pool_verify_stats(Pool* p, starkhip_pool_verify_stats_t* out);
int pool_check_stats(Pool* p, uint64_t out[2]);
double air_verify_cost(int air);
unsigned cpu_budget();  // multipool.cpp: CPUs this process may really use
void host_cpu_seconds(double out[3]);
// a pool per device behind one handle (multipool.cpp): placement by outstanding cost, longest job first
struct MultiPool;
double air_cost(int air);
int multipool_create(const int* devices, size_t n, const starkhip_pool_config_t& cfg, MultiPool** out);
void multipool_destroy(MultiPool* mp);
size_t multipool_size(const MultiPool* mp);
Pool* multipool_pool(MultiPool* mp, size_t slot);
int multipool_device(const MultiPool* mp, size_t slot);
int multipool_submit(MultiPool* mp, int slot, int air, const starkhip_config_t* cfg, const TraceInput& in, const uint64_t* pis, size_t n_pis, uint64_t pow,
                     uint64_t* ticket);
int multipool_submit_witness(MultiPool* mp, int slot, int air, const starkhip_config_t* cfg, const uint32_t* operands, size_t n_limbs, uint64_t pow,
                             uint64_t* ticket);
int multipool_submit_witness_batch(MultiPool* mp, size_t n, const int* airs, const uint32_t* const* operands, const size_t* n_limbs, uint64_t pow,
                                   uint64_t* tickets, int* rcs);
int multipool_ticket_slot(const MultiPool* mp, uint64_t ticket);
int multipool_wait(MultiPool* mp, uint64_t ticket, uint64_t** proof, size_t* words, starkhip_ticket_info_t* info);
int multipool_set_option(MultiPool* mp, const char* name, long value);
int multipool_submit_verify(MultiPool* mp, int slot, int air, const starkhip_config_t* cfg, const uint64_t* proof, size_t words, uint64_t* ticket);
int multipool_verify_batch(MultiPool* mp, size_t n, const int* airs, const starkhip_config_t* cfgs, const uint64_t* const* proofs, const size_t* words,
                           int* results);
void plan_verify(size_t n, const int* airs, size_t n_pools, int* slots, size_t* order);
void plan_lpt(size_t n, const int* airs, size_t n_pools, int* slots);
size_t ctx_device_bytes(Ctx* c);  // device memory this context holds (work buffers, tables, plans)
size_t ctx_pinned_bytes(Ctx* c);  // page-locked host memory it holds (upload staging; proof blobs are counted by starkhip_proof_blob_stats)

int prove(Ctx* c, const AirInfo& air, const starkhip_config_t& cfg, const TraceInput& in, const uint64_t* pis, size_t n_pis, uint64_t pow_witness,
          uint64_t** proof_out, size_t* proof_words);
// prove() in two halves over one job (prover.hip): upload .. trace_merkle, then quotient .. queries.  prove() is the two back to back with
// no endpoints and no initial challenger.  A system of tables (system.cpp; COMPAT.md 2d) runs every table's first half, reads the trace
// caps, replays the system transcript, has every table compute its CTL polynomials and sums under the system's challenges, checks the
// balances and runs every second half from a copy of the system's challenger.  A job that is not taken through its second half is
// freed with prove_job_free; the first half hands out no job when it fails (a refused trace: its check blob in *proof_out).
struct CtlTable;    // ctl.h
struct Challenger;  // poseidon.h
struct ProveJob;
int prove_first_half(Ctx* c, const AirInfo& air, const starkhip_config_t& cfg, const TraceInput& in, const uint64_t* pis, size_t n_pis, uint64_t pow_witness,
                     const CtlTable* ctl, ProveJob** job_out, uint64_t** proof_out, size_t* proof_words);
int prove_trace_cap(ProveJob* job, const uint64_t** cap, size_t* words);
int prove_job_hasher(ProveJob* job);  // the hasher its transcript and commitments run under (STARKHIP_HASHER_*)
int prove_ctl_polys(ProveJob* job, const uint64_t challenges[4], uint64_t* sums, uint64_t* zero_denominators);  // sums [2 E], zero denominators per endpoint [E]
int prove_second_half(ProveJob* job, const Challenger* initial, uint64_t** proof_out, size_t* proof_words);
void prove_job_free(ProveJob* job);
// starkhip_ctl_polys: the CTL polynomials of one table of a system on one trace, through the kernels the system prover uses (kernels_ctl.hip);
// challenges {beta_0, gamma_0, beta_1, gamma_1}, polys_out [4 E][n_rows], sums_out [2 E], the count of zero denominators
int ctl_polys(Ctx* c, const CtlTable& table, const TraceInput& in, const uint64_t* challenges, uint64_t* polys_out, uint64_t* sums_out, uint64_t* zero_denominators_out);
// starkhip_check_trace: every constraint of `air` on every row of the trace, on the device (kernels_check.hip)
int check_trace(Ctx* c, const AirInfo& air, const TraceInput& in, const uint64_t* pis, uint64_t* violations, uint64_t first[3]);
// starkhip_check_trace_report: the same check with per-constraint counts, the rows and a list (kernels_check.hip, check_report.h)
int check_trace_report(Ctx* c, const AirInfo& air, const TraceInput& in, const uint64_t* pis, uint32_t* per_constraint, uint64_t* row_mask,
                       uint64_t* list, size_t cap, starkhip_check_report_t* out);
// starkhip_check_trace_free_cells: the cells no constraint notices when delta is added to them -- the caught plane of the classes
// below, complemented (kernels_free_classes.hip, free_cells.h)
int check_trace_free_cells(Ctx* c, const AirInfo& air, const TraceInput& in, const uint64_t* pis, uint64_t delta, uint32_t* per_column,
                           uint64_t* free_mask, starkhip_free_cells_t* out);
// starkhip_check_trace_free_cell_classes: those cells as unread, gated off or silent, and the rows each constraint's gates were open on
// (kernels_free_classes.hip, free_cells.h)
int check_trace_free_cell_classes(Ctx* c, const AirInfo& air, const TraceInput& in, const uint64_t* pis, uint64_t delta, uint32_t* per_column,
                                  uint64_t* planes, uint32_t* open_rows, starkhip_free_cell_classes_t* out);
// starkhip_check_trace_permutations: which rows of each permutation pair have no partner on the other side (permutation_check.hip over
// kernels_multiset.hip, permutation_check.h); perm_check_timings: the last call's {upload, sort, classify, read-back} milliseconds
int check_trace_permutations(Ctx* c, const AirInfo& air, const TraceInput& in, uint64_t seed, uint32_t* per_pair, uint64_t* masks, uint64_t* list,
                             size_t cap, starkhip_perm_check_t* out);
void perm_check_timings(Ctx* c, float ms[4]);
// starkhip_lookup_columns: the permuted columns of each lookup written into the caller's trace -- `words`, the memory `in` views (lookup_columns.hip
// over kernels_multiset.hip and kernels_lookup.hip, lookup_columns.h); lookup_timings: the last call's {upload or gather, sort, place, read-back} milliseconds
int lookup_columns(Ctx* c, const TraceInput& in, uint64_t* words, const starkhip_lookup_t* lookups, size_t n_lookups, uint32_t* per_lookup, uint64_t* masks,
                   uint64_t* list, size_t cap, starkhip_lookup_report_t* out);
void lookup_timings(Ctx* c, float ms[4]);
// starkhip_logup_frequencies: the frequencies column of each LogUp lookup of `air` written into the caller's trace -- `words`, the memory
// `in` views (logup_frequencies.hip over kernels_multiset.hip and kernels_logup_freq.hip, logup_frequencies.h);
// logup_frequency_timings: the last call's {upload, table sort, count, write, read-back} milliseconds
int logup_frequencies(Ctx* c, const AirInfo& air, const TraceInput& in, uint64_t* words, uint32_t* per_lookup, uint32_t* per_column, uint64_t* masks, uint64_t* list,
                      size_t cap, starkhip_logup_report_t* out);
void logup_frequency_timings(Ctx* c, float ms[5]);
int ntt_long(Ctx* c, uint64_t* data, size_t n_vecs, unsigned log_len, int inverse);
int lde_batch(Ctx* c, const uint64_t* values, size_t n_cols, unsigned log_n, unsigned rate_bits, uint64_t* coeffs_out, uint64_t* lde_out);
int merkle_cap(Ctx* c, const uint64_t* lde_natural, size_t n_cols, unsigned log_N, unsigned cap_h, uint64_t* cap_out);
int permute_batch(Ctx* c, uint64_t* states, size_t n);
int keccak_permute_batch(Ctx* c, uint64_t* states, size_t n);
// Merkle tree of an LDE given column-major in natural order under `hasher`: leaf digests in tree order (may be NULL) and the cap
int merkle_tree_hasher(Ctx* c, int hasher, const uint64_t* lde_natural, size_t n_cols, unsigned log_N, unsigned cap_h, uint64_t* digests_out, uint64_t* cap_out);
// digests of n_leaves row-major leaves of `width` words under `hasher`
int hash_rows_hasher(Ctx* c, int hasher, const uint64_t* rows, size_t width, size_t n_leaves, uint64_t* digests_out);
int permute_batch_form(Ctx* c, int form, int variant, uint64_t* states, size_t n);
int leaf_hash_lane_group(Ctx* c, const uint64_t* mats, size_t n_segments, size_t n_cols, unsigned log_n, unsigned rate_bits, int grouped, int form,
                         unsigned prefix_mask, uint64_t* digests_out);
// the leaf hash's saved capacity past an identity prefix, cap[4][N], as the context builds it for this shape (kernel-level test entry)
int leaf_prefix_table(Ctx* c, unsigned log_n, unsigned rate_bits, uint64_t* cap_out);
int expand_log(Ctx* c, const TraceLog* log, uint64_t* out_colmajor);
int lde_bench(Ctx* c, size_t n_cols, unsigned log_n, unsigned rate_bits, unsigned reps, unsigned const_per_64, const uint64_t* device_values, float* ms_out, float* each_ms = nullptr);
int field_ops(Ctx* c, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
// starkhip_permutation_zs: the Z polynomials of an AIR with permutation pairs on one trace, through the kernels prove() uses
// (kernels_permutation.hip); challenges B x 2 x {beta, gamma}, zs_out [nZ][n_rows], closing_out [nZ]
int permutation_zs(Ctx* c, const AirInfo& air, const TraceInput& in, const uint64_t* challenges, uint64_t* zs_out, uint64_t* closing_out);
// starkhip_logup_polys: the auxiliary polynomials of an AIR with LogUp lookups on one trace, through the kernels prove() uses
// (kernels_logup.hip); challenges {chi_0, chi_1}, polys_out [nA][n_rows], closing_out [2][n_lookups], the count of zero denominators
int logup_polys(Ctx* c, const AirInfo& air, const TraceInput& in, const uint64_t* challenges, uint64_t* polys_out, uint64_t* closing_out, uint64_t* zero_denominators_out);
int host_alloc(Ctx* c, size_t bytes, void** out);
void host_free(void* p);

int verify_proof(const AirInfo& air, const starkhip_config_t& cfg, const uint64_t* proof, size_t words);

}  // namespace starkhip

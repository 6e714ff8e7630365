// Launchers of the gfx950 kernels (definitions in kernels_*.hip).  All launches are asynchronous on `st`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gl.h"
#include "poseidon_tables.h"  // the host-built tables of the leaf-hash forms and their CPU checks

// First statement of every kernel except the lane-form leaf hash: its waves raise their issue priority (s_setprio 2).  A lane-form group
// of four saturates the SIMDs' issue slots for a third of a second; whatever else is resident beside it in that time -- the LDE and the
// quotient of the proofs that are not in the group, Merkle levels, openings, the small AIRs' commitments -- would get the slots the
// arbiter's round robin leaves them and crawl (an LDE measured 255 ms in flight against 17 alone).  At a raised priority those waves
// issue first and the hash waves take every other slot: the same work, but the proofs outside the group reach THEIR commitment sooner
// and the next group is ready when this one ends.  Measured on 16 hardware queues, 48 proofs from operands: 7.02 - 7.08 proofs/s without,
// 7.57 - 7.58 with (profiles/r04_ab_experiments.txt 19; on HIP's default of four queues, where bench.py ran until the end of round 4,
// the same build measured 5.79 against 5.90: kernels of different proofs waited behind each other in shared queues anyway).
// -DSTARKHIP_NO_PRIO builds without it.
#ifndef STARKHIP_NO_PRIO
#define STARKHIP_PRIO_ENTRY __builtin_amdgcn_s_setprio(2);
#else
#define STARKHIP_PRIO_ENTRY
#endif

namespace starkhip {
struct QOp;  // quotient_ops.h
struct QTRec;  // quotient_plan.h
struct QTStream;
struct QTContrib;
struct VQProof;  // verify_query.h
struct VQLeaf;
}

namespace starkhip {

// workgroups of `bs` lanes that cover n items, one lane each: what the launchers size a grid with
inline unsigned nb(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

// kernels_ntt.hip
hipError_t launch_fill_powers(gl_t* out, gl_t base, gl_t mult, size_t count, hipStream_t st);  // out[i] = base * mult^i
hipError_t launch_fill_coset_scale(gl_t* out, unsigned log_n, unsigned rate_bits, hipStream_t st);
hipError_t launch_transpose(const gl_t* in, gl_t* out, size_t rows, size_t cols, hipStream_t st);
// compact trace log (trace_log.h) -> column-major values[col][row]; `values` must be zeroed
hipError_t launch_expand_trace(const uint32_t* words, const uint32_t* offsets, size_t n_records, gl_t* values, size_t n_rows, hipStream_t st);
hipError_t launch_zero_cells(const uint32_t* col_row, size_t n_cells, gl_t* values, size_t n_rows, hipStream_t st);
// from_coeffs == 0: `values` holds evaluations on the subgroup (PolynomialBatch::from_values);
// from_coeffs != 0: `values` already holds coefficients (PolynomialBatch::from_coeffs), coeffs_out unused.
// 2^1 .. 2^7 rows (radix-2 in LDS, kernels_ntt.hip)
hipError_t launch_lde_columns(const gl_t* values, gl_t* coeffs, gl_t* lde, size_t n_cols, unsigned log_n, unsigned rate_bits,
                              const gl_t* tw_fwd, const gl_t* tw_inv, unsigned tw_log, const gl_t* coset_scale, int from_coeffs,
                              hipStream_t st);
// 2^8 .. 2^13 rows (register radix-16 Stockham passes, kernels_lde.hip) with its own host-built tables
bool lde_v2_supported(unsigned log_n);
size_t lde_v2_tw_words(unsigned log_n);
size_t lde_v2_oh_words(unsigned log_n, unsigned rate_bits);  // closed-form tables of unit-vector columns (0: shape without them)
hipError_t lde_v2_upload_tables(unsigned log_n, unsigned rate_bits, gl_t* d_tw_fwd, gl_t* d_tw_inv, gl_t* d_cs, gl_t* d_oh, hipStream_t st);
// col_base / unit_count (both LDE kernels with closed forms, 2^12 and 2^13 rows; null: nothing is counted): the absolute index of the launch's
// first column in its trace and a device word that gains 1 for every column c < n found to be the unit vector e_c -- see LeafPrefix below
hipError_t launch_lde_columns_v2(const gl_t* values, gl_t* coeffs, gl_t* lde, size_t n_cols, unsigned log_n, unsigned rate_bits,
                                 const gl_t* tw_fwd, const gl_t* tw_inv, const gl_t* cs, const gl_t* oh, int from_coeffs, hipStream_t st,
                                 unsigned col_base = 0, unsigned* unit_count = nullptr);
// 2^13 rows, values -> LDE only (no coefficient output): the wave-resident kernel (kernels_lde.hip; tools/lde_wave_model.py)
bool lde_wave_supported(unsigned log_n);
size_t lde_wave_table_words(unsigned rate_bits);
hipError_t lde_wave_upload_tables(unsigned rate_bits, gl_t* d_tab, hipStream_t st);
hipError_t launch_lde_columns_wave(const gl_t* values, gl_t* lde, size_t n_cols, unsigned rate_bits, const gl_t* d_tab, const gl_t* oh, unsigned* next,
                                   hipStream_t st, unsigned col_base = 0, unsigned* unit_count = nullptr);
// 2^14 .. 2^26 points, a vector split over workgroups in two passes (kernels_lde_long.hip; tools/lde_long_model.py).  `sub`: the
// sub-transforms' twiddles (lde_long_sub_words() words, the same for every length; the inverse ones carry the inverse's n^-1);
// tw_fwd / tw_inv: the inter-pass twiddles w_n^(+-j0 k1) of ONE length (2^log_n words each, lde_long_fill_twiddles).
bool lde_long_supported(unsigned log_n);
size_t lde_long_sub_words();
hipError_t lde_long_upload_sub_tables(gl_t* d_sub, hipStream_t st);
hipError_t lde_long_fill_twiddles(gl_t* d_fwd, gl_t* d_inv, unsigned log_n, hipStream_t st);
struct LdeLongTables {
    const gl_t *sub, *tw_fwd, *tw_inv;
};
// values -> coeffs -> lde (coset-major); `coeffs` is required unless from_coeffs (it is the transforms' scratch too; may be `values`);
// cs[s][j] = (7 w_N^s)^j, N words
hipError_t launch_lde_columns_long(const gl_t* values, gl_t* coeffs, gl_t* lde, size_t n_cols, unsigned log_n, unsigned rate_bits, const LdeLongTables& tb,
                                   const gl_t* cs, int from_coeffs, hipStream_t st);
// n_vecs vectors, vec_stride words apart in src, mid and dst alike: src (* pre_scale) -> mid -> dst (* post_scale); the inverse carries
// n^-1.  mid must not overlap src; dst may be mid or src.
hipError_t launch_ntt_long(const gl_t* src, gl_t* mid, gl_t* dst, size_t n_vecs, size_t vec_stride, unsigned log_n, bool inverse, const gl_t* pre_scale,
                           const gl_t* post_scale, const LdeLongTables& tb, hipStream_t st);
// one workgroup per vector: the short vectors of a proof (up to 2^15 words), and those beyond 2^26
hipError_t launch_ntt_global(gl_t* data, size_t n_vecs, size_t vec_stride, unsigned log_n, const gl_t* tw, unsigned tw_log,
                             const gl_t* pre_scale, const gl_t* post_scale, gl_t final_mul, hipStream_t st);

// kernels_hash.hip
// up to LEAF_HASH_MAX_BATCH matrices of one shape hashed by one launch (the trace commitments of proofs of the same AIR)
static const unsigned LEAF_HASH_MAX_BATCH = 64;
// The saved sponge state past a fixed identity prefix (lane and pair forms; the other forms and the Keccak hasher ignore it).  Where the
// first n columns of an n-row trace are the unit vectors e_0 .. e_{n-1} -- FinalExp's one-hot row selectors, which its constraints force --
// their LDE is the closed form of kernels_lde.hip: column c at point (s, k) is e0[s][(k - c) mod n], a table of the shape alone.  n columns
// are n / 8 whole blocks of the rate-8 sponge and the next block, a full one, overwrites the whole rate: the state of leaf q = s n + k after
// them is its four capacity words, cap[w][q] (struct of arrays: a wave reads 512-byte runs), the same for every such trace.  `count` is the
// proof's own evidence that it has such a trace: the LDE kernels add 1 to it for every column c < n they find to be e_c (each column is
// transformed once per proof), so *count == n exactly when the prefix is the identity.  A kernel given both starts its leaves from `cap`
// at block n / 8 when *count == n and n_cols >= n + 8, and hashes every block otherwise.  Null pointers: never skip.
struct LeafPrefix {
    const unsigned* count = nullptr;
    const gl_t* cap = nullptr;  // [4][N]
};
size_t leaf_prefix_words(unsigned log_n, unsigned rate_bits);  // 4 N, or 0 for a shape whose LDE kernels have no closed forms
// cap[4][N] from the LDE-of-e_0 half of the closed-form table `oh` (lde_v2_upload_tables): one lane per leaf, n / 8 permutations each
hipError_t launch_leaf_prefix_build(const gl_t* oh, unsigned log_n, unsigned rate_bits, gl_t* cap, hipStream_t st);
struct LeafHashBatch {
    const gl_t* mat[LEAF_HASH_MAX_BATCH];
    gl_t* digests[LEAF_HASH_MAX_BATCH];
    const unsigned* prefix_count[LEAF_HASH_MAX_BATCH];  // LeafPrefix per member (lane form; null: that member never skips)
    const gl_t* prefix_cap[LEAF_HASH_MAX_BATCH];
};
hipError_t launch_leaf_hash_multi(const LeafHashBatch& B, unsigned count, size_t n_cols, unsigned log_n, unsigned rate_bits, hipStream_t st);
// the same in the lane form (one lane per leaf): the big commitments of a pool's lane group as ONE grid, grid.y = commitment
hipError_t launch_leaf_hash_lane_group(const LeafHashBatch& B, unsigned count, size_t n_cols, unsigned log_n, unsigned rate_bits, hipStream_t st);
// The leaf-hash forms in the numbering of the "leaf_hash_form" option and of the test entries (starkhip_poseidon_permute_batch_form,
// starkhip_hash_table_image).  FORM_AUTO: the option's "the library picks"; as a permutation entry, the generic loop.
enum LeafHashForm : int {
    FORM_AUTO = 0,
    FORM_QUAD = 1,  // four lanes per leaf
    FORM_ROW = 2,   // 16 lanes per leaf: shorter chain per leaf, 4x the lane-instructions -- for a lone commitment of few leaves
    FORM_LANE = 3,  // one lane per leaf: fewest instructions per permutation, but 1/4 of the waves -- for big commitments when several are in flight
    FORM_PAIR = 4,  // two lanes per leaf, one 256-register wave per SIMD at 32 768 leaves: a LONE big commitment
};
// How a trace commitment went out, as starkhip_ticket_info_t.leaf_hash_form reports it (starkhip.h: public values)
enum LeafHashSent : int {
    SENT_QUAD = 0,
    SENT_ROW = 1,
    SENT_MERGED = 2,  // one grid merged with other proofs' commitments (quad form)
    SENT_LANE = 3,
    SENT_HOST = 4,    // hashed by host threads
    SENT_PAIR = 5,
    SENT_KECCAK = 6,  // the Keccak hasher's leaf hash (kernels_keccak.hip), always the context's own launch
};
// what a lone launch of `form` (not FORM_AUTO) is reported as
inline LeafHashSent leaf_hash_sent(LeafHashForm form) {
    return form == FORM_ROW ? SENT_ROW : form == FORM_LANE ? SENT_LANE : form == FORM_PAIR ? SENT_PAIR : SENT_QUAD;
}
// the same digests from every form; hipErrorInvalidValue for FORM_AUTO
hipError_t launch_leaf_hash_form(LeafHashForm form, const gl_t* mat, size_t n_cols, unsigned log_n, unsigned rate_bits, gl_t* digests, hipStream_t st,
                                 LeafPrefix prefix = LeafPrefix());
// Copies a host-built table (poseidon_tables.h) to its __constant__ symbol once per device, under a lock.  `done`: the symbol's own
// flags, one per device, set after a successful copy.  hipErrorInvalidDevice for a device index outside 0 .. 63, hipErrorInvalidValue
// for an image that could not be built (null).
hipError_t upload_table_once(const void* symbol, const void* image, size_t bytes, bool (&done)[64]);
hipError_t launch_leaf_hash_rows(const gl_t* rows, size_t width, size_t n_leaves, gl_t* digests, hipStream_t st);
hipError_t launch_merkle_levels(gl_t* digests, unsigned log_leaves, unsigned cap_h, hipStream_t st);
hipError_t launch_permute_batch(gl_t* states, size_t n, hipStream_t st);
// how many variants of its permutation a form's leaf kernel uses (0: no such form); kernels_hash.hip, the test entry points
inline unsigned permute_form_variants(int form) {
    switch (form) {
        case FORM_AUTO: case FORM_ROW: return 1u;
        case FORM_QUAD: case FORM_LANE: case FORM_PAIR: return 2u;
    }
    return 0u;
}
hipError_t launch_permute_quad_form(bool cap_only, const gl_t* in, gl_t* out, size_t n, hipStream_t st);   // kernels_hash_quad_form.hip
// variant 1 = the form's capacity-only last round (quad, lane, pair)
hipError_t launch_permute_batch_form(int form, int variant, const gl_t* in, gl_t* out, size_t n, hipStream_t st);
hipError_t launch_pow_grind(const gl_t* base_state, int pos, unsigned pow_bits, uint64_t start, uint64_t count, unsigned long long* best,
                            hipStream_t st);
// kernels_keccak.hip: the Keccak hasher's counterparts of the launches above (keccak.h) -- one lane per hash, the same digest slots
hipError_t launch_leaf_hash_keccak(const gl_t* mat, size_t n_cols, unsigned log_n, unsigned rate_bits, gl_t* digests, hipStream_t st);
hipError_t launch_leaf_hash_rows_keccak(const gl_t* rows, size_t width, size_t n_leaves, gl_t* digests, hipStream_t st);
hipError_t launch_merkle_levels_keccak(gl_t* digests, unsigned log_leaves, unsigned cap_h, hipStream_t st);
hipError_t launch_permute_batch_keccak(gl_t* states, size_t n, hipStream_t st);
hipError_t launch_pow_grind_keccak(const gl_t* base_state, int pos, unsigned pow_bits, uint64_t start, uint64_t count, unsigned long long* best,
                                   hipStream_t st);
// by hasher id (starkhip.h: 0 Poseidon, 1 Keccak), where a proof's phases pick
inline hipError_t launch_leaf_hash_rows_by(int hasher, const gl_t* rows, size_t width, size_t n_leaves, gl_t* digests, hipStream_t st) {
    return hasher ? launch_leaf_hash_rows_keccak(rows, width, n_leaves, digests, st) : launch_leaf_hash_rows(rows, width, n_leaves, digests, st);
}
inline hipError_t launch_merkle_levels_by(int hasher, gl_t* digests, unsigned log_leaves, unsigned cap_h, hipStream_t st) {
    return hasher ? launch_merkle_levels_keccak(digests, log_leaves, cap_h, st) : launch_merkle_levels(digests, log_leaves, cap_h, st);
}
// kernels_selftest.hip
hipError_t launch_field_ops(int op, const gl_t* a, const gl_t* b, gl_t* out, size_t n, hipStream_t st);

// kernels_quotient.hip
hipError_t launch_quotient_tables(gl_t* tab, unsigned log_n, unsigned qdb, hipStream_t st);
hipError_t launch_quotient_eval(const QOp* ops, const uint32_t* loads, unsigned n_slots, const uint32_t* chunk_batch, unsigned n_chunks,
                                const gl_t* pis, const gl_t* lde, const gl_t* tab, const gl_t* apow, gl_t alpha0, gl_t alpha1, gl_t* partial,
                                unsigned log_n, unsigned rate_bits, unsigned qdb, hipStream_t st);
hipError_t launch_quotient_combine(const gl_t* partial, const gl_t* chunk_scale, unsigned n_chunks, const gl_t* tab, unsigned log_n,
                                   unsigned qdb, gl_t* out, hipStream_t st);

// tiled evaluator (quotient_plan.h): per-proof record weights, the LDS-tiled pass, the sum over chunks / Z_H
hipError_t launch_quotient_weights(QTRec* recs, const uint32_t* contrib_off, const QTContrib* contribs, uint32_t n_recs, gl_t* apow, uint32_t K,
                                   const gl_t* consts, const gl_t* pis, gl_t alpha0, gl_t alpha1, hipStream_t st);
hipError_t launch_quotient_tiles(const QTRec* recs, const QTStream* streams, const uint32_t* chunk_tile_off,
                                 const uint32_t* tile_list, unsigned n_chunks, const gl_t* lde, const gl_t* tab, gl_t* partial, unsigned log_n,
                                 unsigned rate_bits, unsigned qdb, unsigned n_cols, unsigned dbg, hipStream_t st, const uint32_t* work = nullptr,
                                 unsigned n_work = 0, unsigned n_accs = 1);
// by class (QTClassPlan, "quotient_cosets" = 0): the classes' sums on their cosets / Z_H as 2 n_vecs vectors of n words, and -- after the
// inverse transform of those -- the quotient's coefficient chunks [2][n << qdb] (kernels_quotient.hip)
hipError_t launch_quotient_class_sums(const gl_t* partial, const uint32_t* sum_off, const uint32_t* vec_slot, unsigned n_vecs, unsigned n_slots,
                                      const gl_t* tab, unsigned log_n, unsigned qdb, gl_t* out, hipStream_t st);
hipError_t launch_quotient_class_solve(const gl_t* a, const uint32_t* vec_of, unsigned n_classes, const gl_t* solve, unsigned log_n, unsigned qdb,
                                       gl_t* out, hipStream_t st);
hipError_t launch_quotient_tiles_combine(const gl_t* partial, unsigned n_chunks, const gl_t* tab, unsigned log_n, unsigned qdb, gl_t* out,
                                         hipStream_t st);

// kernels_check.hip: the trace checkers' kernels (starkhip_check_trace, starkhip_check_trace_report).  What all three read: the op
// stream of compile_quotient_ops cut into chunks, and a column-major trace [C][2^log_n] with its public inputs.
struct CheckView {  // the four pointers the op loop reads come first: one fetch of kernel arguments brings them
    const QOp* ops;
    const uint32_t* chunk_op;  // [n_chunks + 1] first op of each chunk
    const gl_t* trace;         // column-major [C][2^log_n]
    const gl_t* pis;
    const uint32_t* chunk_k0;  // [n_chunks] index of each chunk's first constraint
    unsigned n_chunks, log_n;
};
// Every constraint on every row: out[0] += violations, out[1] = min(out[1], (k << 32) | row); the caller presets them to 0 and ~0.
hipError_t launch_check_trace(const CheckView& v, unsigned long long* out, hipStream_t st);
// The report's two passes.  Count: counts[k] += rows on which constraint k is violated, row_mask[r >> 6] |= 1 << (r & 63) for every
// row with a violation; both preset to 0.  List: over chunks[0 .. n_launched), the violations of the constraints with base[k] != ~0
// as {k, row, value} at list[base[k] + (a slot from cursors[k], preset to 0)]; slots at or past list_len are not written.
hipError_t launch_check_report_count(const CheckView& v, uint32_t* counts, unsigned long long* row_mask, hipStream_t st);
hipError_t launch_check_report_list(const CheckView& v, const uint32_t* chunks, unsigned n_launched, uint32_t* cursors, const unsigned long long* row_mask,
                                    const uint32_t* base, unsigned long long* list, uint32_t list_len, hipStream_t st);

// kernels_free_classes.hip: the free-cell kernel (starkhip_check_trace_free_cell_classes, and starkhip_check_trace_free_cells as its
// caught plane) over the same view; `cons` and `pivots` are compile_free_cells' (free_cells.h).  planes [3][C][(n + 63) / 64] -- read,
// open, caught; plane_words = C x (n + 63) / 64 -- and open_rows [K] are zeroed by the caller and only gain bits and counts: a cell's
// caught bit is set when some constraint notices delta added to it.  The count leaves the planes as they are and sets
// per_column[c][0 .. 2] to the column's silent, gated and unread rows.
struct FreeCon;
hipError_t launch_free_cell_classes(const CheckView& v, const FreeCon* cons, const uint32_t* pivots, uint32_t n_constraints, gl_t delta,
                                    unsigned long long* planes, size_t plane_words, uint32_t* open_rows, hipStream_t st);
hipError_t launch_free_cell_classes_count(const unsigned long long* planes, size_t plane_words, uint32_t n_cols, unsigned log_n,
                                          uint32_t* per_column, hipStream_t st);

// kernels_fri.hip
hipError_t launch_ext_powers(gl2_t* out, gl2_t base, size_t count, hipStream_t st);
// weights of the evaluation at z (and, rotated by one, at w_n z) from values on coset 0 of the LDE; scale = (z^n - 7^n) / (n 7^n)
hipError_t launch_coset_weights(gl2_t* wz, gl2_t* wgz, gl2_t z, gl2_t scale, unsigned log_n, hipStream_t st);
// vectors of n words, `stride` words apart (coefficients: stride = n; coset 0 of an LDE: stride = 2^rate n)
hipError_t launch_openings(const gl_t* coeffs, size_t stride, size_t n_polys, size_t n, const gl2_t* zpow, const gl2_t* gzpow, gl2_t* out_z,
                           gl2_t* out_gz, hipStream_t st);
hipError_t launch_fri_combine(const gl_t* coeffs, size_t stride, size_t n_polys, size_t n, const gl2_t* apow, size_t polys_per_chunk,
                              size_t n_chunks, gl2_t* partial, hipStream_t st);
hipError_t launch_ext_reduce(const gl2_t* partial, size_t n_chunks, size_t n, gl_t* out, hipStream_t st);  // two vectors of n words
hipError_t launch_fri_leaves(const gl_t* vals, unsigned log_len, unsigned arity_bits, gl_t* rows, hipStream_t st);
hipError_t launch_fri_fold(const gl_t* in, size_t len, unsigned arity_bits, gl2_t beta, gl_t* out, hipStream_t st);

// kernels_query.hip: query-round leaves and Merkle paths written in proof-blob layout (stride = words per query round)
hipError_t launch_query_leaf_colmajor(const gl_t* mat, size_t n_cols, unsigned log_n, unsigned rate_bits, const uint32_t* xs, size_t n_queries,
                                      gl_t* out, size_t stride, size_t off, hipStream_t st);
hipError_t launch_query_leaf_rows(const gl_t* rows, size_t width, const uint32_t* xs, unsigned shift, size_t n_queries, gl_t* out, size_t stride,
                                  size_t off, hipStream_t st);
hipError_t launch_query_path(const gl_t* digests, size_t n_leaves, unsigned depth, const uint32_t* xs, unsigned shift, size_t n_queries, gl_t* out,
                             size_t stride, size_t off, hipStream_t st);

// device verifier (verifier_device.cpp): the row-form digests of opened leaves (kernels_hash.hip), then kernels_verify.hip's range check
// of the query sections (bad[p] |= 1), fri_combine_initial's sums (two per query) and the per-query checks (one status word per query)
// (hashers: bit h set when some leaf of the list belongs to a proof of hasher h; each hasher's kernel walks the list and takes its own)
hipError_t launch_verify_leaf_digests(const gl_t* words, const VQLeaf* leaves, size_t n_leaves, gl_t* digests, unsigned hashers, hipStream_t st);
hipError_t launch_verify_leaf_digests_keccak(const gl_t* words, const VQLeaf* leaves, size_t n_leaves, gl_t* digests, hipStream_t st);
hipError_t launch_verify_range(const gl_t* words, const VQProof* proofs, size_t n_proofs, uint32_t* bad, hipStream_t st);
hipError_t launch_verify_combine(const gl_t* words, const VQProof* proofs, const uint32_t* query_proof, size_t n_queries, const gl2_t* apow,
                                 gl2_t* sums, hipStream_t st);
hipError_t launch_verify_queries(const gl_t* words, const VQProof* proofs, const uint32_t* query_proof, const uint64_t* x_index, size_t n_queries,
                                 const gl_t* digests, const gl2_t* sums, uint32_t* status, hipStream_t st);

}  // namespace starkhip

/* libstarkhip -- C ABI of the MI355X-native STARK prover for the four BLS12-381 AIRs of
 * Electron-Labs/starky_bls12_381.
 *
 * Drop-in boundary: each entry point replaces one call the reference makes into the
 * (un-vendored) starky / plonky2 crates or into its own AIR modules:
 *
 *   starkhip_prove            <- starky::prover::prove::<F, C, S, D>(stark, &config, trace_poly_values,
 *                                &public_inputs, &mut timing)         src/aggregate_proof.rs:59-65,
 *                                                                     :105-111, :138-144, :169-175
 *   starkhip_verify           <- starky::verifier::verify_stark_proof src/aggregate_proof.rs:67,113,146,177
 *   starkhip_config_standard_fast <- StarkConfig::standard_fast_config()  src/aggregate_proof.rs:32,76,122,155
 *   starkhip_air_*            <- the associated consts S::COLUMNS / S::PUBLIC_INPUTS / constraint_degree()
 *                                src/fp12_mul.rs:21-27,142-144; src/final_exponentiate.rs:1362-1364 ...
 *   starkhip_trace_*          <- S::generate_trace(..) + trace_rows_to_poly_values
 *                                src/fp12_mul.rs:44-48, src/final_exponentiate.rs:240-279,
 *                                src/miller_loop.rs, src/calc_pairing_precomp.rs:150-348;
 *                                src/aggregate_proof.rs:57,104,137,168
 *   starkhip_trace_ecc_aggregate <- ECCAggStark::generate_trace + the public inputs of ec_aggregate_main
 *                                src/ecc_aggregate.rs:39-84, src/aggregate_proof.rs:181-221
 *   starkhip_native_*         <- crate::native (Fp12 mul, final_exponentiate, miller_loop,
 *                                calc_pairing_precomp)               src/native.rs:1201-1468
 *
 * Because `S: Stark` is a compile-time generic in the reference, the AIR is selected by id.
 * All field elements are canonical Goldilocks values (< 2^64 - 2^32 + 1) in little-endian
 * uint64_t -- every word the library writes, and every public input, program constant, `delta` and proof word it is given
 * (anything else there is STARKHIP_ERR_BAD_SHAPE, or a rejected proof).  The one exception is the CELLS OF A TRACE: see starkhip_prove.
 * Fp elements are 12 little-endian u32 limbs (src/fp.rs:1).
 *
 * Threading: one in-flight prove per context; different contexts (GPUs) may run concurrently.
 * Ownership: the caller owns every input for the duration of the call; buffers returned through
 * `uint64_t** out` are owned by the library until starkhip_free().
 */
#ifndef STARKHIP_H
#define STARKHIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* starky's StarkConfig with its FriConfig, flattened.  Accepted range (one rule for every prove, pool, multipool and verify entry
 * point; starkhip_fri_geometry applies it): num_challenges == 2, rate_bits <= 8 and at least log2 of the AIR's quotient degree
 * factor (degree - 1), cap_height <= 16 and <= degree_bits + rate_bits, 1 <= arity_bits <= 8, proof_of_work_bits <= 64.  The FRI
 * layers are plonky2's ConstantArityBits(arity_bits, final_poly_bits): while db > final_poly_bits && db + rate_bits - arity_bits >=
 * cap_height (over the integers) a layer of arity_bits; a config where a layer would take db below zero (plonky2's
 * assert!(degree_bits >= arity_bits)) or that needs more than 16 layers is refused.  num_query_rounds may be 0 (a proof with no
 * query rounds, as plonky2 makes it); security_bits is not read.  Anything else is STARKHIP_ERR_BAD_SHAPE before any device work. */
typedef struct {
    uint32_t security_bits;      /* 100 */
    uint32_t num_challenges;     /* 2   */
    uint32_t rate_bits;          /* 1 (2 for PairingPrecomp / FinalExp) */
    uint32_t cap_height;         /* 4   */
    uint32_t proof_of_work_bits; /* 16  */
    uint32_t arity_bits;         /* ConstantArityBits(4, 5) */
    uint32_t final_poly_bits;
    uint32_t num_query_rounds;   /* 84  */
} starkhip_config_t;

/* Ids of AIRs registered at run time (starkhip_air_register): BASE, BASE + 1, ... in registration order, never reused; at most
 * CAPACITY of them per process */
#define STARKHIP_AIR_CUSTOM_BASE 1024
#define STARKHIP_AIR_CUSTOM_CAPACITY 4096
/* Trace lengths.  A REGISTERED AIR is proved, checked and submitted to pools on any power of two of rows in 2 .. 2^STARKHIP_MAX_LOG_ROWS;
 * the built-in AIRs (STARKHIP_AIR_TEST_FIBONACCI included) keep the reference's largest trace, 8192 rows -- their layouts are the
 * reference's; a registered copy of a built-in program is how a caller proves it longer.  The bound comes from 32-bit byte offsets
 * into one LDE column in the quotient kernel (2^(20 + 8) points of 8 bytes with rate_bits <= 8).  A trace whose buffers do not fit the
 * device is STARKHIP_ERR_OOM and leaves the context usable. */
#define STARKHIP_MAX_LOG_ROWS 20
/* limits of a registered constraint program (starkhip_air_check_program); the five built-in AIRs are far inside them
 * (MillerLoop: 97 330 columns, ECCAgg: 12 824 public inputs, FinalExp: 2.4 M code words) */
#define STARKHIP_AIR_MAX_COLUMNS (1u << 20)
#define STARKHIP_AIR_MAX_PUBLIC_INPUTS 65535u /* a public-input index travels in 16 bits of a device op (quotient_ops.h) */
#define STARKHIP_AIR_MAX_CODE_WORDS (1u << 26)
#define STARKHIP_AIR_MAX_DEGREE 8u /* 4 gates + 3 factors + 1 for a first / last-row constraint: the most a program can reach */
#define STARKHIP_AIR_MAX_PERMUTATION_PAIRS 64u   /* permutation pairs of a program, and entries of one pair */
#define STARKHIP_AIR_MAX_PERMUTATION_ENTRIES 64u
#define STARKHIP_AIR_MAX_LOGUP_LOOKUPS 64u /* LogUp lookups of a program, and looked-up columns of one lookup */
#define STARKHIP_AIR_MAX_LOGUP_COLUMNS 64u
#define STARKHIP_AIR_MAX_LOGUP_POLYS 1024u /* nA: the auxiliary polynomials a proof of the program commits (header word 14) */

typedef enum {
    STARKHIP_AIR_FP12_MUL = 0,
    STARKHIP_AIR_PAIRING_PRECOMP = 1,
    STARKHIP_AIR_MILLER_LOOP = 2,
    STARKHIP_AIR_FINAL_EXP = 3,
    STARKHIP_AIR_ECC_AGGREGATE = 4, /* ECCAggStark: sum of the 512 sync-committee keys whose bit is set (src/ecc_aggregate.rs) */
    STARKHIP_AIR_TEST_FIBONACCI = 100, /* 2-column toy AIR used by the unit tests */
    /* widens the enum's range over the ids of registered AIRs (starkhip_air_register), which C++ callers cast to starkhip_air_t */
    STARKHIP_AIR_CUSTOM_LAST = (STARKHIP_AIR_CUSTOM_BASE + STARKHIP_AIR_CUSTOM_CAPACITY - 1)
} starkhip_air_t;

enum {
    STARKHIP_OK = 0,
    STARKHIP_ERR_QUOTIENT_NOT_DIVISIBLE = -1, /* "Quotient has failed, the vanishing polynomial is not divisible by Z_H" */
    STARKHIP_ERR_ZETA_IN_SUBGROUP = -2, /* the challenge zeta lies in the trace subgroup H: starky's "Opening point is in the subgroup" (probability
                                          2^-115 per proof, deterministic for the input it hits).  zeta on the coset 7 H, where the trace polynomials'
                                          values are kept, is proven as the reference proves it (the opening is then the value itself) */
    STARKHIP_ERR_BAD_SHAPE = -3,
    STARKHIP_ERR_HIP = -4,
    STARKHIP_ERR_OOM = -5,
    STARKHIP_ERR_NO_DEVICE = -6,
    STARKHIP_ERR_VERIFY = -7,
    STARKHIP_ERR_BAD_AIR = -8,
    STARKHIP_ERR_TRACE = -9 /* "check_trace" / "check_traces": the trace violates the AIR; a check blob is handed back instead of a proof */
};

#define STARKHIP_POW_SEARCH UINT64_MAX

/* The hasher of a proof -- plonky2's `C: GenericConfig`: PoseidonGoldilocksConfig (what the reference's drivers select, and the default)
 * or KeccakGoldilocksConfig (KeccakHash<25>; COMPAT.md K1 - K8).  Chosen per context ("hasher", starkhip_set_option) or per pool, and
 * carried in header word 12 of the proof, which every verify entry reads: a proof is verified under the hasher its header names, and a
 * batch may mix both.  A Keccak digest is 25 bytes; in the blob it is the four field elements plonky2's challenger observes for it
 * (the bytes in little-endian chunks of 7, 7, 7 and 4), so a digest is 4 words under either hasher, every proof word stays a canonical
 * field element and the blob layout below holds for both.  A Keccak proof with a digest word outside those ranges (2^56, the last 2^32)
 * is rejected. */
enum {
    STARKHIP_HASHER_POSEIDON = 0,
    STARKHIP_HASHER_KECCAK = 1
};

/* --- configuration ------------------------------------------------------------------- */
void starkhip_config_standard_fast(starkhip_config_t* cfg);
/* the per-AIR config the reference builds (rate_bits override for PairingPrecomp / FinalExp) */
int starkhip_config_for_air(starkhip_air_t air, starkhip_config_t* cfg);

/* --- AIR metadata -------------------------------------------------------------------- */
int starkhip_air_columns(starkhip_air_t air);
int starkhip_air_public_inputs(starkhip_air_t air);
int starkhip_air_constraint_degree(starkhip_air_t air);
int starkhip_air_num_constraints(starkhip_air_t air);
int starkhip_air_default_rows(starkhip_air_t air);
/* serialised constraint program (format: starky_bls12_381_amd/csrc/air_ir.h); library-owned */
int starkhip_air_program(starkhip_air_t air, const uint64_t** blob, size_t* words);
/* What one call of S::eval_packed_generic leaves in the ConstraintConsumer (the reference folds
 * acc_j = acc_j * alpha_j + mask(kind) * c_k constraint by constraint; e.g. src/final_exponentiate.rs:907-1136) on ONE
 * frame over the quadratic extension — the host evaluator the verifier uses.  All field arguments are (a0, a1) pairs:
 * local / next hold starkhip_air_columns() pairs, masks = {1, z_last, L_first, L_last} as the consumer applies them to
 * constraint / constraint_transition / constraint_first_row / constraint_last_row, acc_out n_alpha pairs.  public_inputs
 * are base-field.  Host only. */
int starkhip_air_eval_frame(starkhip_air_t air, const uint64_t* local, const uint64_t* next, const uint64_t* public_inputs,
                            const uint64_t masks[8], const uint64_t* alphas, int n_alpha, uint64_t* acc_out);
/* Permutation arguments (starky's Stark::permutation_pairs(); COMPAT.md P1 - P8).  A registered program may declare pairs of column
 * lists: the rows of the lhs columns are a permutation of the rows of the rhs columns.  The pairs are cut into batches of
 * B = max(1, degree - 1) in declaration order; every batch has one running-product polynomial Z per challenge (2 of them), index
 * batch * 2 + challenge, committed between the trace and the quotient.  The two queries: the number of pairs, and nZ = 2 x batches
 * (0 for an AIR without pairs, which is every built-in one); BAD_AIR for an unknown id.  A proof of an AIR with pairs always evaluates
 * its quotient on every coset ("quotient_cosets" = 1, as degree > 5 does), behind either "quotient_impl". */
int starkhip_air_permutation_pairs(starkhip_air_t air);
int starkhip_air_permutation_zs(starkhip_air_t air);
/* LogUp lookups (starky >= 0.2's Lookup { columns, table_column, frequencies_column }; COMPAT.md L1 - L7).  A registered program may
 * declare lookups instead of permutation pairs (a program with both is refused): every cell of a lookup's m columns occurs in its table
 * column, and its frequencies column holds, row by row, how often that row's table value is looked up.  With d the program's degree
 * (>= 2) the m columns are cut in declaration order into H = ceil(m / (d - 1)) helper batches.  Per challenge (2), then per lookup, a
 * proof commits the H helper polynomials and one running sum Z, between the trace and the quotient: nA = 2 sum (H + 1) polynomials
 * (at most STARKHIP_AIR_MAX_LOGUP_POLYS), and nL = 2 sum (H + 2) constraints follow the AIR's own in the alpha fold.  The two queries:
 * the number of lookups, and nA (0 for an AIR without them, which is every built-in one); BAD_AIR for an unknown id.  starkhip_prove
 * refuses a trace whose running sums do not close (wrong frequencies, a value missing from the table) or in which a denominator
 * chi + cell is zero with STARKHIP_ERR_QUOTIENT_NOT_DIVISIBLE, before the auxiliary polynomials are committed; the context stays
 * usable.  Such a proof evaluates its quotient on every coset, behind either "quotient_impl".  The frequencies column is filled by
 * starkhip_logup_frequencies, or inside prove() under "fill_frequencies" ("LogUp FREQUENCIES" below), which also says which cells
 * miss the table. */
int starkhip_air_logups(starkhip_air_t air);
int starkhip_air_logup_polys(starkhip_air_t air);
/* the looked-up columns of all LogUp lookups of the AIR together (sum m: the length of starkhip_logup_frequencies' per_column; 0 for
 * an AIR without them); BAD_AIR for an unknown id */
int starkhip_air_logup_columns(starkhip_air_t air);
/* General lookups (upstream's Column and Filter, COMPAT.md 2c): a program may declare its lookups in the section "LOGUPS02" instead of
 * "LOGUPS01" (never both; u64 words, in the same place):
 *     "LOGUPS02", n_lookups, then per lookup: n_columns, COLUMN table, COLUMN frequencies, n_columns x { COLUMN value, FILTER }
 *     COLUMN := n_local | n_next << 32, constant, then (n_local + n_next) x { trace column, coefficient }   (local terms first)
 *     FILTER := n_products | n_sums << 32, then 2 n_products + n_sums COLUMNs (each product's A then B, then the sums)
 * A COLUMN is constant + sum coefficient * cell over the local and the next row (the last row's next is row 0; at most 16 terms,
 * coefficients canonical and nonzero); a FILTER is sum A B + sum C (at most 4 products and 4 sums) and 1 when empty.  With phi_c the
 * filter of the looked-up value v_c the helpers are h_j = sum over batch j of phi_c / (chi + v_c), the running sum steps by
 * sum_j h_j - f / (chi + t); polynomials, constraints and their order are those above, and so is the proof layout: a proof of a
 * "LOGUPS02" program whose lookups are all plain (every COLUMN one local cell with coefficient 1 and constant 0, every FILTER empty)
 * is byte for byte the proof of the "LOGUPS01" program.  A zero chi + v_c counts as a zero denominator whatever its filter says.
 * starkhip_air_logup_general: 1 when some lookup of the AIR is not plain, 0 otherwise (0 for an AIR without lookups); BAD_AIR for an
 * unknown id.  The fill ("LogUp FREQUENCIES" below), extended: the keys of a table are its COLUMN's values; a looked-up cell is
 * skipped when its filter is 0 on the row, looked up and counted when it is 1, and counts as MISSING on its row when it is anything
 * else; an AIR is fillable when every frequencies COLUMN is one plain column that no COLUMN or FILTER of any lookup reads and no two
 * lookups share. */
int starkhip_air_logup_general(starkhip_air_t air);

/* --- user-defined AIRs ------------------------------------------------------------------
 * A starky user's own `impl Stark` reaches the library as its constraint program: the blob starkhip_air_program returns (format:
 * starky_bls12_381_amd/csrc/air_ir.h and INTEGRATION.md; starky_bls12_381_amd/air_builder.py builds one).  starkhip_air_check_program
 * is the validator every registration runs: OK, or STARKHIP_ERR_BAD_AIR with the reason in `why` (NUL-terminated, truncated to
 * why_len; why may be NULL).  What it accepts cannot make a kernel, the plan builder or a verifier address outside its buffers. */
int starkhip_air_check_program(const uint64_t* blob, size_t words, char* why, size_t why_len);
/* Validates and registers a program; *id_out is its id from then on, for every entry point that takes an AIR (prove, the pools,
 * verify, verify_batch, the queries above, starkhip_check_trace).  The same blob again: the same id (its first name and rows stay).
 * name may be NULL; default_rows is 0 or a power of two in 2..2^STARKHIP_MAX_LOG_ROWS (what starkhip_air_default_rows reports).  BAD_AIR for a program
 * the validator refuses or a full registry (STARKHIP_AIR_CUSTOM_CAPACITY), BAD_SHAPE for bad arguments.  Thread-safe.  A registered
 * AIR has no trace generator: starkhip_pool_submit_witness and the witness batch refuse it with BAD_AIR.  Its config
 * (starkhip_config_for_air) is standard_fast with the smallest rate_bits >= 1 with 2^rate_bits >= degree - 1. */
int starkhip_air_register(const uint64_t* blob, size_t words, const char* name, uint32_t default_rows, starkhip_air_t* id_out);
/* Does `trace` satisfy the AIR?  Every row r is checked with local = r, next = (r + 1) mod n: plain constraints on every row,
 * transition constraints on rows < n - 1, first-row ones on row 0, last-row ones on row n - 1 -- oracle_check_trace's rule.
 * *violations = the (row, constraint) pairs whose value is nonzero; first = {constraint, row, value} of the lowest violated constraint
 * and, of its rows, the lowest (all zero when there is none).  trace, n_rows, n_cols, layout, on_device and public_inputs (the AIR's
 * count) as starkhip_prove takes them -- a cell is any 64-bit word of its class mod p, and the answer is the one for the trace reduced
 * mod p, here, in the report and in the free-cell audit below (their host replays included) -- one call at a time per context, not
 * beside a prove on it.  The constraints are evaluated on the context's device (csrc/kernels_check.hip), which reduces every cell
 * as it loads it; a value is recomputed on the host from the one frame. */
int starkhip_check_trace(void* ctx, starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout, int on_device,
                         const uint64_t* public_inputs, uint64_t* violations, uint64_t first[3]);
/* The same check, reported in full: which constraints fail, on which rows, and the values of the first of them.  The rule, trace,
 * n_rows, n_cols, layout, on_device, public_inputs and the BAD_SHAPE cases are starkhip_check_trace's; cap > STARKHIP_CHECK_LIST_MAX,
 * a NULL `out`, or a NULL `list` with cap > 0 are BAD_SHAPE too.  One call at a time per context, not beside a prove on it.
 *   per_constraint[k] (starkhip_air_num_constraints(air) entries, or NULL): the rows on which constraint k is violated;
 *   row_mask ((n_rows + 63) / 64 words, or NULL): bit (r & 63) of word r >> 6 is set when some constraint is violated on row r;
 *   list (cap x {constraint, row, value}; may be NULL when cap == 0): the first min(cap, violations) violations in the order
 *     (constraint ascending, then row ascending), each with the value G * body of that constraint on that row as the device
 *     computed it (canonical, nonzero).  A cut inside a constraint's rows keeps its lowest rows.  The list is the same on every run.
 * A satisfying trace gives an all-zero report.  Two passes on the context's device (csrc/kernels_check.hip): one counts,
 * and, when there is something to list, one over the chunks of the listed constraints writes the entries; the host orders them.
 * starkhip_check_trace itself is unchanged and cheaper: it is the one to ask "does it hold?". */
#define STARKHIP_CHECK_LIST_MAX (1u << 20)
typedef struct {
    uint64_t violations;            /* (row, constraint) pairs with a nonzero value: starkhip_check_trace's number */
    uint64_t constraints_violated;  /* constraints with at least one such row */
    uint64_t rows_violated;         /* rows with at least one such constraint */
    uint64_t listed;                /* entries written to `list`: min(cap, violations) */
} starkhip_check_report_t;
int starkhip_check_trace_report(void* ctx, starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout, int on_device,
                                const uint64_t* public_inputs, uint32_t* per_constraint, uint64_t* row_mask, uint64_t* list, size_t cap,
                                starkhip_check_report_t* out);
/* tests: starkhip_check_trace_report's host side (argument checks, selection of the listed constraints, ordering, truncation, summary)
 * with the two device passes replayed by host loops over the program's per-constraint evaluator, which fill each constraint's
 * entries in a scrambled row order.  `trace` is host memory.  It walks the program on every row, each pass, on one thread --
 * O(rows x program), times up to a group's length for the constraints late in a group: for small shapes.  No device needed. */
int starkhip_check_trace_report_replay(starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout,
                                       const uint64_t* public_inputs, uint32_t* per_constraint, uint64_t* row_mask, uint64_t* list, size_t cap,
                                       starkhip_check_report_t* out);
/* --- the check inside prove() ------------------------------------------------------------------------------------
 * With the context option "check_trace" = 1 (a pool's "check_traces") every starkhip_prove, _prove_columns and _prove_compact runs
 * starkhip_check_trace's rule -- every constraint on every row, cells read mod p -- on the copy of the trace it has just put in device
 * memory (parked in the LDE buffer, in the trace buffer, or the caller's own column-major device memory read in place), after the
 * upload and before anything of the LDE is enqueued.  Nothing goes up twice, and it works for a recording and a column table, which the
 * stand-alone checkers do not take.  A satisfying trace: the proof goes on, with the bytes it has without the option.  A violating one:
 * the call returns STARKHIP_ERR_TRACE, no later phase has been enqueued (a pooled proof has not asked for its commitment), the context
 * stays usable, and *proof / *proof_words hand back a CHECK BLOB instead of a proof -- library-owned, released with starkhip_free:
 *   word 0  STARKHIP_CHECK_MAGIC ("SSCHK001"; a proof starts with the proof magic)     word 4  constraints_violated
 *   word 1  AIR id                                                                     word 5  rows_violated
 *   word 2  n_rows                                                                     word 6  listed
 *   word 3  violations                                                                 word 7  0
 *   then listed x {constraint, row, value}: what starkhip_check_trace_report returns for the same trace with cap = "check_trace_list"
 *   (0 .. STARKHIP_CHECK_LIST_MAX, default 16) -- same order, same values, same cut.  `violations` is starkhip_check_trace's count and
 *   entry 0 its `first`.
 * The plain check kernel decides (24.6 ms for FinalExp); the report's two passes run only for a violating trace.  The
 * first checked proof of an AIR on a context allocates the AIR's check program on the device, and a device allocation waits for every
 * stream of the device: a pool sees one such pause per context and AIR (there is no warm-up for it).
 * starkhip_check_blob_layout validates magic and length (BAD_SHAPE otherwise; a proof blob, a truncated blob and one whose `listed`
 * disagrees with its length are refused) and points *list (may be NULL) into the blob, NULL when nothing is listed.
 * starkhip_check_stats: out = {traces checked, traces rejected} by this context's proofs so far. */
#define STARKHIP_CHECK_MAGIC 0x3130304B48435353ULL
int starkhip_check_blob_layout(const uint64_t* blob, size_t words, starkhip_check_report_t* out, const uint64_t** list);
int starkhip_check_stats(void* ctx, uint64_t out[2]);
/* tests: what a checking prove must hand back for `trace` (host memory) with "check_trace_list" = cap, without a device: STARKHIP_OK
 * and *blob = NULL for a satisfying trace, STARKHIP_ERR_TRACE and the blob (starkhip_free) otherwise.  Built on
 * starkhip_check_trace_report_replay: for small shapes.  Arguments and BAD_SHAPE cases as there. */
int starkhip_check_blob_replay(starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout, const uint64_t* public_inputs,
                               size_t cap, uint64_t** blob, size_t* words);
/* The opposite question: which cells of the trace could a prover change without any constraint noticing?  Under-constrained cells
 * are a soundness bug that a satisfying trace never shows.  `delta` is a nonzero canonical field element.  Cell (r, c) is CAUGHT
 * when some constraint that reads column c is nonzero on the frame the read puts the cell in, with this one cell replaced by
 * cell + delta mod p: a read as a local cell tests frame r, a read as a next cell tests frame (r - 1) mod n, a constraint that reads
 * c both ways tests both, each with only its own occurrence changed; and the constraint has to apply to that frame by
 * starkhip_check_trace's rule (plain: every row, the wrap frame n - 1 included; transition: rows < n - 1; first / last: row 0 / n - 1).
 * Every other cell is FREE: all cells of a column no constraint reads, row 0 of a column that only transition constraints read and
 * only as `next`, a gated cell on the rows where its gate is off.  The trace itself need not satisfy the AIR: a cell is free when
 * the constraints that read it are all zero AFTER the change; on a satisfying trace that is "the changed trace still satisfies".
 *   per_column (n_cols entries, or NULL): the free rows of each column;
 *   free_mask (n_cols x (n_rows + 63) / 64 words, or NULL): bit (r & 63) of word r >> 6 of column c is set when cell (r, c) is free;
 *     bits at or beyond n_rows are zero.  It is read back from the device only when asked for (75 MB for FinalExp);
 *   out: cells = n_rows * n_cols, free_cells, free_columns (all n_rows rows free), partly_free_columns.
 * Two limits.  The test is NECESSARY, NOT SUFFICIENT: it changes one cell at a time and does not see a cheat that changes several
 * cells together.  And it is PROBABILISTIC IN delta: a constrained cell reads as free for at most `degree` values of delta per
 * (constraint, cell) pair -- the roots of the constraint as a polynomial in delta -- so draw delta at random for a real audit.
 * trace, n_rows, n_cols, layout, on_device, public_inputs and the BAD_SHAPE cases are starkhip_check_trace's; delta == 0,
 * delta >= p and a NULL `out` are BAD_SHAPE too.  The result is a pure function of the arguments, the same on every run.  One call at
 * a time per context, not beside a prove on it; starkhip_check_trace, the report and their results are unchanged.  On the context's
 * device it is the run of starkhip_check_trace_free_cell_classes below (csrc/kernels_free_classes.hip), whose caught plane,
 * complemented on the rows of the trace, is free_mask: several times the plain check's work. */
typedef struct {
    uint64_t cells;                /* n_rows * n_cols */
    uint64_t free_cells;           /* cells no constraint notices */
    uint64_t free_columns;         /* columns with all n_rows rows free */
    uint64_t partly_free_columns;  /* columns with some, not all, rows free */
} starkhip_free_cells_t;
int starkhip_check_trace_free_cells(void* ctx, starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout,
                                    int on_device, const uint64_t* public_inputs, uint64_t delta, uint32_t* per_column,
                                    uint64_t* free_mask, starkhip_free_cells_t* out);
/* tests: the same rule as host loops over the program's per-constraint evaluator on changed frames, on one thread -- O(rows x
 * (constraint, cell) pairs x constraint length): for small shapes.  `trace` is host memory.  No device needed. */
int starkhip_check_trace_free_cells_replay(starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout,
                                           const uint64_t* public_inputs, uint64_t delta, uint32_t* per_column, uint64_t* free_mask,
                                           starkhip_free_cells_t* out);
/* The audit's free cells, told apart: of the cells starkhip_check_trace_free_cells calls free, which does no constraint read, which
 * are read only behind closed gates, and which are read with the gates open and still not noticed?  Only the last class is where a
 * missing constraint hides.  An OCCURRENCE is constraint k reading column c as a local or as a next cell (a gate counts as a read).
 * It puts cell (r, c) in frame r (local) or frame (r - 1) mod n (next), and it counts only when k applies to that frame.  On that
 * frame, with this one cell replaced by cell + delta mod p (only this occurrence's read changed), let G' be the product of the
 * group's gates (1 for a group without gates) and body' the constraint's body.  Per cell, over its counting occurrences:
 *   read:   there is one;   open: some has G' != 0;   caught: some has G' * body' != 0 -- starkhip_check_trace_free_cells's rule, bit
 *   for bit.  read contains open contains caught, and the classes are CAUGHT = caught, SILENT = open and not caught (a body with no
 *   live coefficient for the cell on that frame, e.g. a zero co-factor), GATED = read and not open, UNREAD = not read (padding, a
 *   column no constraint reads, row 0 of a column read only as `next`).  SILENT, GATED and UNREAD partition the audit's free cells.
 * G' is taken AFTER the change: a cell that is itself a gate opens or closes its own gate.  open_rows[k] is taken on the UNCHANGED
 * trace: the frames r constraint k applies to with G != 0 -- zero for a constraint this trace never exercised.
 *   per_column (n_cols x 3, or NULL): the silent, gated and unread rows of each column;
 *   planes (3 x n_cols x (n_rows + 63) / 64 words, or NULL): plane 0 read, 1 open, 2 caught, each laid out as free_mask above, bits
 *     at or beyond n_rows zero.  Cumulative, not disjoint class masks: the audit of several traces of one shape is the OR of their
 *     planes.  Read back from the device only when asked for (3 x 75 MB for FinalExp);
 *   open_rows (starkhip_air_num_constraints(air) entries, or NULL);
 *   out: cells = caught + silent + gated + unread, the columns holding a silent cell, the constraints with open_rows[k] == 0.
 * The audit's two limits carry over: NECESSARY, NOT SUFFICIENT (one cell at a time), and PROBABILISTIC IN delta (a caught cell reads
 * as silent, an open one as gated, for the at most `degree` roots in delta per occurrence).  Arguments, layouts, the BAD_SHAPE cases
 * (delta == 0, delta >= p, a NULL `out`) and "one call at a time per context, not beside a prove" are starkhip_check_trace_free_cells's;
 * cells are read mod p, the trace need not satisfy the AIR, and the result is a pure function of the arguments, the same bytes on
 * every run.  On the context's device (csrc/kernels_free_classes.hip) every constraint is re-evaluated once per cell it reads, the
 * body skipped where every gate product of the wave is zero, and the audit is this run's caught plane; the other checkers and their
 * results are unchanged. */
typedef struct {
    uint64_t cells, caught, silent, gated, unread;  /* caught + silent + gated + unread == cells */
    uint64_t silent_columns;                        /* columns with at least one silent cell */
    uint64_t constraints_never_open;                /* constraints with open_rows[k] == 0 */
} starkhip_free_cell_classes_t;
int starkhip_check_trace_free_cell_classes(void* ctx, starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout,
                                           int on_device, const uint64_t* public_inputs, uint64_t delta, uint32_t* per_column,
                                           uint64_t* planes, uint32_t* open_rows, starkhip_free_cell_classes_t* out);
/* tests: the same rule as host loops on one thread, as starkhip_check_trace_free_cells_replay: for small shapes.  No device needed. */
int starkhip_check_trace_free_cell_classes_replay(starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout,
                                                  const uint64_t* public_inputs, uint64_t delta, uint32_t* per_column, uint64_t* planes,
                                                  uint32_t* open_rows, starkhip_free_cell_classes_t* out);
/* The trace checkers above look at the AIR's own constraints.  This one looks at its PERMUTATION PAIRS (starky's permutation_pairs()),
 * one pair at a time and exactly: are the rows of the pair's lhs columns a permutation of the rows of its rhs columns, and if not,
 * which rows have no partner?  The rule, per pair q of the AIR (not per batch): a row r holds on each side a tuple of n_entries cells,
 * every cell read mod p as every trace reader does.  Let L(v) be the number of lhs rows holding tuple v and R(v) the number of rhs
 * rows holding it.  The pair holds when L(v) = R(v) for every v.  Otherwise, for every v with L(v) > R(v) the L - R HIGHEST lhs rows
 * holding v are UNMATCHED, and for every v with R(v) > L(v) the R - L highest rhs rows holding v are: each side of a pair has the
 * same number of unmatched rows.  The result is a pure function of (AIR, trace mod p), the same bytes on every run whatever `seed`
 * (except for pairs reported undecided, below); the trace need not satisfy the AIR's own constraints.
 * One consequence (COMPAT.md 2a): the argument of a proof uses one (beta, gamma) for a whole batch, so a proof shows only that the
 * UNION of a batch's lhs tuples equals the union of its rhs tuples, with tuples of different widths that agree up to trailing zeros
 * identified.  A trace can close every Z of starkhip_permutation_zs and still fail this check: a finding about how the pairs are
 * batched, not a false alarm.
 * How: the rows are sorted by a 64-bit key, key(row) = sum_t seed^t cell_t mod p (for a one-entry pair the cell itself: exact and
 * independent of the seed), and every item whose key equals its predecessor's compares its tuple with the predecessor's cell by
 * cell.  If all agree, equal keys mean equal tuples and the answer is exact.  If two different tuples shared a key the pair is run
 * again under the next seed, s' = 7 s + 1 mod p (applied again while below 2), STARKHIP_PERM_CHECK_ATTEMPTS seeds in all
 * (starkhip_perm_check_seeds lists them); a pair that still collides is UNDECIDED: per_pair = UINT32_MAX, zero masks, nothing in
 * `unmatched` or `list`, and the call still returns STARKHIP_OK.  As with delta above, draw seed at random for a real audit.
 *   per_pair (starkhip_air_permutation_pairs(air) entries, or NULL): the unmatched rows per side; UINT32_MAX = undecided;
 *   masks (n_pairs x 2 x (n_rows + 63) / 64 words, or NULL): [pair][side: 0 lhs, 1 rhs], bit (r & 63) of word r >> 6 = row r unmatched;
 *   list (cap x {pair, side, row}; may be NULL when cap == 0): the first min(cap, unmatched) flagged rows in the order pair, side
 *     (lhs first), row ascending.
 * trace, n_rows, n_cols, layout, on_device and their BAD_SHAPE cases are starkhip_check_trace's (both layouts, host or device memory,
 * column-major device memory read in place, 2 .. 2^STARKHIP_MAX_LOG_ROWS rows).  BAD_AIR for an unknown AIR or one without pairs;
 * BAD_SHAPE also for seed < 2 or seed >= p, cap > STARKHIP_CHECK_LIST_MAX, a NULL `out`, a NULL `list` with cap > 0.  One call at a
 * time per context, not beside a prove on it.  On the context's device: a stable radix sort and a classification per pair
 * (csrc/kernels_multiset.hip); the masks are read back only for a violated pair and only when `masks` or `list` asks for them. */
#define STARKHIP_PERM_CHECK_ATTEMPTS 4
typedef struct {
    uint64_t pairs, pairs_violated, pairs_undecided;
    uint64_t unmatched;   /* flagged rows over all decided pairs, both sides (even) */
    uint64_t listed;      /* entries written to `list`: min(cap, unmatched) */
    uint64_t reseeds;     /* reruns of a pair because two different tuples shared a key */
} starkhip_perm_check_t;
int starkhip_check_trace_permutations(void* ctx, starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout,
                                      int on_device, uint64_t seed, uint32_t* per_pair, uint64_t* masks, uint64_t* list, size_t cap,
                                      starkhip_perm_check_t* out);
/* tests: the same host driver -- argument checks, the seed sequence, undecided pairs, the list from the masks, the summary -- with the
 * device steps replaced by host loops: the keys, std::stable_sort by key, the same classification.  `trace` is host memory.  No device
 * needed. */
int starkhip_check_trace_permutations_replay(starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout, uint64_t seed,
                                             uint32_t* per_pair, uint64_t* masks, uint64_t* list, size_t cap, starkhip_perm_check_t* out);
/* out = the seeds the check tries for `seed`, in order.  BAD_SHAPE for seed < 2, seed >= p or a NULL out. */
int starkhip_perm_check_seeds(uint64_t seed, uint64_t out[STARKHIP_PERM_CHECK_ATTEMPTS]);
/* ms = {upload and gather of the pair columns, keys and sort passes, classification and counts, read-backs of masks} of the last
 * starkhip_check_trace_permutations on this context: the first three from events on its stream, summed over pairs and attempts, the
 * last the host's time in the copies. */
int starkhip_perm_check_timings(void* ctx, float ms[4]);

/* LOOKUPS.  Nobody declares a permutation pair for its own sake: a pair range-checks a column or looks it up in a table, in the
 * Halo2-style argument plonky2's evm/src/lookup.rs builds on starky's pairs (COMPAT.md 2b).  For a lookup of column a in table
 * column t the trace carries two witness columns: a' a permutation of a, t' a permutation of t, with a'[i] = t'[i] or a'[i] =
 * a'[i - 1] on every row.  This entry FILLS those two columns of a trace, per lookup {input, table, permuted_input, permuted_table}
 * (four column numbers; the call takes no AIR), by one rule -- a pure function of the two multisets, cells read mod p as every trace
 * reader does, outputs canonical:
 *   A = a sorted ascending, T = t sorted ascending; permuted_input = A.  Position i of A is a HEAD when i = 0 or A[i] != A[i - 1];
 *   position j of T is USED when it is the first position of T holding its value and that value occurs in a.  The lookup HOLDS
 *   when every value of a occurs in t; then heads and used positions are equally many, permuted_table[i] = A[i] on every head, and
 *   the k-th non-head position of A takes the k-th unused entry of T (both ascending).  It FAILS when some value of a is absent
 *   from t: those rows of the input column are its MISSING rows, and its two output columns are left exactly as they were; the
 *   other lookups of the call are still written.
 * This is a valid witness, not the one evm's permuted_cols computes (which hands unused table values out last-in first-out).
 * The output columns are written into the caller's trace where it lies: device memory in place (element r of a column at stride 1
 * for layout 1, n_cols for layout 0); of a host trace the four columns of each lookup of a batch go up in one copy and, for a
 * lookup that holds, the two output columns come back.  Nothing else in the trace is touched.
 *   per_lookup (n_lookups entries, or NULL): the missing rows of each lookup;
 *   missing_masks (n_lookups x (n_rows + 63) / 64 words, or NULL): bit (r & 63) of word r >> 6 = row r of the lookup's input is missing;
 *   list (cap x {lookup, row}; may be NULL when cap == 0): the first min(cap, missing_rows) missing rows by lookup, then row.
 * The same bytes on every run.  STARKHIP_OK whether or not lookups failed: the report says.  trace, n_rows, n_cols, layout and
 * on_device are starkhip_check_trace_permutations' (2 .. 2^STARKHIP_MAX_LOG_ROWS rows, a power of two).  BAD_SHAPE for a NULL
 * trace, lookups or out, an unknown layout, rows outside the limits, n_lookups = 0 or > STARKHIP_LOOKUPS_MAX, a column >= n_cols,
 * an output column that is also any lookup's input or table column or another output column of the call, cap >
 * STARKHIP_CHECK_LIST_MAX, a NULL list with cap > 0.  A table column shared by several lookups is fine.  One call at a time per
 * context, not beside a prove on it.  On the context's device: the stable sort of csrc/kernels_multiset.hip, then a mark pass, a scan
 * and two placements per lookup (csrc/kernels_lookup.hip), the lookups of a call in batches that share each launch (grid.y = lookup;
 * DESIGN.md 13c) with one host wait per batch; the placements of a lookup write only when its missing count on the device is zero. */
#define STARKHIP_LOOKUPS_MAX 64
typedef struct {
    uint32_t input, table, permuted_input, permuted_table;
} starkhip_lookup_t;
typedef struct {
    uint64_t lookups, lookups_failed;
    uint64_t missing_rows;   /* over all lookups */
    uint64_t listed;         /* entries written to `list`: min(cap, missing_rows) */
} starkhip_lookup_report_t;
int starkhip_lookup_columns(void* ctx, uint64_t* trace, size_t n_rows, size_t n_cols, int layout, int on_device,
                            const starkhip_lookup_t* lookups, size_t n_lookups, uint32_t* per_lookup, uint64_t* missing_masks,
                            uint64_t* list, size_t cap, starkhip_lookup_report_t* out);
/* tests: the same host driver -- argument checks, the loop over the lookups, the list from the masks, the report -- with the device
 * steps replaced by host loops that implement the rule literally (std::stable_sort).  `trace` is host memory.  No device needed. */
int starkhip_lookup_columns_replay(uint64_t* trace, size_t n_rows, size_t n_cols, int layout, const starkhip_lookup_t* lookups,
                                   size_t n_lookups, uint32_t* per_lookup, uint64_t* missing_masks, uint64_t* list, size_t cap,
                                   starkhip_lookup_report_t* out);
/* ms = {upload or gather of the lookups' columns, keys and sort passes, mark + scan + placements, read-backs of masks and of a host
 * trace's output columns} of the last starkhip_lookup_columns on this context: the first three from events on its stream, summed over
 * the lookups, the last the host's time in the copies. */
int starkhip_lookup_timings(void* ctx, float ms[4]);
/* tests: the program the C++ AirBuilder (csrc/air_ir.h) makes of n_cols columns, no public inputs and `degree` with one
 * AirBuilder::lookup per entry of `lookups` -- per lookup the constraint (N(pi) - L(pi)) (N(pi) - N(pt)), the last-row constraint
 * N(pi) - N(pt), and the pairs [(input, pi)], [(table, pt)] -- for comparison with the Python builder's.  *words = its length; the blob
 * is written when it fits cap_words (BAD_SHAPE otherwise, and for arguments the builder refuses). */
int starkhip_lookup_air_blob(uint32_t n_cols, uint32_t degree, const starkhip_lookup_t* lookups, size_t n_lookups, uint64_t* blob,
                             size_t cap_words, size_t* words);
/* --- an AIR that knows its lookups, and the fill inside prove() ------------------------------------------------------
 * starkhip_air_register_lookups registers a program together with the list of its lookups.  The list is witness information: no
 * verifier reads it and it is no part of the blob.  The registry's key is (blob, list): the same two again return their first id,
 * another list -- or the same blob through starkhip_air_register, which has none -- is another AIR with an id of its own, and a proof
 * made under one id verifies under the other (the program is the same).  starkhip_air_lookups returns the length of an AIR's list and
 * writes its first min(cap, length) entries to `out` (may be NULL); 0 for built-in AIRs, plain registrations and unknown ids.
 * starkhip_air_check_lookups is the validation, callable without registering: STARKHIP_OK, or STARKHIP_ERR_BAD_AIR with the reason in
 * `why` (may be NULL) for a blob starkhip_air_check_program refuses, n_lookups outside 1 .. STARKHIP_LOOKUPS_MAX, a column >= n_cols, a
 * lookup whose two output columns are one, an output column that is any lookup's input or table or another lookup's output, and a
 * lookup whose pairs [(input, permuted_input)] and [(table, permuted_table)] the program does not both declare -- such a list would
 * have the fill write columns that the proof does not bind.
 *
 * With the context option "fill_lookups" = 1 (a pool's option of the same name) every starkhip_prove, _prove_columns and
 * _prove_compact of an AIR that has a list runs starkhip_lookup_columns' rule on the copy of the trace it has just put in device
 * memory: after the upload has left the trace column-major there, BEFORE "check_trace" (which therefore sees the filled columns)
 * and before the pair columns are copied aside for the Zs.  The caller submits a trace whose permuted columns hold anything and gets
 * the proof that starkhip_prove without the option gives for the trace starkhip_lookup_columns would have filled: the same bytes.
 * The caller's buffer is only read: column-major device memory, which prove otherwise reads where it lies, is first copied into the
 * context's own trace buffer (one device-to-device copy of 8 n_rows n_cols bytes) and the proof works on that copy.  The lookups run
 * in batches, one host wait per batch; on its own copy the prover places every lookup without waiting for its count.
 * Some lookup fails: the call returns STARKHIP_ERR_TRACE, no later phase has been enqueued, the context stays usable, starkhip_check_stats
 * counts the trace as checked and rejected, and *proof / *proof_words hand back a LOOKUP BLOB -- library-owned, released with
 * starkhip_free:
 *   word 0  STARKHIP_LOOKUP_MAGIC ("SSLKP001")       word 4  lookups_failed
 *   word 1  AIR id                                   word 5  missing_rows
 *   word 2  n_rows                                   word 6  listed
 *   word 3  lookups                                  word 7  0
 *   then listed x {lookup, row}: starkhip_lookup_columns' list for the same trace and the AIR's list with cap = "check_trace_list".
 * An AIR without a list (every built-in AIR, every plain registration): nothing is enqueued and every byte of every proof is what it is
 * without the option.  starkhip_last_timings[0] includes the fill; starkhip_lookup_timings reports the last fill of the context,
 * whichever entry ran it.  "lookup_batch" (0 = automatic, the default; 1 .. STARKHIP_LOOKUPS_MAX = at most that many lookups share one
 * set of launches) is for tests: results do not depend on it.
 * starkhip_lookup_blob_layout validates magic and length like starkhip_check_blob_layout (a proof, a check blob, a truncated blob and
 * a `listed` that disagrees with the length: BAD_SHAPE).  starkhip_lookup_blob_replay (tests): what a filling prove must hand back for
 * `trace` (host memory, only read) with "check_trace_list" = cap, without a device: STARKHIP_OK and *blob = NULL when every lookup
 * holds or the AIR has no list, STARKHIP_ERR_TRACE and the blob (starkhip_free) otherwise. */
#define STARKHIP_LOOKUP_MAGIC 0x313030504B4C5353ULL
int starkhip_air_check_lookups(const uint64_t* blob, size_t words, const starkhip_lookup_t* lookups, size_t n_lookups, char* why, size_t why_len);
int starkhip_air_register_lookups(const uint64_t* blob, size_t words, const char* name, uint32_t default_rows, const starkhip_lookup_t* lookups,
                                  size_t n_lookups, starkhip_air_t* id_out);
size_t starkhip_air_lookups(starkhip_air_t air, starkhip_lookup_t* out, size_t cap);
int starkhip_lookup_blob_layout(const uint64_t* blob, size_t words, starkhip_lookup_report_t* out, const uint64_t** list);
int starkhip_lookup_blob_replay(starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout, size_t cap, uint64_t** blob,
                                size_t* words);
/* tests: starkhip_lookup_air_blob's program registered with AirBuilder::lookups() as its list */
int starkhip_lookup_air_register(uint32_t n_cols, uint32_t degree, const starkhip_lookup_t* lookups, size_t n_lookups, const char* name, uint32_t default_rows,
                                 starkhip_air_t* id_out);

/* --- LogUp FREQUENCIES -------------------------------------------------------------------------------------------------
 * The witness of a LogUp lookup (starkhip_air_logups above) is its frequencies column.  This entry FILLS the frequencies columns of
 * a trace, for the lookups the AIR's program declares.  The rule, per lookup with m looked-up columns, table column t and
 * frequencies column f over n rows, cells read mod p, outputs canonical:
 *   row r of the table is a FIRST when no row r' < r has t[r'] = t[r]; a looked-up cell is MISSING when its value occurs nowhere in
 *   t; the lookup HOLDS when it has no missing cell.  When it holds, f[r] = the number of cells among the m n looked-up cells that
 *   equal t[r] if r is a first, and 0 otherwise: sum f = m n, and a value the table holds several times gives all its count to the
 *   lowest such row (any split over duplicate table rows closes the argument -- COMPAT.md 2c; this one is the prover's choice).
 *   When the lookup fails, its frequencies column is left exactly as it was; the other lookups of the call are still written.
 *   Nothing but the frequencies columns is written.
 * A pure function of the trace: the device, starkhip_logup_frequencies_replay and a numpy reference agree byte for byte, and two runs
 * give identical bytes.  trace, n_rows, n_cols, layout and on_device as in starkhip_lookup_columns: a device trace is read and written
 * in place in either layout; of a host trace only the distinct columns the lookups read go up and, for a lookup that holds, its
 * frequencies column comes back.
 *   per_lookup (n_lookups entries, or NULL): the missing cells of each lookup;
 *   per_column (sum m entries, or NULL): the missing cells of each looked-up column, the lookups' columns back to back in
 *     declaration order -- it names the offending column;
 *   missing_masks (n_lookups x (n_rows + 63) / 64 words, or NULL): bit (r & 63) of word r >> 6 = row r has at least one missing cell;
 *   list (cap x {lookup, row}; may be NULL when cap == 0): the first min(cap, missing_rows) missing rows by lookup, then row.
 * STARKHIP_OK whether or not lookups failed: the report says.  BAD_AIR for an unknown AIR or one without LogUp lookups; BAD_SHAPE for
 * a NULL trace or out, an unknown layout, a column count that is not the AIR's, rows that are no power of two in
 * 2 .. 2^STARKHIP_MAX_LOG_ROWS, cap > STARKHIP_CHECK_LIST_MAX, a NULL list with cap > 0, and an AIR that is not FILLABLE: one in which
 * a frequencies column is also a looked-up or table column of any lookup or another lookup's frequencies column
 * (starkhip_air_logup_fillable: 1, 0, or BAD_AIR for an unknown AIR or one without LogUp lookups) -- so the order of the lookups does
 * not matter.  One call at a time per context.  Implementation: the table column of each lookup sorted once per distinct table
 * (csrc/kernels_multiset.hip, n items), one lane per looked-up cell counting at the lower bound of its value, one lane per sorted
 * position writing (csrc/kernels_logup_freq.hip); the lookups of a call share each launch, one host wait per batch. */
typedef struct {
    uint64_t lookups, lookups_failed;
    uint64_t missing_cells;  /* over all lookups */
    uint64_t missing_rows;   /* over all lookups: rows with at least one missing cell */
    uint64_t listed;
} starkhip_logup_report_t;
int starkhip_air_logup_fillable(starkhip_air_t air);
int starkhip_logup_frequencies(void* ctx, starkhip_air_t air, uint64_t* trace, size_t n_rows, size_t n_cols, int layout, int on_device,
                               uint32_t* per_lookup, uint32_t* per_column, uint64_t* missing_masks, uint64_t* list, size_t cap,
                               starkhip_logup_report_t* out);
/* tests: the same host driver with the device steps replaced by host loops that follow the rule literally; no device needed */
int starkhip_logup_frequencies_replay(starkhip_air_t air, uint64_t* trace, size_t n_rows, size_t n_cols, int layout, uint32_t* per_lookup,
                                      uint32_t* per_column, uint64_t* missing_masks, uint64_t* list, size_t cap,
                                      starkhip_logup_report_t* out);
/* ms = {upload of a host trace's columns, keys and sort of the tables, count, write, read-backs of masks and of a host trace's
 * frequencies columns} of the last fill on this context, whichever entry ran it: the first four from events on its stream, summed
 * over the batches, the last the host's time in the copies. */
int starkhip_logup_frequency_timings(void* ctx, float ms[5]);
/* The fill inside prove().  With the context option "fill_frequencies" = 1 (a pool's option of the same name) every starkhip_prove,
 * _prove_columns and _prove_compact of a fillable AIR with LogUp lookups runs the rule on the copy of the trace it has just put in
 * device memory, at the place and under the terms of "fill_lookups" above: before "check_trace" and before the named columns are
 * copied aside, the caller's buffer only read (column-major device memory is copied first), the write not gated.  The proof is, byte
 * for byte, the proof of the pre-filled trace without the option.  An AIR with LogUp lookups that is not fillable: STARKHIP_ERR_BAD_AIR.
 * An AIR without LogUp lookups: nothing changes.  Some lookup fails: STARKHIP_ERR_TRACE, nothing later is enqueued, the context stays
 * usable, starkhip_check_stats counts the trace as checked and rejected, and *proof / *proof_words hand back a LOGUP BLOB
 * (starkhip_free), the lookup blob's word layout under its own magic:
 *   word 0  STARKHIP_LOGUP_MAGIC ("SSLGU001")        word 4  lookups_failed
 *   word 1  AIR id                                   word 5  missing_rows
 *   word 2  n_rows                                   word 6  listed
 *   word 3  lookups                                  word 7  missing_cells
 *   then listed x {lookup, row}: starkhip_logup_frequencies' list for the same trace with cap = "check_trace_list".
 * starkhip_logup_blob_layout validates magic and length (anything else, a lookup blob included: BAD_SHAPE; starkhip_lookup_blob_layout
 * refuses a LogUp blob likewise).  starkhip_logup_blob_replay (tests): what a filling prove must hand back for `trace` (host memory,
 * only read) with "check_trace_list" = cap, without a device: STARKHIP_OK and *blob = NULL when every lookup holds, STARKHIP_ERR_TRACE
 * and the blob otherwise; BAD_AIR for an AIR without LogUp lookups or one that is not fillable. */
#define STARKHIP_LOGUP_MAGIC 0x31303055474C5353ULL
int starkhip_logup_blob_layout(const uint64_t* blob, size_t words, starkhip_logup_report_t* out, const uint64_t** list);
int starkhip_logup_blob_replay(starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout, size_t cap, uint64_t** blob,
                               size_t* words);

/* --- natives + trace generation (host)----------------------------------------------- */
/* inputs are u32 limb arrays: Fp = 12, Fp2 = 24, Fp12 = 144 limbs.
 * trace is written row-major [n_rows][columns]; public_inputs has starkhip_air_public_inputs() entries. */
int starkhip_trace_fp12_mul(const uint32_t x[144], const uint32_t y[144], uint64_t* trace, size_t n_rows, uint64_t* public_inputs);
int starkhip_trace_final_exp(const uint32_t x[144], uint64_t* trace, size_t n_rows, uint64_t* public_inputs);
int starkhip_trace_miller_loop(const uint32_t px[12], const uint32_t py[12], const uint32_t qx[24], const uint32_t qy[24],
                               const uint32_t qz[24], uint64_t* trace, size_t n_rows, uint64_t* public_inputs);
int starkhip_trace_pairing_precomp(const uint32_t qx[24], const uint32_t qy[24], const uint32_t qz[24], uint64_t* trace,
                                   size_t n_rows, uint64_t* public_inputs);
/* points: 512 affine G1 points as [x(12 limbs), y(12 limbs)]; bits: 512 bytes (0 / 1).  The aggregate is computed here and
 * written to the last 24 public inputs.  At least one of the first two bits must be set; consecutive operands must differ in x. */
int starkhip_trace_ecc_aggregate(const uint32_t* points, const uint8_t* bits, uint64_t* trace, size_t n_rows, uint64_t* public_inputs);
int starkhip_native_g1_aggregate(const uint32_t* points, const uint8_t* bits, uint32_t out[24]);
int starkhip_trace_fibonacci(uint64_t x0, uint64_t x1, uint64_t* trace, size_t n_rows, uint64_t* public_inputs);
int starkhip_native_fp12_mul(const uint32_t x[144], const uint32_t y[144], uint32_t out[144]);
int starkhip_native_final_exponentiate(const uint32_t x[144], uint32_t out[144]);
int starkhip_native_miller_loop(const uint32_t px[12], const uint32_t py[12], const uint32_t qx[24], const uint32_t qy[24],
                                const uint32_t qz[24], uint32_t out[144]);
int starkhip_native_pairing_precomp(const uint32_t qx[24], const uint32_t qy[24], const uint32_t qz[24], uint32_t out[68 * 72]);

/* --- prover (GPU) -------------------------------------------------------------------- */
int starkhip_init(int device_ordinal, void** ctx);
void starkhip_shutdown(void* ctx);

/* trace_layout: 0 = row-major [n_rows][C] (what generate_trace returns), 1 = column-major [C][n_rows]
 * (what trace_rows_to_poly_values returns).  trace_on_device != 0: `trace` is a device pointer
 * (already resident in HBM; the benchmark path).  pow_witness: STARKHIP_POW_SEARCH = smallest valid
 * nonce, otherwise use the given one.  *proof is a blob in the layout below.
 * Shapes: n_rows a power of two, 2 <= n_rows <= 8192 for a built-in AIR (the reference's largest trace; one LDS image per column) and
 * 2 <= n_rows <= 2^STARKHIP_MAX_LOG_ROWS for a registered one (from 2^14 rows on a column is transformed by several workgroups in two
 * passes: csrc/kernels_lde_long.hip),
 * n_pis and n_cols as the AIR declares (n_cols is checked before the buffer is touched: it is read as n_rows x n_cols words), num_challenges = 2, and rate_bits large enough for the AIR's
 * constraint degree (2^rate_bits >= degree - 1); anything else is STARKHIP_ERR_BAD_SHAPE before any GPU work.
 * Trace cells: a 64-bit word w of the trace is read as the field element w mod p, so p .. 2^64 - 1 are accepted as second
 * representatives of 0 .. 2^32 - 2 (plonky2's GoldilocksField keeps such words in memory).  This holds for every entry that reads a
 * trace -- this one, starkhip_prove_columns, the pools' submits, starkhip_check_trace, its report and the free-cell audit, on host
 * or device memory, in either layout -- and every result (proof bytes, counts, `first`, lists and their values, masks) is what the same
 * call returns for the trace reduced mod p.  The caller's buffer is only read -- with "fill_lookups" too, which fills the permuted
 * columns in the context's own copy (column-major device memory is copied for it; see "the fill inside prove()").  (A refusal would cost a pass over 4.8 GB of a
 * device-resident FinalExp trace, after the point where bad shapes are refused; tests/test_gpu_noncanonical_cells.py.) */
int starkhip_prove(void* ctx, starkhip_air_t air, const starkhip_config_t* cfg, const uint64_t* trace, size_t n_rows, size_t n_cols,
                   int trace_layout, int trace_on_device, const uint64_t* public_inputs, size_t n_pis, uint64_t pow_witness,
                   uint64_t** proof, size_t* proof_words);

/* The same proof from the LITERAL argument of starky's prove(): `trace_poly_values: Vec<PolynomialValues<F>>`
 * (src/aggregate_proof.rs:57-65, :104-111, :137-144, :168-175) is one heap allocation per column -- 73 527 of them for FinalExp.
 * `columns` is a table of n_cols host pointers, each to n_rows words, canonical or not: read mod p, as starkhip_prove reads its
 * trace (PolynomialValues<GoldilocksField>::values; the field type is repr(transparent) over u64, and its words may be >= p).  The library gathers the scattered columns through the context's page-locked staging, half
 * by half under the copies, so a binding at prove() itself needs no 4.8 GB host-side repack.  Byte-identical to starkhip_prove on
 * the same matrix; shapes and errors as starkhip_prove (a NULL column pointer: STARKHIP_ERR_BAD_SHAPE). */
int starkhip_prove_columns(void* ctx, starkhip_air_t air, const starkhip_config_t* cfg, const uint64_t* const* columns, size_t n_rows, size_t n_cols,
                           const uint64_t* public_inputs, size_t n_pis, uint64_t pow_witness, uint64_t** proof, size_t* proof_words);

/* Tuning knobs of a context (defaults are the measured best; tests and profiling tools use them to reach the other code
 * paths): "quotient_impl" 0 = tiled evaluator / 1 = op-stream interpreter, "quotient_cosets" (tiled evaluator only; 0, the default =
 * every constraint is evaluated on the cosets of n_rows points that its own degree needs -- max(1, d - 1) of them for d cell factors, d
 * for a first-row or last-row constraint -- and the classes' values are recombined into the quotient's coefficient chunks; 1 = every
 * constraint on all 2^quotient_degree_bits cosets and one inverse transform of all values.  For a trace that satisfies the AIR the two
 * give the same proof bytes.  For a trace that violates a constraint they do not: the violated class's sum is not divisible by Z_H, so
 * its values on a few cosets and on all of them interpolate to different polynomials; either proof is rejected by the verifier, an AIR
 * whose quotient has a spare coset (degree 4) fails with STARKHIP_ERR_QUOTIENT_NOT_DIVISIBLE either way, and starkhip_check_trace is the
 * tool for such a trace -- or "check_trace" below, which refuses it inside the prove call.  AIRs of degree above 5, AIRs with permutation pairs, the profiling modes and the comparison of the two evaluators always run as 1),
 * "quotient_chunks" (0 = automatic),
 * "check_trace" (0 = default / 1: every prove on the context checks its trace against the AIR before the LDE and returns
 * STARKHIP_ERR_TRACE with a check blob for a violating one -- "the check inside prove()" above), "check_trace_list" (0 ..
 * STARKHIP_CHECK_LIST_MAX, default 16: the violations such a blob lists),
 * "fill_lookups" (0 = default / 1: every prove of an AIR registered with its lookups fills their permuted columns in its own copy of
 * the trace first -- "the fill inside prove()" above; STARKHIP_ERR_TRACE with a lookup blob when a lookup fails), "lookup_batch" (0 =
 * automatic / 1 .. STARKHIP_LOOKUPS_MAX: the lookups that share one set of launches, there and in starkhip_lookup_columns),
 * "fill_frequencies" (0 = default / 1: every prove of a fillable AIR with LogUp lookups fills their frequencies columns in its own
 * copy of the trace first -- "LogUp FREQUENCIES" above; STARKHIP_ERR_TRACE with a LogUp blob when a lookup fails),
 * "logup_count_combine" (1 = default / 0: the count kernel of that fill adds every cell alone; the same bytes, for measurements),
 * "hasher" (STARKHIP_HASHER_POSEIDON, the default, or STARKHIP_HASHER_KECCAK: the hash of every prove entry of the context -- trace
 * and quotient commitments, FRI layers, proof of work and the transcript's sponge.  With 0 every byte of every proof is what it is
 * without the option.  Under STARKHIP_HASHER_KECCAK "leaf_hash_form" and "host_commit_leaves" do not apply: they pick among Poseidon
 * forms and are ignored),
 * "quotient_waves", "quotient_slots", "lde_closed_forms" (1 = constant and unit-vector trace columns take their closed-form LDE
 * instead of five transforms, 0 = every column is transformed; same bytes either way; traces of 2^14 rows and more have no closed forms and transform every column), "host_commit_leaves" (default 64: trace commitments of at most this many leaves -- FP12Mul's 32 -- are hashed by host threads with the
 * challenger's permutation, 0.8 us against 5.6 us per permutation of a lone GPU wave; 0 = never; only with "leaf_hash_form" 0), "leaf_hash_form" (0 = a context on its own
 * hashes commitments of <= 4096 leaves in the row form -- 16 lanes per leaf, the shortest chain per leaf --, those of >= 32 768 leaves in
 * the pair form -- two lanes per leaf, one 256-register wave per SIMD -- and the ones between in the quad form; 1 = quad always; 2 = row always;
 * 3 = lane form, one lane per leaf: what a pool with five or more big contexts uses for groups of big commitments, slower than the pair form for
 * one commitment alone; 4 = pair always; same digests; a pool's commitments always go through its scheduler),
 * "leaf_hash_prefix" (1, the default = the lane and pair forms start the leaves of a Poseidon-hashed trace of 2^12 or 2^13 rows and at
 * least rows + 8 columns from a saved state past its first `rows` columns when those are the unit vectors e_0 .. e_{rows-1} -- FinalExp's
 * one-hot row selectors, 1 024 of its 9 191 permutations per leaf; each proof decides on the device, from what its own LDE found, and a
 * trace without that prefix is hashed in full; 0 = the kernels are never given the saved state; same bytes either way; 1 MB of device
 * memory per context and shape),
 * "lde_impl" (1 = 8192-row traces through lde_columns_v2_kernel instead of the wave-resident kernel; same bytes), "zeta_on_coset"
 * (TESTS ONLY: k + 1 substitutes zeta = 7 w_n^k for the transcript's challenge, a point of the coset the trace values are kept on -- the
 * branch a real transcript takes with probability 2^-115; the result is compared with the oracle under the same substitution and is not a
 * proof the verifier accepts; 0 = off).  Unknown name or value out of range: STARKHIP_ERR_BAD_SHAPE. */
int starkhip_set_option(void* ctx, const char* name, long value);

/* --- compact traces: on-device trace expansion -----------------------------------------------
 * Between starkhip_trace_log_begin and _end the calling thread's ONE starkhip_trace_* call records its writes as runs
 * (a limb vector + the rows it repeats on) instead of filling n_rows x C cells; its `trace` argument is ignored and may
 * be NULL, public inputs are produced as usual.  FinalExp: ~150 MB of records instead of 4.8 GB of rows.
 * starkhip_prove_compact uploads the records and expands them on the device straight into the column-major matrix;
 * the proof is bit-identical to the one from the dense trace.  A log is immutable after _end and may be proven any
 * number of times, from any thread; release it with starkhip_trace_log_free. */
int starkhip_trace_log_begin(void** log);
/* Host threads ONE recording generator call may use (process-wide, default 1; returns the previous value).  Only
 * starkhip_trace_final_exp uses more than one so far: the reference's generate_trace (src/final_exponentiate.rs:240-279) fills
 * its 32 ops one after the other, but once the 32 native results are known every op's rows are independent.  The recorded
 * trace -- and the proof -- does not depend on the setting.  A driver that records many traces at once keeps it at 1. */
int starkhip_trace_set_threads(int n);
int starkhip_trace_log_end(void* log);
void starkhip_trace_log_free(void* log);
int starkhip_trace_log_info(const void* log, size_t* n_rows, size_t* n_cols, size_t* n_records, size_t* n_words);
/* A finished log from explicit cell writes, (row, col, value) triples applied in order through the recorder's `set` (values < 2^32;
 * a zero clears as the fillers' "selector(b) = 0" does).  For tests of the recorder's corner cases -- the generators are the
 * product's way to make a log.  Release with starkhip_trace_log_free. */
int starkhip_trace_log_from_writes(size_t n_rows, size_t n_cols, const uint64_t* writes, size_t n_writes, void** log);
/* The two traces of the fillers' one overwriting idiom ("selector = 1 on rows a..b", then "selector(b) = 0") in a finished log:
 * records whose run the clear took back to ZERO rows (a one-row run cleared again: the record stays in the log and stands for no
 * cell -- kernels_trace.hip skips it) and cells cleared inside a longer run (zeroed after the expansion).  Tests. */
int starkhip_trace_log_overwrites(const void* log, size_t* empty_runs, size_t* late_zeros);
/* CPU replay into a row-major matrix (tests): *conflicts = cells that two records wrote with different values (must be 0) */
int starkhip_trace_log_expand_host(const void* log, uint64_t* trace_rowmajor, size_t* conflicts);
int starkhip_prove_compact(void* ctx, starkhip_air_t air, const starkhip_config_t* cfg, const void* log, const uint64_t* public_inputs,
                           size_t n_pis, uint64_t pow_witness, uint64_t** proof, size_t* proof_words);

/* --- proof pool: submit / wait ------------------------------------------------------------------------------------
 * The reference's caller proves one AIR after the other on one thread (src/aggregate_proof.rs:304-370: pp1, ml1, pp2, ml2,
 * fp12_mul, final_exp; `aggregate_proof` :402-414) and lets rayon fill the cores inside each prove().  On a GPU several
 * proofs in flight are what fills the chip, so the library schedules them itself: a pool owns `big_contexts` prover contexts
 * for the 8192-row AIRs (FinalExp, ECCAgg: 19.6 GB of buffers each) and `small_contexts` for the others, one host thread
 * per context, `generator_threads` host threads that record traces (starkhip_pool_submit_witness), and a commitment
 * scheduler: the trace commitments of small proofs that arrive together are hashed by ONE merged launch (and, by option, a
 * FinalExp-class commitment -- a one-shot grid that owns the chip -- never shares the chip with a small one).  Proofs are byte-identical to
 * starkhip_prove's.  submit returns at once with a ticket; wait blocks until that proof is done and hands it over
 * (starkhip_free), exactly once per ticket, from any thread.  Inputs of submit / submit_compact (trace, log, public inputs)
 * stay the caller's and must stay valid until the ticket has been waited for; submit_witness copies its operands.
 * Hardware queues: starkhip_pool_create sets GPU_MAX_HW_QUEUES=16 unless the variable exists, but the HIP runtime reads it only when
 * the process first uses HIP -- a process that has used HIP before it creates its first pool exports the variable itself, earlier
 * (what four queues cost; starkhip_hw_queues_in_effect: what the process has). */
typedef struct {
    int device;
    unsigned big_contexts;      /* 0 = default (3).  Five or more: the trace commitments of these proofs go out in groups of up to four in the
                                   lane form of the leaf hash (6.3 against 5.65 proofs/s on one MI355X; 19.6 GB of HBM per context,
                                   starkhip_pool_reservation) */
    unsigned small_contexts;    /* 0 = default (16) */
    unsigned generator_threads; /* recordings under way at once; 0 = default (a quarter of the CPUs the process may use -- its
                                   cgroup quota or affinity mask --, 3 .. 12) */
    unsigned trace_threads;     /* host threads ONE recording may use; 0 = automatic (FinalExp-class: 3/4 of the CPU budget, at most 16;
                                   the others at most 4) */
    unsigned commit_policy;     /* 0 = default: small commitments that arrive together share one launch; 1 = in addition a FinalExp-class
                                   commitment never shares the chip with a small one; 2 = no commitment scheduling (every context
                                   launches its own; for A/B measurements) */
    unsigned stream_priority;   /* 0 = all contexts alike; 1 = the last wave of FinalExp-class proofs (no more of them waiting than there are
                                   contexts) on high-priority streams; 2 = the small contexts, 3 = all FinalExp-class proofs (measurements) */
    unsigned warm_up;           /* != 0: starkhip_pool_create returns when every context has allocated what the BLS pipeline's AIRs of its class
                                   need (FinalExp on the big contexts; MillerLoop, PairingPrecomp, FP12Mul on the small ones: tables, constraint
                                   plans, buffers, upload staging), so that no proof pays for -- or stalls the device with -- allocations;
                                   2: the same without the page-locked upload staging: for a caller whose traces are already column-major
                                   device memory (starkhip_pool_submit with trace_on_device) */
    float gather_ms;            /* how long a merged launch waits for small proofs that have started but not reached their commitment; 0 = default (25) */
} starkhip_pool_config_t;
typedef struct {
    float phase_ms[11];   /* as starkhip_last_timings */
    float kernel_ms[3];   /* as starkhip_last_kernel_timings */
    float host_ms[2];     /* as starkhip_last_host_timings */
    double t_submit, t_generate_start, t_generate_end, t_prove_start, t_done; /* seconds since the pool was created */
    int leaf_hash_form;       /* how the trace commitment went out: 0 quad form, 1 row form, 2 one grid merged with other proofs' commitments
                                 (quad form), 3 lane form, 4 hashed by host threads (at most "host_commit_leaves" leaves), 5 pair form,
                                 6 the Keccak leaf hash ("hasher" 1: always the context's own launch); kernel_ms[1] is
                                 that kernel's own duration on its launch stream (form 4: the host's time) */
    unsigned leaf_hash_group; /* commitments that were launched side by side with it (itself included) */
} starkhip_ticket_info_t;
typedef struct {
    unsigned long big_commit_launches, small_commit_launches, small_commit_requests, max_merged_commitments;
    unsigned long big_commit_grids; /* kernel launches behind big_commit_launches (which counts commitments): a lane-form group is ONE grid */
} starkhip_pool_stats_t;
int starkhip_pool_create(const starkhip_pool_config_t* cfg, void** pool);
void starkhip_pool_destroy(void* pool); /* runs what is queued to the end first */
/* as starkhip_prove / starkhip_prove_compact */
int starkhip_pool_submit(void* pool, starkhip_air_t air, const starkhip_config_t* cfg, const uint64_t* trace, size_t n_rows, size_t n_cols,
                         int trace_layout, int trace_on_device, const uint64_t* public_inputs, size_t n_pis, uint64_t pow_witness,
                         uint64_t* ticket);
/* as starkhip_prove_columns; the pointer TABLE is copied before this returns, the columns themselves (and the public inputs) stay the
 * caller's until the ticket has been waited for */
int starkhip_pool_submit_columns(void* pool, starkhip_air_t air, const starkhip_config_t* cfg, const uint64_t* const* columns, size_t n_rows,
                                 size_t n_cols, const uint64_t* public_inputs, size_t n_pis, uint64_t pow_witness, uint64_t* ticket);
int starkhip_pool_submit_compact(void* pool, starkhip_air_t air, const starkhip_config_t* cfg, const void* log, const uint64_t* public_inputs,
                                 size_t n_pis, uint64_t pow_witness, uint64_t* ticket);
/* generate_trace + prove (src/aggregate_proof.rs:23-179, one driver each) from the driver's operands as u32 limbs, packed:
 *   FP12_MUL x[144] y[144];  FINAL_EXP x[144];  MILLER_LOOP px[12] py[12] qx[24] qy[24] qz[24];  PAIRING_PRECOMP qx[24] qy[24] qz[24];
 *   ECC_AGGREGATE points[512][24] then 512 words of 0 / 1;  TEST_FIBONACCI x0 (lo, hi) x1 (lo, hi).
 * The trace is recorded on a generator thread of the pool (default rows of the AIR); cfg == NULL: starkhip_config_for_air.
 * The public inputs are the tail of the proof blob. */
int starkhip_pool_submit_witness(void* pool, starkhip_air_t air, const starkhip_config_t* cfg, const uint32_t* operands, size_t n_limbs,
                                 uint64_t pow_witness, uint64_t* ticket);
/* returns the proof's status (what starkhip_prove would have returned); info may be NULL */
int starkhip_pool_wait(void* pool, uint64_t ticket, uint64_t** proof, size_t* proof_words, starkhip_ticket_info_t* info);
int starkhip_pool_stats(void* pool, starkhip_pool_stats_t* out);
/* What the pool has reserved (a warmed pool: everything its proofs will ever need; read it between proofs): device memory of all
 * contexts, page-locked upload staging, and the largest context of each class.  A FinalExp-class context holds the LDE (19.3 GB; the trace
 * columns wait for it inside that buffer, row-major uploads and recordings are staged in it before the LDE kernel writes it, and
 * coefficients are not kept) and ~ 0.3 GB of small buffers. */
typedef struct {
    uint64_t device_bytes, pinned_host_bytes, big_context_device_bytes, small_context_device_bytes;
    unsigned big_contexts, small_contexts;
} starkhip_pool_reservation_t;
int starkhip_pool_reservation(void* pool, starkhip_pool_reservation_t* out);
/* The host side of a pool: the CPUs it plans with -- the process's budget (cgroup quota, else affinity mask, divided by
 * LOCAL_WORLD_SIZE under torch.distributed.run and by the number of pools of a multi-device handle: starkhip_cpu_budget is the
 * process's figure before that last division) --, its generator threads, the threads one recording of each class may use, and its
 * prover threads (one per context; they launch kernels, hash the Fiat-Shamir transcript and gather uploads).  A scaling curve that
 * bends for want of host CPUs shows here: a pool whose budget is 2 records one FinalExp trace at a time on one thread (212 ms). */
typedef struct {
    unsigned cpu_budget, generator_threads, trace_threads_big, trace_threads_small, prover_threads;
    int device;
    unsigned pools_on_device; /* pools of the same multi-device handle on this pool's device: 1, unless the handle was given one ordinal
                               * several times -- the rehearsal of N devices on one card (the tests do it); such a handle's figures are not a
                               * measurement of N devices, and starkhip_multipool_create says so once on stderr */
    unsigned hw_queues;       /* starkhip_hw_queues_in_effect: hardware queues per stream priority class of this process */
    unsigned stream_budget;   /* default-class streams this pool can have busy at once (at most 16); above hw_queues its contexts share queues */
} starkhip_pool_host_info_t;
int starkhip_pool_host_info(void* pool, starkhip_pool_host_info_t* out);
unsigned starkhip_cpu_budget(void);
/* Where the pools' host CPU time goes, process-wide and cumulative (seconds of CPU, not of wall): [0] recording traces (the generator
 * threads inside starkhip_trace_* and the helper threads of multi-threaded recordings), [1] the context threads inside prove() (kernel
 * launches, the challenger's Fiat-Shamir sponge, gathering uploads, the FRI batches' host arithmetic), [2] the part of [1] spent INSIDE the waits for the device (an event wait that sleeps costs next to nothing).  What a process's
 * total CPU time holds beyond these two is the HIP runtime's own threads and the caller. */
void starkhip_host_cpu_seconds(double out[3]);
/* Proof blobs of a warmed pool are recycled page-locked buffers (the final device-to-host copy of 21 .. 69 MB runs at PCIe rate and
 * touches no fresh pages); starkhip_free() hands them back.  Process-wide counters: [0] blobs held, [1] of them with a caller,
 * [2] bytes held, [3] proofs served from them, [4] proofs served by malloc (no idle blob that fits).  STARKHIP_PINNED_PROOFS=0 in
 * the environment of starkhip_pool_create turns the reservation off. */
void starkhip_proof_blob_stats(uint64_t out[5]);

/* 0: GPU_MAX_HW_QUEUES was in the environment before the HIP runtime came up (the library's 16 or the caller's own value); 1: the
 * runtime was already initialised when the first pool / multi-device handle of this process set it, so the pools run on HIP's default
 * of 4 hardware queues (a line on stderr says so once).  Detected without touching HIP (the runtime's open /dev/kfd).
 * 0 says WHEN the variable was set, not that its value is enough: starkhip_hw_queues_in_effect is the number of hardware queues per
 * stream priority class the process really has -- the variable's value when it was in the environment before the runtime came up (the
 * caller's own value is respected, never overridden), 4 when it came late; 0 before the first pool of the process.  A pool whose
 * default-class streams outnumber it (a stream per context and one per merged window: 10 for eight big contexts and a small one) shares
 * queues among its contexts, and starkhip_pool_create says so once on stderr.  The pool's launches that last hundreds of milliseconds
 * (lane-form groups, the lone pair-form commitment) run in a priority class of their own and hold none of those queues, so four are
 * enough for them. */
int starkhip_hw_queues_status(void);
int starkhip_hw_queues_in_effect(void);

/* --- verification inside a pool ----------------------------------------------------------------------------------
 * The reference's drivers call verify_stark_proof straight after prove (src/aggregate_proof.rs:67,113,146,177).  A pool does the same on its
 * own device: a verifier per pool with persistent device memory (an arena in two halves), its own stream at normal priority, preludes on
 * a few host threads (at the generator threads' nice value) and proofs batched as their preludes finish; after its one-time setup it
 * allocates nothing and never synchronises the device.
 * Options (STARKHIP_ERR_BAD_SHAPE for an unknown name or a value out of range):
 *   "verify_proofs"   0 (default) or 1: every proving ticket submitted from then on is checked before starkhip_pool_wait returns it.  OK: wait
 *                     behaves as without the option; otherwise wait returns starkhip_verify's code (STARKHIP_ERR_VERIFY, BAD_SHAPE) and
 *                     frees the proof.  The verifier reads the host blob the caller receives; the prover context is free already.
 *   "verify_arena_mb" the verifier's device memory (default 1024), allocated at the first verify work, or when "verify_proofs" is
 *                     switched on in a pool created with warm_up.  A proof larger than half of it is verified alone.  Changing it
 *                     once the arena exists: STARKHIP_ERR_BAD_SHAPE.
 *   "check_traces"    0 (default) or 1: every proving ticket submitted from then on has its trace checked against the AIR by its context,
 *                     as the context option "check_trace" does, whichever submit it came through (a witness job's recording included).
 *                     A violating trace: starkhip_pool_wait returns STARKHIP_ERR_TRACE and hands over the check blob in *proof
 *                     (starkhip_free); with "verify_proofs" on as well it never reaches the verifier.
 *   "check_trace_list" 0 .. STARKHIP_CHECK_LIST_MAX (default 16): the violations such a blob lists; read at submit too.
 *   "fill_lookups"    0 (default) or 1: every proving ticket submitted from then on has the permuted columns of its AIR's lookups filled
 *                     by its context, as the context option "fill_lookups" does, before "check_traces" looks at the trace.  A failing
 *                     lookup: starkhip_pool_wait returns STARKHIP_ERR_TRACE and hands over the lookup blob in *proof (starkhip_free);
 *                     it never reaches the verifier, and starkhip_pool_check_stats counts it as rejected.
 *   "fill_frequencies" 0 (default) or 1: the same for the frequencies columns of the LogUp lookups of a ticket's AIR, as the context
 *                     option "fill_frequencies" does; a failing lookup hands over the LogUp blob.  Read at submit too.
 *   "hasher"          STARKHIP_HASHER_POSEIDON (default) or STARKHIP_HASHER_KECCAK: the hasher of every proving ticket submitted from then
 *                     on, as the context option "hasher".  A Keccak proof's trace commitment is launched by its context on its own stream,
 *                     not by the pool's commitment scheduler (whose merged and lane-group launches are Poseidon forms): the counters of
 *                     starkhip_pool_stats do not move for it and its ticket reports leaf_hash_form 6.  The pool's verifier
 *                     ("verify_proofs", verify jobs) takes each proof's hasher from its header, whatever this option says. */
int starkhip_pool_set_option(void* pool, const char* name, long value);
/* out = {traces checked, traces rejected}, summed over the pool's contexts (per slot of a multi-device handle: starkhip_multipool_pool) */
int starkhip_pool_check_stats(void* pool, uint64_t out[2]);
/* A verification job for any proof (of this pool, another one, or the oracle); cfg == NULL: starkhip_config_for_air.  The proof stays the
 * caller's until the ticket has been waited for.  starkhip_pool_wait on the ticket returns exactly starkhip_verify's code for it (OK,
 * VERIFY, BAD_SHAPE, BAD_AIR), or HIP / OOM if the device work failed; it sets *proof = NULL and *proof_words = 0, and of `info` only
 * t_submit, t_prove_start (the prelude started) and t_done (every other field is zero). */
int starkhip_pool_submit_verify(void* pool, starkhip_air_t air, const starkhip_config_t* cfg, const uint64_t* proof, size_t proof_words,
                                uint64_t* ticket);
/* cumulative: proofs checked for "verify_proofs", verify jobs, rejections (of both), device batches; the batches' summed upload and
 * kernel time (ms of stream time), the preludes' summed wall ms and the prelude threads' CPU seconds; the arena's bytes (0: none yet) */
typedef struct {
    unsigned long proofs_checked, verify_jobs, rejected, device_batches;
    double upload_ms, device_ms, prelude_ms, prelude_cpu_s;
    uint64_t arena_bytes;
} starkhip_pool_verify_stats_t;
int starkhip_pool_verify_stats(void* pool, starkhip_pool_verify_stats_t* out);

/* --- one caller, many devices -------------------------------------------------------------------------------------
 * The reference's caller is ONE process: generate_aggregate_proof issues its six proves from one thread (src/aggregate_proof.rs:304-370,
 * `aggregate_proof` :402-414).  A multi-device handle lets that caller use a node of GPUs as it is -- no process group, no collective
 * (the proofs are independent; operands reach every pool through host memory): one proof pool per entry of
 * `devices` (an ordinal may repeat: two pools on one card), each configured by `cfg` (cfg->device is ignored), the process's CPU budget
 * split between them.  Jobs are placed longest processing time first: `slot` = -1 lets the library choose -- a FinalExp-class job goes
 * to the pool with the fewest of them open, any job to the pool with the least outstanding cost (starkhip_air_cost), ties to the lowest
 * slot -- and `slot` >= 0 names the pool (required for a trace in device memory: it lives on one device).  submit_witness_batch places a
 * whole batch in order of decreasing cost (ties in the caller's order): BASELINE configs[3] (one signature's six proofs on six
 * devices: each pool gets one) and configs[4] (48 proofs on 8: every device gets a FinalExp proof first, then two MillerLoop, ...).
 * Tickets are the handle's own (they carry the slot); everything else -- proofs, ownership, errors, ticket info -- is as starkhip_pool_*.
 * starkhip_multipool_pool hands out the pool of a slot for starkhip_pool_stats / _reservation (not for submit / wait / destroy). */
int starkhip_multipool_create(const int* devices, size_t n_devices, const starkhip_pool_config_t* cfg, void** mpool);
void starkhip_multipool_destroy(void* mpool); /* runs what is queued to the end first */
size_t starkhip_multipool_size(const void* mpool);
void* starkhip_multipool_pool(void* mpool, size_t slot);
int starkhip_multipool_device(const void* mpool, size_t slot);
int starkhip_multipool_submit(void* mpool, int slot, starkhip_air_t air, const starkhip_config_t* cfg, const uint64_t* trace, size_t n_rows,
                              size_t n_cols, int trace_layout, int trace_on_device, const uint64_t* public_inputs, size_t n_pis,
                              uint64_t pow_witness, uint64_t* ticket);
int starkhip_multipool_submit_columns(void* mpool, int slot, starkhip_air_t air, const starkhip_config_t* cfg, const uint64_t* const* columns,
                                      size_t n_rows, size_t n_cols, const uint64_t* public_inputs, size_t n_pis, uint64_t pow_witness,
                                      uint64_t* ticket);
int starkhip_multipool_submit_compact(void* mpool, int slot, starkhip_air_t air, const starkhip_config_t* cfg, const void* log,
                                      const uint64_t* public_inputs, size_t n_pis, uint64_t pow_witness, uint64_t* ticket);
int starkhip_multipool_submit_witness(void* mpool, int slot, starkhip_air_t air, const starkhip_config_t* cfg, const uint32_t* operands,
                                      size_t n_limbs, uint64_t pow_witness, uint64_t* ticket);
/* operands[i] / n_limbs[i] as starkhip_pool_submit_witness takes them; tickets[i] = 0 and rcs[i] (may be NULL) != 0 for a job that was
 * refused; returns the first failure */
int starkhip_multipool_submit_witness_batch(void* mpool, size_t n_jobs, const starkhip_air_t* airs, const uint32_t* const* operands,
                                            const size_t* n_limbs, uint64_t pow_witness, uint64_t* tickets, int* rcs);
int starkhip_multipool_ticket_slot(const void* mpool, uint64_t ticket); /* -1: not a ticket of this handle */
int starkhip_multipool_wait(void* mpool, uint64_t ticket, uint64_t** proof, size_t* proof_words, starkhip_ticket_info_t* info);
/* the option on every pool of the handle */
int starkhip_multipool_set_option(void* mpool, const char* name, long value);
/* as starkhip_pool_submit_verify; slot = -1: the pool with the least outstanding verify cost (starkhip_air_verify_cost) */
int starkhip_multipool_submit_verify(void* mpool, int slot, starkhip_air_t air, const starkhip_config_t* cfg, const uint64_t* proof,
                                     size_t proof_words, uint64_t* ticket);
/* starkhip_verify_batch's contract, with the proofs spread over the handle's devices as verify jobs: longest first by
 * starkhip_air_verify_cost, each to the pool with the least cost so far (starkhip_plan_verify) */
int starkhip_multipool_verify_batch(void* mpool, size_t n, const starkhip_air_t* airs, const starkhip_config_t* cfgs, const uint64_t* const* proofs,
                                    const size_t* proof_words, int* results);
/* that placement alone (no GPU needed): slots[i] for proof i on n_pools idle pools, order[k] the k-th proof placed (order may be NULL);
 * starkhip_air_verify_cost: the CPU verifier's milliseconds per proof of the AIR (profiles/r07_verify_device_split.json) */
int starkhip_plan_verify(size_t n, const starkhip_air_t* airs, size_t n_pools, int* slots, size_t* order);
double starkhip_air_verify_cost(starkhip_air_t air);
/* the placement rule alone (no GPU needed): the slot each job of a batch gets on n_pools idle pools; starkhip_air_cost is the relative
 * single-GPU proving cost the rule uses (FinalExp 92, MillerLoop 12.5, PairingPrecomp 4.5, ECCAgg 3, FP12Mul 0.22) */
int starkhip_plan_lpt(size_t n_jobs, const starkhip_air_t* airs, size_t n_pools, int* slots);
double starkhip_air_cost(starkhip_air_t air);

/* per-phase device timings of the last prove on this ctx, milliseconds (HIP events; with "check_trace" on, [0] includes the check):
 * [0] upload/transpose [1] ifft+lde [2] trace leaf hash + merkle [3] quotient (for an AIR with permutation pairs: the Z polynomials,
 * their LDE and commitment first) [4] quotient commit
 * [5] openings [6] fri combine [7] fri commit [8] pow [9] queries [10] total */
#define STARKHIP_N_PHASES 11
int starkhip_last_timings(void* ctx, float ms[STARKHIP_N_PHASES]);
/* durations (ms, HIP events on the launch stream) of the three heavy kernels of the last prove:
 * [0] the trace's LDE kernel, the sum of its launches (lde_columns_wave_kernel for 8192 rows, lde_columns_v2_kernel for the other sizes
 * from 2^8 on and with "lde_impl" = 1) [1] the trace commitment's leaf hash in the form it went out in (leaf_hash_kernel / _row_kernel /
 * _lane_kernel / _pair_kernel / merged) [2] quotient_tiles_kernel */
int starkhip_last_kernel_timings(void* ctx, float ms[3]);
/* host time (ms, wall) inside the last prove: [0] Fiat-Shamir hashing -- the challenger's sequential Poseidon sponge over the
 * caps, the 2 (2 C + Q) opening words and the FRI data, on the proof's critical path (it falls inside the device phases
 * "fri_combine" and "fri_commit" above) -- [1] the other host arithmetic (the two divisions by X - z of the FRI batches) */
int starkhip_last_host_timings(void* ctx, float ms[2]);

/* Page-locked, reusable host memory for traces (starkhip_trace_* take any pointer).  Measured on FinalExp (4.8 GB of
 * rows): the upload itself already runs at link speed from pageable memory (86 ms, 56 GB/s) and stays there; what a
 * long-lived buffer saves is the first-touch page faulting of a fresh 4.8 GB allocation per trace (host generation
 * 815 -> 315 ms).  Needs an initialised context; release with starkhip_host_free. */
int starkhip_host_alloc(void* ctx, size_t bytes, void** out);
void starkhip_host_free(void* p);

/* --- kernel-level entry points (parity tests / micro-benchmarks) ---------------------- */
/* The Z polynomials of an AIR with permutation pairs on one trace, as prove() computes them (csrc/kernels_permutation.hip): trace as
 * in starkhip_check_trace (layout 0 row-major / 1 column-major, host or device memory, any word of a cell's class mod p);
 * challenges: B x 2 x {beta, gamma} canonical words, set-major (B = max(1, degree - 1)); zs_out [nZ][n_rows]: Z[0] = 1,
 * Z[r + 1] = Z[r] ratio(r); closing_out [nZ]: Z[n - 1] ratio(n - 1), 1 exactly when the batch's lhs and rhs agree as multisets (up to
 * the challenges' luck).  The inverse of a zero denominator is 0.  BAD_AIR for an unknown AIR or one without pairs, BAD_SHAPE for a
 * bad trace argument, rows that are no power of two in 2 .. 2^STARKHIP_MAX_LOG_ROWS or a challenge >= p. */
int starkhip_permutation_zs(void* ctx, starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout, int on_device,
                            const uint64_t* challenges, uint64_t* zs_out, uint64_t* closing_out);
/* the same from plain loops on the host (host memory only); no device needed */
int starkhip_permutation_zs_replay(starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout, const uint64_t* challenges,
                                   uint64_t* zs_out, uint64_t* closing_out);
/* starkhip_air_eval_frame plus the permutation constraints (COMPAT.md P4): zs / zs_next hold nZ pairs (the Z openings at zeta and
 * g zeta), challenges B x 2 x {beta, gamma} base-field words; acc_out is the fold over all K + 2 nZ constraints -- the AIR's own K,
 * then nZ first-row constraints Z_i - 1, then nZ plain ones Z_i(next) prod red_rhs - Z_i(local) prod red_lhs.  For an AIR without pairs
 * zs, zs_next and challenges may be NULL and the result is starkhip_air_eval_frame's.  Host only. */
int starkhip_air_eval_frame_full(starkhip_air_t air, const uint64_t* local, const uint64_t* next, const uint64_t* public_inputs,
                                 const uint64_t masks[8], const uint64_t* alphas, int n_alpha, const uint64_t* zs, const uint64_t* zs_next,
                                 const uint64_t* challenges, uint64_t* acc_out);
/* The auxiliary polynomials of an AIR with LogUp lookups on one trace, as prove() computes them (csrc/kernels_logup.hip): trace as in
 * starkhip_permutation_zs; challenges: chi_0, chi_1, canonical words; polys_out [nA][n_rows], challenge-major, per lookup its helpers
 * h_j(r) = sum over batch j of 1 / (chi + c(r)) and then Z with Z[0] = 0, Z[r + 1] = Z[r] + sum_j h_j(r) - f(r) / (chi + t(r));
 * closing_out [2][n_lookups], challenge-major: Z[n - 1] plus the last row's increment, 0 exactly when the frequencies hold the
 * multiplicities (up to the challenges' luck); *zero_denominators_out: how many chi + cell were zero -- their inverse is taken as 0.
 * BAD_AIR for an unknown AIR or one without LogUp lookups, BAD_SHAPE for a bad trace argument, rows that are no power of two in
 * 2 .. 2^STARKHIP_MAX_LOG_ROWS or a challenge >= p. */
int starkhip_logup_polys(void* ctx, starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout, int on_device,
                         const uint64_t* challenges, uint64_t* polys_out, uint64_t* closing_out, uint64_t* zero_denominators_out);
/* the same from plain loops on the host (host memory only); no device needed */
int starkhip_logup_polys_replay(starkhip_air_t air, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout, const uint64_t* challenges,
                                uint64_t* polys_out, uint64_t* closing_out, uint64_t* zero_denominators_out);
/* starkhip_air_eval_frame plus the LogUp constraints (COMPAT.md L4): aux / aux_next hold nA pairs (the auxiliary openings at zeta and
 * g zeta), challenges chi_0, chi_1 base-field words; acc_out is the fold over all K + nL constraints -- the AIR's own K, then per
 * (challenge, lookup) the helper constraints h_j prod (chi + c) - sum_c prod_{c' != c} (chi + c'), Z on the first row, and
 * (Z(next) - Z) (chi + t) - (sum_j h_j) (chi + t) + f.  For an AIR without LogUp lookups aux, aux_next and challenges may be NULL and
 * the result is starkhip_air_eval_frame's.  Host only. */
int starkhip_air_eval_frame_logup(starkhip_air_t air, const uint64_t* local, const uint64_t* next, const uint64_t* public_inputs,
                                  const uint64_t masks[8], const uint64_t* alphas, int n_alpha, const uint64_t* aux, const uint64_t* aux_next,
                                  const uint64_t* challenges, uint64_t* acc_out);
/* values column-major [C][n] (host) -> coeffs [C][n] and LDE [C][N] in NATURAL point order i <-> 7*w_N^i.  1 <= log_n <=
 * STARKHIP_MAX_LOG_ROWS and rate_bits <= 8, BAD_SHAPE otherwise; from log_n 14 on through csrc/kernels_lde_long.hip */
int starkhip_lde_batch(void* ctx, const uint64_t* values, size_t n_cols, unsigned log_n, unsigned rate_bits, uint64_t* coeffs_out,
                       uint64_t* lde_out);
/* n_vecs vectors of 2^log_len words (16 <= log_len <= 26; BAD_SHAPE otherwise) transformed in place by the multi-workgroup transform, as
 * prove() transforms the quotient's values and the FRI layers: X[k] = sum_j x[j] w^(jk), or the inverse with 2^-log_len (inverse != 0) */
int starkhip_ntt_long(void* ctx, uint64_t* data, size_t n_vecs, unsigned log_len, int inverse);
/* Merkle cap of the matrix whose leaf j is the row bitrev(j) of an LDE given column-major natural order [C][N] */
int starkhip_merkle_cap(void* ctx, const uint64_t* lde_colmajor, size_t n_cols, unsigned log_N, unsigned cap_height, uint64_t* cap_out);
int starkhip_poseidon_permute_batch(void* ctx, uint64_t* states, size_t n_states);
/* micro-benchmark: the values -> LDE kernel prove() uses for this shape on n_cols synthetic columns already in HBM, `const_per_64` of
 * every 64 of them constant (these take a closed form; a FinalExp trace has 11 in 64), `reps` launches between two HIP events; average
 * milliseconds per launch.  const_per_64 + 256: unit vectors instead of constants.  device_values != NULL: the caller's own column-major
 * matrix in device memory (n_cols x 2^log_n words) instead of the synthetic one.  reps == 0: one launch with no warm-up launch in front
 * of it.  each_ms (may be NULL): min(reps, 16) durations, launch by launch.  log_n up to STARKHIP_MAX_LOG_ROWS and rate_bits <= 8
 * (BAD_SHAPE otherwise); columns of 2^14 rows and more have no closed forms, so const_per_64 changes nothing there */
int starkhip_lde_bench(void* ctx, size_t n_cols, unsigned log_n, unsigned rate_bits, unsigned reps, unsigned const_per_64, const uint64_t* device_values,
                       float* ms_per_launch, float* each_ms);
/* a finished log through the device's expansion kernels (csrc/kernels_trace.hip) into a host matrix, COLUMN-major [C][n_rows] */
int starkhip_trace_log_expand_device(void* ctx, const void* log, uint64_t* trace_colmajor);
/* device field arithmetic under test: out[i] = canonical(op(a[i], b[i])) with the lazy-reduction helpers the kernels use
 * (op codes: starky_bls12_381_amd/csrc/kernels_selftest.hip); lets the tests feed boundary operands */
int starkhip_field_ops_batch(void* ctx, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
/* the leaf-hash forms' permutations under test, on whole 12-word states in place (a sponge fixes its first block's capacity, so the
 * commitments cannot steer values into a later round): form 0 the generic loop, 1 quad, 2 row, 3 lane, 4 pair ("leaf_hash_form"),
 * each through the function its leaf kernel calls; variant 0 = the full permutation, variant 1 (quad, lane, pair) = the form with the
 * capacity-only last round, which specifies words 8 .. 11 (pair: 2 .. 5 and 8 .. 11) -- the other words come back unchanged.  Canonical
 * words out.  STARKHIP_ERR_BAD_SHAPE for a form or variant that does not exist, before any device work. */
int starkhip_poseidon_permute_batch_form(void* ctx, int form, int variant, uint64_t* states, size_t n_states);
/* the lane-form leaf hash under test, as a proof pool launches it: n_segments (1 .. 4) coset-major matrices of one shape, each [n_cols][N],
 * N = 2^(log_n + rate_bits) leaves, one after the other in `mats`; grouped != 0: ONE grid over all of them (grid.y = matrix, the pool's
 * lane-form group), grouped == 0: the per-commitment launch, one per matrix.  digests_out: n_segments x N x 4 words, leaf digests in
 * tree order.  STARKHIP_ERR_BAD_SHAPE, before any device work, for no or more than four segments, no columns, or more than 2^20 leaves
 * (a leaf count is a power of two by construction: the tree order is a bit reversal).
 * form: 3 the lane form, 4 the pair form (per-commitment launches only: BAD_SHAPE with grouped != 0).  prefix_mask, bit s: segment s is
 * given the context's saved state past an identity prefix ("leaf_hash_prefix") for this shape and the counter as the context's last
 * starkhip_lde_batch of this shape left it -- that call counts the columns c < n that are e_c, as prove() does -- so the segment skips
 * its first n / 8 blocks exactly when that LDE's first n columns were the identity and n_cols >= n + 8; the other segments, and every
 * segment with "leaf_hash_prefix" = 0 or for a shape without the table (log_n other than 12 and 13), get null pointers and hash every
 * block.  BAD_SHAPE for a mask bit beyond the segments. */
int starkhip_leaf_hash_lane_group(void* ctx, const uint64_t* mats, size_t n_segments, size_t n_cols, unsigned log_n, unsigned rate_bits, int grouped,
                                  int form, unsigned prefix_mask, uint64_t* digests_out);
/* the table behind "leaf_hash_prefix" under test: cap_out [4][N], N = 2^(log_n + rate_bits): word w of the sponge's capacity of leaf
 * q = s n + k (coset s, point k of the coset-major LDE) after the columns e_0 .. e_{n-1}.  BAD_SHAPE for log_n other than 12 and 13 or
 * with the option at 0. */
int starkhip_leaf_prefix_table(void* ctx, unsigned log_n, unsigned rate_bits, uint64_t* cap_out);
/* CPU check (no GPU needed) of the constant tables the leaf-hash kernels use for their merged partial rounds -- three at a time in the
 * quad form, four at a time in the lane and pair forms: replays both formulations on n_states inputs against the plain permutation;
 * returns the number of mismatches (0 = good), -1 if a sum of the four-round merge would not fit its 64-bit accumulator */
int starkhip_selfcheck_hash_tables(unsigned n_states);
/* The host-built table a leaf-hash form's kernels read from constant memory (no GPU needed; form 1 quad, 2 row, 3 lane, 4 pair as in
 * "leaf_hash_form"): returns the image's size in bytes and copies it to `out` when `cap` suffices; 0 for an unknown form */
size_t starkhip_hash_table_image(int form, void* out, size_t cap);
/* The launch plan of a trace's LDE (no GPU needed).  The trace columns wait for the LDE inside the buffer the LDE is written to, as
 * its last n_cols * n words, so the LDE goes out in several launches, each overwriting only parked columns that an earlier launch
 * has read; the last one reads a copy of its columns (csrc/lde_ranges.h).  Writes up to `cap` launches as triples
 * {first column, end column, 1 if it reads the copy} and returns how many the plan has. */
size_t starkhip_lde_launch_ranges(size_t n_cols, unsigned rate_bits, uint64_t* triples, size_t cap);
/* The config rule above for a trace of 2^log_n rows (no GPU needed): STARKHIP_OK and the FRI geometry -- up to `cap` reduction
 * arity bits in arities_out, the layer count in *n_layers and the final polynomial's length in *final_poly_len -- or
 * STARKHIP_ERR_BAD_SHAPE for a config every entry point refuses.  The AIR-dependent part (rate_bits against the degree) is not
 * checked here. */
int starkhip_fri_geometry(const starkhip_config_t* cfg, unsigned log_n, unsigned* arities_out, size_t cap, size_t* n_layers,
                          size_t* final_poly_len);
/* CPU check (no GPU needed) of the tiled constraint plan the quotient kernel executes (csrc/quotient_plan.h): builds the plan
 * of `air` with `want_chunks` chunks, derives the per-proof weights from random alphas / public inputs and replays the
 * record streams on one random frame with the kernel's own accumulators; the result must equal the plain fold
 * acc = acc * alpha + mask * c_k over all constraints.  stats = {chunks, supergroups, pieces, records, LDS cell records,
 * direct loads, tiles, term contributions}.  0 = equal, STARKHIP_ERR_VERIFY = different, BAD_SHAPE = malformed plan. */
int starkhip_quotient_plan_check(starkhip_air_t air, unsigned want_chunks, uint64_t seed, uint64_t stats[8]);
/* The class of every constraint of `air` (n = its constraint count): the number of cosets of n_rows points that fix the constraint's
 * part of the quotient -- max(1, d - 1) for a plain or transition constraint with d cell factors (gates + longest monomial), d for a
 * first-row or last-row one, at most the quotient factor. */
int starkhip_quotient_classes(starkhip_air_t air, uint8_t* classes, size_t n);
/* The constants that turn the classes' values on their cosets into the quotient's coefficient chunks, 656 words: [t] the inverse of
 * coset t's shift g_t = 7 w^t (w of order rows << quotient_degree_bits); [8 + 8 t + m] c_t^m with c_t = g_t^rows; [72 + (8 k + m) 8 + t]
 * entry (m, t) of the inverse of the k x k Vandermonde matrix c_t^m. */
int starkhip_quotient_solve_table(unsigned log_rows, unsigned quotient_degree_bits, uint64_t* out, size_t n);
/* CPU replay of the per-class plans ("quotient_cosets" = 0) on one random frame: every class's chunks give the plain fold restricted
 * to the constraints of that class, the classes add up to the whole fold, and the plan of coset t holds the classes above t and no other.
 * stats: [0] classes, [1] cosets, [2] chunks, [3] work rows, [4] records, [5] piece ends, [6] tile phases, [7] contributions,
 * [8 + c] constraints of class c + 1, [24 + t] chunks of coset t. */
int starkhip_quotient_class_plan_check(starkhip_air_t air, unsigned want_chunks, uint64_t seed, uint64_t stats[32]);
/* --- the Keccak hasher under test (COMPAT.md K1 - K8; csrc/keccak.h) ---
 * keccak256 of `len` bytes on the host: Keccak-f[1600], rate 136, padding 0x01 .. 0x80 (not SHA-3's 0x06), 32 bytes out */
void starkhip_keccak256(const uint8_t* bytes, size_t len, uint8_t out32[32]);
/* the challenger's permutation under STARKHIP_HASHER_KECCAK on the host, in place (canonical words in and out): the 12 elements as 96
 * little-endian bytes, h1 = keccak256 of them, h2 = keccak256 of h1, ...; each h gives four little-endian words, words >= p are
 * skipped, and the first 12 accepted words are the new state */
void starkhip_keccak_permute_host(uint64_t state12[12]);
/* that word filter alone, the function host and device code share: the words below p of words[0 .. n) fill state12 in order; returns
 * how many words it consumed up to and including the twelfth accepted one, or -1 when the stream holds fewer than 12 such words
 * (state12 then holds the ones it found, the rest untouched) */
int starkhip_keccak_state_from_words(const uint64_t* words, size_t n, uint64_t state12[12]);
/* the same permutation on the device, n states of 12 words in place */
int starkhip_keccak_permute_batch(void* ctx, uint64_t* states, size_t n);
/* starkhip_merkle_cap under `hasher`: Merkle tree of the matrix whose leaf j is the row bitrev of j of an LDE given column-major in
 * natural order [n_cols][2^log_N]; digests_out: the 2^log_N leaf digests x 4 words in tree order, or NULL; cap_out: 2^cap_height x 4.
 * Hasher 0 hashes the leaves in the form a lone proof of this shape would.  BAD_SHAPE for an unknown hasher, no columns, or
 * log_N < cap_height or > 28 */
int starkhip_merkle_tree_hasher(void* ctx, int hasher, const uint64_t* lde_colmajor, size_t n_cols, unsigned log_N, unsigned cap_height,
                                uint64_t* digests_out, uint64_t* cap_out);
/* digests (n_leaves x 4 words) of row-major leaves rows[n_leaves][width] under `hasher`, as the FRI layers are hashed */
int starkhip_hash_rows_hasher(void* ctx, int hasher, const uint64_t* rows, size_t width, size_t n_leaves, uint64_t* digests_out);
/* host-side permutation (the one the Fiat-Shamir challenger uses) */
void starkhip_poseidon_permute_host(uint64_t state[12]);
/* n chained host permutations; which = 0: the challenger's tuned permutation, 1: the portable loop */
void starkhip_poseidon_permute_host_many(uint64_t state[12], size_t n, int which);

/* --- verifier (CPU) ------------------------------------------------------------------- */
int starkhip_verify(starkhip_air_t air, const starkhip_config_t* cfg, const uint64_t* proof, size_t proof_words);

/* --- verifier (GPU) -------------------------------------------------------------------
 * The same verdicts as starkhip_verify (verify_stark_proof, src/aggregate_proof.rs:67,113,146,177) for a batch of proofs, with the
 * query rounds -- the verifier's bulk: a re-hash of each opened trace leaf and a dot product over it -- on the context's device.
 * The host runs each proof's prelude (shapes, the Fiat-Shamir replay, proof of work, the quotient identity at zeta) on at most 16
 * threads.  Returns STARKHIP_OK when the call ran; results[i] is then exactly what starkhip_verify returns for proof i (OK,
 * STARKHIP_ERR_VERIFY, STARKHIP_ERR_BAD_SHAPE or STARKHIP_ERR_BAD_AIR).  NULL ctx: STARKHIP_ERR_NO_DEVICE; HIP and OOM errors
 * describe the call, not a proof.  Proofs are uploaded in chunks of at most the context option "verify_chunk_mb" of device memory
 * (default 1024; a proof bigger than that goes alone); page-locked pool blobs are copied directly, other memory through a
 * page-locked staging buffer.  Not concurrently with prove() on the same context. */
int starkhip_verify_batch(void* ctx, size_t n, const starkhip_air_t* airs, const starkhip_config_t* cfgs, const uint64_t* const* proofs,
                          const size_t* proof_words, int* results);
/* the last starkhip_verify_batch of this context: host prelude ms, upload ms (stream time of the copies), device ms (kernels),
 * and the process's CPU seconds during the call */
int starkhip_last_verify_timings(void* ctx, double out[4]);
/* tests: starkhip_verify_batch's host side with the device's part replayed on the CPU (same descriptors, the same per-query
 * routine, the host permutation); no device needed */
int starkhip_verify_batch_replay(size_t n, const starkhip_air_t* airs, const starkhip_config_t* cfgs, const uint64_t* const* proofs,
                                 const size_t* proof_words, int* results);

void starkhip_free(void* p);
const char* starkhip_error_string(int code);

/* Proof blob, uint64 words (canonical field order of StarkProofWithPublicInputs):
 *   [0..16)  header: magic "SSPRF001", C, Q, degree_bits, rate_bits, cap_height, L (FRI layers),
 *            num_query_rounds, final_poly_len, n_pis, arity_bits, num_challenges, hasher (STARKHIP_HASHER_*: 0 for Poseidon),
 *            nZ (permutation Z polynomials: 0 for an AIR without permutation pairs, at most 128),
 *            nA (LogUp auxiliary polynomials: 0 for an AIR without LogUp lookups, at most 1024; never beside nZ),
 *            nC (cross-table-lookup polynomials of a table proof of a system: 4 per endpoint, behind the nA in the same matrix; 0 otherwise)
 *   trace_cap[2^cap_h][4]; [nZ > 0: permutation_zs_cap[2^cap_h][4];] quotient_polys_cap[2^cap_h][4]
 *   openings.local_values[C][2]; openings.next_values[C][2];
 *   [nZ > 0: openings.permutation_zs[nZ][2]; openings.permutation_zs_next[nZ][2];] openings.quotient_polys[Q][2]
 *   commit_phase_merkle_caps[L][2^cap_h][4]
 *   query_round_proofs[num_query_rounds]:
 *       trace leaf[C], trace siblings[log N - cap_h][4], [nZ > 0: Z leaf[nZ], Z siblings[log N - cap_h][4],]
 *       quotient leaf[Q], quotient siblings[log N - cap_h][4],
 *       steps[L]: evals[2^arity][2], siblings[log(N / arity^(l+1)) - cap_h][4]
 *   final_poly[final_poly_len][2]; pow_witness; public_inputs[n_pis]
 * A proof with nA > 0 has the same shape with its auxiliary polynomials in the Zs' place: auxiliary_polys_cap, openings.auxiliary_polys[nA][2]
 * and openings.auxiliary_polys_next[nA][2], the auxiliary leaf[nA] and its siblings.  A proof with nZ = nA = 0 has exactly the bytes it always had.
 * A table proof of a system (nC > 0) has nA + nC polynomials in that matrix, LogUp || CTL, and after public_inputs one more section:
 *   ctl_sums[nC / 2], challenge-major and then in the table's endpoint order.
 */
#define STARKHIP_PROOF_MAGIC 0x3130304652505353ULL

/* Offsets (in uint64 words) of every field of the blob above, so that a caller fills the fields of
 * StarkProofWithPublicInputs (src/aggregate_proof.rs:59, consumed at :67 and :435-439) without parsing the layout by hand.
 * q_* are offsets inside one query round (each round is query_round_words long, round r starts at
 * off_query_rounds + r * query_round_words); siblings are 4 words each. */
typedef struct {
    size_t n_columns, n_quotient_polys, degree_bits, rate_bits, cap_height, n_fri_layers, n_query_rounds, final_poly_len,
        n_public_inputs, arity_bits;
    size_t off_trace_cap, off_quotient_cap, off_local_values, off_next_values, off_quotient_openings, off_fri_caps, off_query_rounds,
        query_round_words, off_final_poly, off_pow_witness, off_public_inputs, total_words;
    size_t q_trace_leaf, q_trace_siblings, q_quotient_leaf, q_quotient_siblings, initial_sibling_count;
    size_t q_step_evals[16], q_step_siblings[16], step_sibling_count[16];
    /* permutation arguments (all 0 for a proof with nZ = 0) */
    size_t n_permutation_zs, off_permutation_zs_cap, off_permutation_zs, off_permutation_zs_next, q_permutation_zs_leaf, q_permutation_zs_siblings;
    /* LogUp lookups: nA (0 for a proof without them).  With nA > 0 the five positions above are those of the auxiliary polynomials,
     * which take the Zs' place in the blob, and n_permutation_zs is 0 */
    size_t n_logup_polys;
    /* cross-table lookups: nC (0 unless the blob is a table proof of a system) and where its nC / 2 sums are.  With nC > 0 the middle
     * matrix holds n_logup_polys + n_ctl_polys polynomials */
    size_t n_ctl_polys, off_ctl_sums;
} starkhip_proof_layout_t;
/* STARKHIP_ERR_BAD_SHAPE when the blob's header is not a proof header or disagrees with proof_words */
int starkhip_proof_layout(const uint64_t* proof, size_t proof_words, starkhip_proof_layout_t* out);
/* the hasher id in the proof's header (STARKHIP_HASHER_*), or STARKHIP_ERR_BAD_SHAPE for a blob that is not a proof or names an unknown
 * hasher.  The verify entries accept either hasher; a caller that insists on one asks here. */
int starkhip_proof_hasher(const uint64_t* proof, size_t proof_words);

/* ---- Cross-table lookups: several registered AIRs proved and verified as one system (COMPAT.md 2d, C1 - C8).
 * A system is an ordered list of T >= 2 tables (registered AIRs without permutation pairs, degree >= 2) and a list of CTLs.  CTL k has
 * a width w, one looked endpoint and L >= 1 looking endpoints; an endpoint is (table, w Columns, one Filter) in the word encoding of
 * the general LogUp section.  For both challenge pairs (beta, gamma) the proof shows  sum over looking of S = S of looked,  where
 * S = sum over rows of filter / (gamma + sum_j beta^j column_j).  The filter's value is the multiplicity.
 * System blob (uint64 words): STARKHIP_SYSTEM_MAGIC, T, T table ids, K, then per CTL: w, L, and its 1 + L endpoints, the looked one
 * first, each: table, w (again), w COLUMNs, FILTER.
 * System proof blob: STARKHIP_SYSTEM_PROOF_MAGIC, T, T + 1 word offsets (table t's proof is [off[t], off[t + 1]); off[T] is the length),
 * then the T table proofs in table order. */
#define STARKHIP_SYSTEM_MAGIC 0x31304C5443535953ULL       /* "SYSCTL01" */
#define STARKHIP_SYSTEM_PROOF_MAGIC 0x31304650535953ULL   /* "SYSPF01" */
#define STARKHIP_SYSTEM_CAPACITY 1024
typedef int starkhip_system_t;
/* STARKHIP_OK, or STARKHIP_ERR_BAD_AIR with the reason in why (may be NULL): a table id that is no registered AIR, a table with
 * permutation pairs or of degree 1, an endpoint's table out of range, a width mismatch between a CTL's endpoints, a column outside
 * its table's n_cols, a Column or Filter beyond the LogUp term limits (16 terms, 4 products, 4 sums), nA + nC above
 * STARKHIP_AIR_MAX_LOGUP_POLYS for some table, a blob that ends early or late, and a count beyond the limits below */
#define STARKHIP_SYSTEM_MAX_TABLES 64u   /* T: tables of a system (at least 2) */
#define STARKHIP_SYSTEM_MAX_CTLS 256u    /* K: CTLs of a system */
#define STARKHIP_SYSTEM_MAX_LOOKING 64u  /* L: looking endpoints of one CTL (at least 1) */
#define STARKHIP_CTL_MAX_WIDTH 64u       /* w: columns of an endpoint (at least 1) */
int starkhip_system_check(const uint64_t* blob, size_t words, char* why, size_t why_len);
/* registers a system that passes the check; the same blob again returns its first id */
int starkhip_system_register(const uint64_t* blob, size_t words, starkhip_system_t* id_out);
/* getters: T, K, table t's AIR, table t's endpoints E_t (its proof carries nC = 4 E_t polynomials and 2 E_t sums); a negative code otherwise */
int starkhip_system_tables(starkhip_system_t sys);
int starkhip_system_ctls(starkhip_system_t sys);
int starkhip_system_table_air(starkhip_system_t sys, size_t table);
int starkhip_system_table_endpoints(starkhip_system_t sys, size_t table);
/* A system prover: one context per table on one device.  starkhip_system_set_option sets a context option ("hasher", ...) on all of them. */
int starkhip_system_create(int device, starkhip_system_t sys, void** handle);
void starkhip_system_destroy(void* handle);
int starkhip_system_set_option(void* handle, const char* name, long value);
/* starkhip_last_timings of table `table`'s context: the phases of that table's last proof (its two halves).  The quotient phase starts
 * where the table's CTL polynomials are enqueued, so they and the auxiliary commitment are timed with it; what the table's stream idles
 * after its trace commitment, while the other tables' first halves run, is counted in trace_merkle, and the host's work between the
 * CTL polynomials and the second half (the other tables' polynomials, the balances) in quotient. */
int starkhip_system_last_timings(void* handle, size_t table, float out_ms[STARKHIP_N_PHASES]);
/* One proof of the whole system.  Per table t: cfgs[t] (the configs may differ in rate_bits only), traces[t] with n_rows[t] rows in
 * layouts[t] (0 row-major, 1 column-major) in host or (on_device[t]) device memory, public_inputs[t] with n_pis[t] words.  Every
 * table's trace is committed once; the system transcript draws the CTL challenges from all the trace caps.  If some CTL's sums do not
 * balance, or a denominator was zero, nothing auxiliary is committed: STARKHIP_ERR_QUOTIENT_NOT_DIVISIBLE with the first such CTL in
 * *failing_ctl (may be NULL; -1 otherwise; zero denominators are counted per endpoint, so the CTL named is the first that does not
 * balance or has one), and the handle stays usable.  *proof is freed with starkhip_free. */
int starkhip_system_prove(void* handle, const starkhip_config_t* cfgs, const uint64_t* const* traces, const size_t* n_rows, const int* layouts,
                          const int* on_device, const uint64_t* const* public_inputs, const size_t* n_pis, uint64_t pow_witness, uint64_t** proof,
                          size_t* proof_words, int* failing_ctl);
/* the CPU verifier of a system proof: the system transcript replayed from the table proofs' trace caps, every table proof from the
 * copied state (the four CTL constraints at zeta with the sums taken from the proof), every CTL's sum equation under both challenges.
 * starkhip_verify and starkhip_verify_batch, given a table proof with endpoints alone, answer STARKHIP_ERR_BAD_SHAPE. */
int starkhip_system_verify(starkhip_system_t sys, const starkhip_config_t* cfgs, const uint64_t* proof, size_t proof_words);
/* the T + 1 offsets of a system proof blob into offsets[cap] (cap >= T + 1) and T into *n_tables; STARKHIP_ERR_BAD_SHAPE otherwise */
int starkhip_system_proof_layout(const uint64_t* proof, size_t proof_words, size_t* n_tables, size_t* offsets, size_t cap);
/* the rows one workgroup of the running sums' scan takes (tests put their row counts on either side of its multiples) */
unsigned starkhip_ctl_span_rows(void);
/* tests: the CTL polynomials [4 E][n_rows] (per (challenge, endpoint) h then Z), the sums [2 E] and the count of zero denominators of
 * table `table` on one trace under challenges {beta_0, gamma_0, beta_1, gamma_1}: through the kernels the system prover uses, and from
 * plain loops on the host */
int starkhip_ctl_polys(void* ctx, starkhip_system_t sys, size_t table, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout, int on_device,
                       const uint64_t* challenges, uint64_t* polys_out, uint64_t* sums_out, uint64_t* zero_denominators_out);
int starkhip_ctl_polys_replay(starkhip_system_t sys, size_t table, const uint64_t* trace, size_t n_rows, size_t n_cols, int layout,
                              const uint64_t* challenges, uint64_t* polys_out, uint64_t* sums_out, uint64_t* zero_denominators_out);
/* tests: starkhip_air_eval_frame_logup of the table's AIR continued over the table's 8 E CTL constraints.  aux / aux_next: the
 * nA + nC middle-matrix polynomials at the point and the next row's (2 words each), logup_challenges {chi_0, chi_1} (read only with
 * nA > 0), ctl_challenges[4], sums [2 E] */
int starkhip_system_eval_frame_ctl(starkhip_system_t sys, size_t table, const uint64_t* local, const uint64_t* next, const uint64_t* public_inputs,
                                   const uint64_t masks[8], const uint64_t* alphas, int n_alpha, const uint64_t* aux, const uint64_t* aux_next,
                                   const uint64_t* logup_challenges, const uint64_t* ctl_challenges, const uint64_t* sums, uint64_t* acc_out);

#ifdef __cplusplus
}
#endif
#endif

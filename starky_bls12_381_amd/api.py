"""ctypes binding of libstarkhip.so (C ABI in include/starkhip.h).

Host-side mirror of the reference's call surface for the starky prove() path
(/root/reference/src/aggregate_proof.rs:23-179): `StarkConfig`, `prove`, `verify_stark_proof`,
per-AIR `generate_trace`.  Python is only the harness here; all work happens behind the C ABI.
There is NO CPU fallback: if the shared library is missing, importing this module raises.
"""
import ctypes as C
import os
import time
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# STARKHIP_LIBRARY: another build of the same C ABI (the sanitizer build of the host code, `make asan`); never a CPU fallback --
# that build answers NO_DEVICE on every device path
LIB_PATH = os.environ.get("STARKHIP_LIBRARY") or os.path.join(_HERE, "libstarkhip.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `make` (or __graft_entry__.build()); "
        "starky_bls12_381_amd has no CPU fallback for the prover")

lib = C.CDLL(LIB_PATH)

P = 0xFFFFFFFF00000001
POW_SEARCH = 0xFFFFFFFFFFFFFFFF
N_PHASES = 11
PHASE_NAMES = ["upload", "ifft_lde", "trace_merkle", "quotient", "quotient_commit", "openings", "fri_combine",
               "fri_commit", "pow", "queries", "total"]

AIR_FP12_MUL, AIR_PAIRING_PRECOMP, AIR_MILLER_LOOP, AIR_FINAL_EXP, AIR_ECC_AGGREGATE, AIR_TEST_FIBONACCI = 0, 1, 2, 3, 4, 100
AIR_NAMES = {AIR_FP12_MUL: "FP12MulStark", AIR_PAIRING_PRECOMP: "PairingPrecompStark", AIR_MILLER_LOOP: "MillerLoopStark",
             AIR_FINAL_EXP: "FinalExponentiateStark", AIR_ECC_AGGREGATE: "ECCAggStark", AIR_TEST_FIBONACCI: "TestFibonacci"}
ECC_NUM_POINTS = 512  # src/ecc_aggregate.rs:7
AIR_CUSTOM_BASE, AIR_CUSTOM_CAPACITY = 1024, 4096  # ids of registered AIRs (register_air): BASE, BASE + 1, ...
MAX_LOG_ROWS = 20  # STARKHIP_MAX_LOG_ROWS: a registered AIR's trace has up to 2^20 rows (a built-in AIR's: 8192)

ERR_QUOTIENT_NOT_DIVISIBLE, ERR_ZETA_IN_SUBGROUP, ERR_BAD_SHAPE, ERR_HIP, ERR_OOM, ERR_NO_DEVICE, ERR_VERIFY, ERR_BAD_AIR, ERR_TRACE = range(-1, -10, -1)


class StarkConfig(C.Structure):
    """Mirror of starky::config::StarkConfig + FriConfig (flattened)."""
    _fields_ = [(n, C.c_uint32) for n in ("security_bits", "num_challenges", "rate_bits", "cap_height", "proof_of_work_bits",
                                          "arity_bits", "final_poly_bits", "num_query_rounds")]

    @staticmethod
    def standard_fast_config():
        cfg = StarkConfig()
        lib.starkhip_config_standard_fast(C.byref(cfg))
        return cfg

    @staticmethod
    def for_air(air):
        cfg = StarkConfig()
        _chk(lib.starkhip_config_for_air(air, C.byref(cfg)))
        return cfg


class StarkhipError(RuntimeError):
    def __init__(self, code):
        self.code = code
        super().__init__(f"starkhip error {code}: {lib.starkhip_error_string(code).decode()}")


def _chk(rc):
    if rc != 0:
        raise StarkhipError(rc)


_u64p = C.POINTER(C.c_uint64)
_u32p = C.POINTER(C.c_uint32)
lib.starkhip_error_string.restype = C.c_char_p
lib.starkhip_error_string.argtypes = [C.c_int]
lib.starkhip_config_standard_fast.argtypes = [C.POINTER(StarkConfig)]
lib.starkhip_config_for_air.argtypes = [C.c_int, C.POINTER(StarkConfig)]
for _f in ("columns", "public_inputs", "constraint_degree", "num_constraints", "default_rows"):
    getattr(lib, "starkhip_air_" + _f).argtypes = [C.c_int]
lib.starkhip_air_program.argtypes = [C.c_int, C.POINTER(_u64p), C.POINTER(C.c_size_t)]
lib.starkhip_init.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
lib.starkhip_shutdown.argtypes = [C.c_void_p]
lib.starkhip_shutdown.restype = None
lib.starkhip_prove.argtypes = [C.c_void_p, C.c_int, C.POINTER(StarkConfig), C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _u64p, C.c_size_t,
                               C.c_uint64, C.POINTER(_u64p), C.POINTER(C.c_size_t)]
lib.starkhip_prove_columns.argtypes = [C.c_void_p, C.c_int, C.POINTER(StarkConfig), C.POINTER(C.c_void_p), C.c_size_t, C.c_size_t, _u64p, C.c_size_t,
                                       C.c_uint64, C.POINTER(_u64p), C.POINTER(C.c_size_t)]
lib.starkhip_last_timings.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
lib.starkhip_last_kernel_timings.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
lib.starkhip_last_host_timings.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
lib.starkhip_ntt_long.argtypes = [C.c_void_p, _u64p, C.c_size_t, C.c_uint, C.c_int]
lib.starkhip_lde_batch.argtypes = [C.c_void_p, _u64p, C.c_size_t, C.c_uint, C.c_uint, _u64p, _u64p]
lib.starkhip_merkle_cap.argtypes = [C.c_void_p, _u64p, C.c_size_t, C.c_uint, C.c_uint, _u64p]
lib.starkhip_poseidon_permute_batch.argtypes = [C.c_void_p, _u64p, C.c_size_t]
lib.starkhip_poseidon_permute_batch_form.argtypes = [C.c_void_p, C.c_int, C.c_int, _u64p, C.c_size_t]
lib.starkhip_leaf_hash_lane_group.argtypes = [C.c_void_p, _u64p, C.c_size_t, C.c_size_t, C.c_uint, C.c_uint, C.c_int, C.c_int, C.c_uint, _u64p]
lib.starkhip_leaf_prefix_table.argtypes = [C.c_void_p, C.c_uint, C.c_uint, _u64p]
lib.starkhip_field_ops_batch.argtypes = [C.c_void_p, C.c_int, _u64p, _u64p, _u64p, C.c_size_t]
lib.starkhip_poseidon_permute_host.argtypes = [_u64p]
lib.starkhip_poseidon_permute_host.restype = None
lib.starkhip_verify.argtypes = [C.c_int, C.POINTER(StarkConfig), _u64p, C.c_size_t]
_verify_batch_args = [C.c_size_t, C.POINTER(C.c_int), C.POINTER(StarkConfig), C.POINTER(_u64p), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
lib.starkhip_verify_batch.argtypes = [C.c_void_p] + _verify_batch_args
lib.starkhip_verify_batch_replay.argtypes = _verify_batch_args
lib.starkhip_last_verify_timings.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
lib.starkhip_free.argtypes = [C.c_void_p]
lib.starkhip_free.restype = None
lib.starkhip_host_alloc.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
lib.starkhip_trace_log_begin.argtypes = [C.POINTER(C.c_void_p)]
lib.starkhip_trace_log_end.argtypes = [C.c_void_p]
lib.starkhip_trace_set_threads.argtypes = [C.c_int]
lib.starkhip_trace_log_free.argtypes = [C.c_void_p]
lib.starkhip_trace_log_free.restype = None
lib.starkhip_trace_log_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_size_t)] * 4
lib.starkhip_trace_log_from_writes.argtypes = [C.c_size_t, C.c_size_t, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(C.c_void_p)]
lib.starkhip_lde_bench.argtypes = [C.c_void_p, C.c_size_t, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
lib.starkhip_trace_log_expand_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
lib.starkhip_trace_log_overwrites.argtypes = [C.c_void_p] + [C.POINTER(C.c_size_t)] * 2
lib.starkhip_trace_log_expand_host.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)]
lib.starkhip_prove_compact.argtypes = [C.c_void_p, C.c_int, C.POINTER(StarkConfig), C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t, C.c_uint64,
                                       C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_size_t)]
lib.starkhip_host_free.argtypes = [C.c_void_p]
lib.starkhip_host_free.restype = None
lib.starkhip_trace_fibonacci.argtypes = [C.c_uint64, C.c_uint64, _u64p, C.c_size_t, _u64p]
lib.starkhip_trace_fp12_mul.argtypes = [_u32p, _u32p, _u64p, C.c_size_t, _u64p]
lib.starkhip_trace_final_exp.argtypes = [_u32p, _u64p, C.c_size_t, _u64p]
lib.starkhip_trace_miller_loop.argtypes = [_u32p, _u32p, _u32p, _u32p, _u32p, _u64p, C.c_size_t, _u64p]
lib.starkhip_trace_pairing_precomp.argtypes = [_u32p, _u32p, _u32p, _u64p, C.c_size_t, _u64p]
lib.starkhip_native_fp12_mul.argtypes = [_u32p, _u32p, _u32p]
lib.starkhip_native_final_exponentiate.argtypes = [_u32p, _u32p]
lib.starkhip_native_miller_loop.argtypes = [_u32p, _u32p, _u32p, _u32p, _u32p, _u32p]
lib.starkhip_native_pairing_precomp.argtypes = [_u32p, _u32p, _u32p, _u32p]
_u8p = C.POINTER(C.c_uint8)
HASHER_POSEIDON, HASHER_KECCAK = 0, 1  # STARKHIP_HASHER_*: the "hasher" option of a Prover or a ProofPool, and header word 12 of a proof
LEAF_HASH_FORM_KECCAK = 6  # TicketInfo.leaf_hash_form of a Keccak proof
lib.starkhip_keccak256.argtypes = [C.c_char_p, C.c_size_t, _u8p]
lib.starkhip_keccak256.restype = None
lib.starkhip_keccak_permute_host.argtypes = [_u64p]
lib.starkhip_keccak_permute_host.restype = None
lib.starkhip_keccak_state_from_words.argtypes = [_u64p, C.c_size_t, _u64p]
lib.starkhip_keccak_permute_batch.argtypes = [C.c_void_p, _u64p, C.c_size_t]
lib.starkhip_merkle_tree_hasher.argtypes = [C.c_void_p, C.c_int, _u64p, C.c_size_t, C.c_uint, C.c_uint, _u64p, _u64p]
lib.starkhip_hash_rows_hasher.argtypes = [C.c_void_p, C.c_int, _u64p, C.c_size_t, C.c_size_t, _u64p]
lib.starkhip_proof_hasher.argtypes = [_u64p, C.c_size_t]
lib.starkhip_trace_ecc_aggregate.argtypes = [_u32p, _u8p, _u64p, C.c_size_t, _u64p]
lib.starkhip_native_g1_aggregate.argtypes = [_u32p, _u8p, _u32p]


def _p64(a):
    return a.ctypes.data_as(_u64p)


def _p32(a):
    return a.ctypes.data_as(_u32p)


def _limbs(x, n):
    a = np.ascontiguousarray(x, dtype=np.uint32).reshape(-1)
    assert a.size == n, (a.size, n)
    return a


# ----------------------------------------------------------------------------- AIR metadata
def air_columns(air):
    r = lib.starkhip_air_columns(air)
    if r < 0:
        raise StarkhipError(r)
    return r


def air_public_inputs(air):
    r = lib.starkhip_air_public_inputs(air)
    if r < 0:
        raise StarkhipError(r)
    return r


def air_constraint_degree(air):
    r = lib.starkhip_air_constraint_degree(air)
    if r < 0:
        raise StarkhipError(r)
    return r


def air_num_constraints(air):
    r = lib.starkhip_air_num_constraints(air)
    if r < 0:
        raise StarkhipError(r)
    return r


def air_default_rows(air):
    r = lib.starkhip_air_default_rows(air)
    if r < 0:
        raise StarkhipError(r)
    return r


def air_permutation_pairs(air):
    """Permutation pairs the AIR declares (starky's permutation_pairs(); 0 for every built-in AIR)."""
    r = lib.starkhip_air_permutation_pairs(air)
    if r < 0:
        raise StarkhipError(r)
    return r


def air_permutation_zs(air):
    """nZ: the Z polynomials a proof of the AIR commits for its permutation pairs, 2 per batch of max(1, degree - 1) pairs."""
    r = lib.starkhip_air_permutation_zs(air)
    if r < 0:
        raise StarkhipError(r)
    return r


def air_logups(air):
    """LogUp lookups the AIR declares (AirBuilder.logup; 0 for every built-in AIR)."""
    r = lib.starkhip_air_logups(air)
    if r < 0:
        raise StarkhipError(r)
    return r


def air_logup_columns(air):
    """The looked-up columns of all LogUp lookups of the AIR together (starkhip_air_logup_columns): the length of a LogupReport's per_column."""
    r = lib.starkhip_air_logup_columns(air)
    if r < 0:
        raise StarkhipError(r)
    return r


def air_logup_polys(air):
    """nA: the auxiliary polynomials a proof of the AIR commits for its LogUp lookups: per challenge (2) and lookup its
    ceil(m / (degree - 1)) helpers and one running sum."""
    r = lib.starkhip_air_logup_polys(air)
    if r < 0:
        raise StarkhipError(r)
    return r


def air_logup_general(air):
    """starkhip_air_logup_general: 1 when some LogUp lookup of the AIR is over Column combinations or has a filter (the general kernels
    run), 0 when all are plain."""
    r = lib.starkhip_air_logup_general(air)
    if r < 0:
        raise StarkhipError(r)
    return r


def air_program(air):
    """Serialised constraint program (numpy uint64 copy)."""
    blob = _u64p()
    words = C.c_size_t()
    _chk(lib.starkhip_air_program(air, C.byref(blob), C.byref(words)))
    return np.ctypeslib.as_array(blob, shape=(words.value,)).copy()


lib.starkhip_air_check_program.argtypes = [_u64p, C.c_size_t, C.c_char_p, C.c_size_t]
lib.starkhip_air_register.argtypes = [_u64p, C.c_size_t, C.c_char_p, C.c_uint32, C.POINTER(C.c_int)]
lib.starkhip_check_trace.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _u64p, _u64p, _u64p]
CHECK_LIST_MAX = 1 << 20  # STARKHIP_CHECK_LIST_MAX


class _CheckReportStruct(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("violations", "constraints_violated", "rows_violated", "listed")]


_u32p = C.POINTER(C.c_uint32)
lib.starkhip_check_trace_report.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _u64p, _u32p, _u64p, _u64p,
                                            C.c_size_t, C.POINTER(_CheckReportStruct)]
lib.starkhip_check_trace_report_replay.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, _u64p, _u32p, _u64p, _u64p, C.c_size_t,
                                                   C.POINTER(_CheckReportStruct)]


class CheckReport:
    """What starkhip_check_trace_report found.  `violations`: (row, constraint) pairs with a nonzero value (check_trace's number);
    `constraints_violated`, `rows_violated`; `per_constraint` (np.uint32[K]): rows on which each constraint is violated; `row_mask`
    (np.uint64[(n + 63) // 64]): bit r & 63 of word r >> 6; `rows`: the violated rows, ascending; `list` (np.uint64[listed, 3]): the
    first min(cap, violations) violations as (constraint, row, value), by constraint, then row."""

    def __init__(self, summary, per_constraint, row_mask, entries):
        self.violations, self.constraints_violated, self.rows_violated = (int(summary.violations), int(summary.constraints_violated),
                                                                          int(summary.rows_violated))
        self.per_constraint, self.row_mask = per_constraint, row_mask
        self.rows = np.flatnonzero(np.unpackbits(row_mask.view(np.uint8), bitorder="little"))
        self.list = entries[:int(summary.listed)].copy()

    def __repr__(self):
        return (f"CheckReport(violations={self.violations}, constraints_violated={self.constraints_violated}, "
                f"rows_violated={self.rows_violated}, listed={len(self.list)})")


def _check_trace_report(call, air, n_rows, cap):
    """`call(per_constraint, row_mask, list, cap, summary)` -> rc: one of the two report entry points with its leading arguments bound."""
    cap = int(cap)
    if cap < 0:
        raise StarkhipError(ERR_BAD_SHAPE)
    per = np.zeros(air_num_constraints(air), dtype=np.uint32)
    mask = np.zeros((n_rows + 63) // 64, dtype=np.uint64)
    entries = np.zeros((min(cap, CHECK_LIST_MAX), 3), dtype=np.uint64)  # a larger cap is the library's to refuse
    summary = _CheckReportStruct()
    _chk(call(per.ctypes.data_as(_u32p), _p64(mask), _p64(entries) if cap else None, cap, C.byref(summary)))
    return CheckReport(summary, per, mask, entries)


CHECK_MAGIC = 0x3130304B48435353  # STARKHIP_CHECK_MAGIC, "SSCHK001"
lib.starkhip_check_blob_layout.argtypes = [_u64p, C.c_size_t, C.POINTER(_CheckReportStruct), C.POINTER(_u64p)]
lib.starkhip_check_blob_replay.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, _u64p, C.c_size_t, C.POINTER(_u64p), C.POINTER(C.c_size_t)]
lib.starkhip_check_stats.argtypes = [C.c_void_p, _u64p]
lib.starkhip_pool_check_stats.argtypes = [C.c_void_p, _u64p]


class CheckBlobReport(CheckReport):
    """A check blob read (parse_check_blob): a CheckReport with the summary -- `violations`, `constraints_violated`, `rows_violated` --
    and `list` (np.uint64[listed, 3]): the first "check_trace_list" violations as (constraint, row, value), by constraint, then row;
    with the blob's `air` and `n_rows`.  The per-constraint counts and the row mask are not in a blob: `per_constraint`, `row_mask`
    and `rows` are None."""

    def __init__(self, air, n_rows, summary, entries):
        self.air, self.n_rows = int(air), int(n_rows)
        self.per_constraint = self.row_mask = self.rows = None
        self.violations, self.constraints_violated, self.rows_violated = (int(summary.violations), int(summary.constraints_violated),
                                                                          int(summary.rows_violated))
        self.list = entries

    def __repr__(self):
        return (f"CheckBlobReport(air={self.air}, n_rows={self.n_rows}, violations={self.violations}, "
                f"constraints_violated={self.constraints_violated}, rows_violated={self.rows_violated}, listed={len(self.list)})")


def parse_check_blob(blob):
    """starkhip_check_blob_layout on a check blob (np.uint64): its CheckBlobReport; StarkhipError(ERR_BAD_SHAPE) for anything else."""
    b = np.ascontiguousarray(blob, dtype=np.uint64).reshape(-1)
    summary = _CheckReportStruct()
    lst = _u64p()
    _chk(lib.starkhip_check_blob_layout(_p64(b), b.size, C.byref(summary), C.byref(lst)))
    listed = int(summary.listed)
    entries = b[8:8 + 3 * listed].reshape(listed, 3).copy()
    return CheckBlobReport(b[1], b[2], summary, entries)


LOOKUP_MAGIC = 0x313030504B4C5353
LOGUP_MAGIC = 0x31303055474C5353  # STARKHIP_LOGUP_MAGIC


class TraceViolation(StarkhipError):
    """ERR_TRACE from a prove with "check_trace" on, or from a pool with "check_traces": the trace violates the AIR.  `.blob` is the
    check blob (np.uint64) and `.report` its CheckBlobReport.  From a prove or a pool with "fill_lookups" for a trace some lookup of
    which fails: `.blob` is the lookup blob, `.lookup_report` its LookupBlobReport and `.report` is None (else `.lookup_report` is).
    With "fill_frequencies" for a trace some LogUp lookup of which fails: `.blob` is the LogUp blob and `.logup_report` its
    LogupBlobReport (None otherwise)."""

    def __init__(self, blob):
        super().__init__(ERR_TRACE)
        self.blob = blob
        self.report = self.lookup_report = self.logup_report = None
        if len(blob) and int(blob[0]) == LOOKUP_MAGIC:
            self.lookup_report = parse_lookup_blob(blob)
        elif len(blob) and int(blob[0]) == LOGUP_MAGIC:
            self.logup_report = parse_logup_blob(blob)
        else:
            self.report = parse_check_blob(blob)


def _take_blob(rc, out, words, keep=True):
    """The result of a proving call: the proof as a numpy copy (None unless `keep`), the library's blob freed; TraceViolation with the
    check blob for ERR_TRACE, StarkhipError for every other failure."""
    if rc == ERR_TRACE and out:
        blob = np.ctypeslib.as_array(out, shape=(words.value,)).copy()
        lib.starkhip_free(out)
        raise TraceViolation(blob)
    _chk(rc)
    proof = np.ctypeslib.as_array(out, shape=(words.value,)).copy() if keep else None
    lib.starkhip_free(out)
    return proof


def check_blob_replay(air, trace, public_inputs, layout=0, cap=16):
    """starkhip_check_blob_replay (tests, small shapes): the check blob a checking prove must hand back for `trace` with
    "check_trace_list" = cap, or None for a satisfying trace; no device needed."""
    trace = np.ascontiguousarray(trace, dtype=np.uint64)
    if trace.ndim != 2 or layout not in (0, 1) or int(cap) < 0:
        raise StarkhipError(ERR_BAD_SHAPE)
    n_rows, n_cols = trace.shape if layout == 0 else trace.shape[::-1]
    pis = np.ascontiguousarray(public_inputs, dtype=np.uint64)
    if pis.size != air_public_inputs(air):
        raise StarkhipError(ERR_BAD_SHAPE)
    out = _u64p()
    words = C.c_size_t()
    rc = lib.starkhip_check_blob_replay(air, trace.ctypes.data_as(C.c_void_p), n_rows, n_cols, layout, _p64(pis), int(cap), C.byref(out),
                                        C.byref(words))
    if rc == 0:
        return None
    if rc != ERR_TRACE:
        raise StarkhipError(rc)
    blob = np.ctypeslib.as_array(out, shape=(words.value,)).copy()
    lib.starkhip_free(out)
    return blob


class _FreeCellsStruct(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("cells", "free_cells", "free_columns", "partly_free_columns")]


lib.starkhip_check_trace_free_cells.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _u64p, C.c_uint64, _u32p,
                                                _u64p, C.POINTER(_FreeCellsStruct)]
lib.starkhip_check_trace_free_cells_replay.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, _u64p, C.c_uint64, _u32p, _u64p,
                                                       C.POINTER(_FreeCellsStruct)]
# The delta free_cells adds when the caller names none: fixed, so that a result can be reproduced.  A constrained cell reads as free
# for at most `degree` values of delta per (constraint, cell) pair: a real audit should pass a random one, 1 <= delta < P.
DEFAULT_DELTA = 0x9E3779B97F4A7C15


class FreeCells:
    """What starkhip_check_trace_free_cells found: the cells of a trace that no constraint notices when delta is added to them, one
    at a time.  `cells` = rows x columns, `free` of them free; `free_columns`: columns with every row free (no constraint reads
    them, or none that applies), `partly_free_columns`: some rows; `per_column` (np.uint32[C]): the free rows of each column; `mask`
    (bool[n, C], or None when it was not asked for): mask[r, c] is True when cell (r, c) is free; `mask_words` (np.uint64[C, (n + 63)
    // 64], or None): the same as the library wrote it, bit r & 63 of word r >> 6 of column c.  A necessary test, not a sufficient
    one: it does not see a cheat that changes several cells together."""

    def __init__(self, summary, per_column, words, n_rows):
        self.cells, self.free = int(summary.cells), int(summary.free_cells)
        self.free_columns, self.partly_free_columns = int(summary.free_columns), int(summary.partly_free_columns)
        self.per_column, self.mask_words = per_column, words
        self._n_rows, self._mask = n_rows, None

    @property
    def mask(self):  # unpacked on first use: eight times the words, 600 MB for FinalExp
        if self._mask is None and self.mask_words is not None:
            bits = np.unpackbits(self.mask_words.view(np.uint8).reshape(self.mask_words.shape[0], -1), axis=1, bitorder="little")
            self._mask = np.ascontiguousarray(bits[:, :self._n_rows].T).astype(bool)
        return self._mask

    def __repr__(self):
        return (f"FreeCells(cells={self.cells}, free={self.free}, free_columns={self.free_columns}, "
                f"partly_free_columns={self.partly_free_columns})")


def _free_cells(call, n_rows, n_cols, mask):
    """`call(per_column, free_mask, summary)` -> rc: one of the two free-cell entry points with its leading arguments bound."""
    per = np.zeros(n_cols, dtype=np.uint32)
    words = np.zeros((n_cols, (n_rows + 63) // 64), dtype=np.uint64) if mask else None
    summary = _FreeCellsStruct()
    _chk(call(per.ctypes.data_as(_u32p), _p64(words) if mask else None, C.byref(summary)))
    return FreeCells(summary, per, words, n_rows)


def _free_cells_args(air, public_inputs, delta):
    pis = np.ascontiguousarray(public_inputs, dtype=np.uint64)
    delta = int(delta)
    if pis.size != air_public_inputs(air) or not 0 <= delta < 1 << 64:
        raise StarkhipError(ERR_BAD_SHAPE)
    return pis, delta


class _FreeCellClassesStruct(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("cells", "caught", "silent", "gated", "unread", "silent_columns", "constraints_never_open")]


lib.starkhip_check_trace_free_cell_classes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _u64p, C.c_uint64,
                                                       _u32p, _u64p, _u32p, C.POINTER(_FreeCellClassesStruct)]
lib.starkhip_check_trace_free_cell_classes_replay.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, _u64p, C.c_uint64, _u32p, _u64p,
                                                              _u32p, C.POINTER(_FreeCellClassesStruct)]
_POPCOUNT8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint32)


def _plane_rows(words):
    """Set bits per column of uint64 words [C, W]."""
    return _POPCOUNT8[words.view(np.uint8)].reshape(words.shape[0], -1).sum(axis=1, dtype=np.uint32)


class FreeCellClasses:
    """What starkhip_check_trace_free_cell_classes found: FreeCells' free cells told apart.  A cell is unread when no constraint that
    applies reads it, gated when every constraint that reads it has a zero gate product there, silent when one reads it with its gates
    open and still does not notice delta added to it -- where a missing constraint hides -- and caught otherwise.  The summary:
    `cells` = `n_caught` + `n_silent` + `n_gated` + `n_unread`, `silent_columns` (columns holding a silent cell) and
    `constraints_never_open`; `per_column` (np.uint32[C, 3]): the silent, gated and unread rows of each column; `open_rows`
    (np.uint32[K]): per constraint, the rows of the unchanged trace on which its gates were open.  `plane_words` (np.uint64[3, C,
    (n + 63) // 64], or None when the planes were not asked for): the cumulative bitmaps read, open, caught as the library wrote
    them; `read`, `open`, `caught` (bool[n, C], None without planes) unpack them, and `silent` = open & ~caught, `gated` = read & ~open,
    `unread` = ~read.  The limits are FreeCells': one cell at a time, probabilistic in delta."""

    def __init__(self, summary, per_column, plane_words, open_rows, n_rows):
        self.cells, self.n_caught, self.n_silent = int(summary.cells), int(summary.caught), int(summary.silent)
        self.n_gated, self.n_unread = int(summary.gated), int(summary.unread)
        self.silent_columns, self.constraints_never_open = int(summary.silent_columns), int(summary.constraints_never_open)
        self.per_column, self.plane_words, self.open_rows = per_column, plane_words, open_rows
        self._n_rows, self._planes = n_rows, None

    def _plane(self, i):  # unpacked on first use: eight times the words
        if self.plane_words is None:
            return None
        if self._planes is None:
            w = self.plane_words
            bits = np.unpackbits(w.view(np.uint8).reshape(3, w.shape[1], -1), axis=2, bitorder="little")
            self._planes = np.ascontiguousarray(bits[:, :, :self._n_rows].transpose(0, 2, 1)).astype(bool)
        return self._planes[i]

    read = property(lambda self: self._plane(0))
    open = property(lambda self: self._plane(1))
    caught = property(lambda self: self._plane(2))
    silent = property(lambda self: None if self.plane_words is None else self._plane(1) & ~self._plane(2))
    gated = property(lambda self: None if self.plane_words is None else self._plane(0) & ~self._plane(1))
    unread = property(lambda self: None if self.plane_words is None else ~self._plane(0))

    def merge(self, other):
        """The audit of both traces (one AIR, one shape): the OR of the planes.  Summary and per_column are recomputed from the merged
        planes, open_rows are added.  Both results need their planes."""
        a, b = self.plane_words, other.plane_words
        if a is None or b is None or a.shape != b.shape or self._n_rows != other._n_rows or self.open_rows.shape != other.open_rows.shape:
            raise StarkhipError(ERR_BAD_SHAPE)
        words = a | b
        per = np.stack([_plane_rows(words[1] & ~words[2]), _plane_rows(words[0] & ~words[1]),
                        np.uint32(self._n_rows) - _plane_rows(words[0])], axis=1).astype(np.uint32)
        open_rows = self.open_rows + other.open_rows
        summary = _FreeCellClassesStruct(self.cells, int(_plane_rows(words[2]).sum()), int(per[:, 0].sum()), int(per[:, 1].sum()),
                                         int(per[:, 2].sum()), int((per[:, 0] != 0).sum()), int((open_rows == 0).sum()))
        return FreeCellClasses(summary, per, words, open_rows, self._n_rows)

    def __repr__(self):
        return (f"FreeCellClasses(cells={self.cells}, caught={self.n_caught}, silent={self.n_silent}, gated={self.n_gated}, "
                f"unread={self.n_unread}, silent_columns={self.silent_columns}, constraints_never_open={self.constraints_never_open})")


def _free_cell_classes(call, air, n_rows, n_cols, planes):
    """`call(per_column, planes, open_rows, summary)` -> rc: one of the two entry points with its leading arguments bound."""
    per = np.zeros((n_cols, 3), dtype=np.uint32)
    words = np.zeros((3, n_cols, (n_rows + 63) // 64), dtype=np.uint64) if planes else None
    open_rows = np.zeros(air_num_constraints(air), dtype=np.uint32)
    summary = _FreeCellClassesStruct()
    _chk(call(per.ctypes.data_as(_u32p), _p64(words) if planes else None, open_rows.ctypes.data_as(_u32p), C.byref(summary)))
    return FreeCellClasses(summary, per, words, open_rows, n_rows)


def air_check_program(blob):
    """The validator starkhip_air_register runs: None for a program it accepts, else the reason it refuses it."""
    blob = np.ascontiguousarray(blob, dtype=np.uint64)
    why = C.create_string_buffer(512)
    rc = lib.starkhip_air_check_program(_p64(blob), blob.size, why, len(why))
    if rc == 0:
        return None
    if rc != ERR_BAD_AIR:
        raise StarkhipError(rc)
    return why.value.decode()


def register_air(blob, name=None, default_rows=0, lookups=None):
    """Register a constraint program (csrc/air_ir.h format; air_builder.AirBuilder makes one) and return its AIR id, usable wherever a
    built-in id is.  The same blob again returns the same id.  A program the validator refuses raises StarkhipError(ERR_BAD_AIR).
    default_rows: 0, or a power of two in 2 .. 2^MAX_LOG_ROWS (anything else: ERR_BAD_SHAPE).
    lookups: [(input, table, permuted_input, permuted_table), ...] (AirBuilder.lookups) registers the program together with its lookups
    (starkhip_air_register_lookups): a prover or pool with "fill_lookups" then fills their permuted columns itself.  The id is that of
    (blob, lookups); the same blob without a list keeps an id of its own.  A list air_check_lookups refuses: ERR_BAD_AIR."""
    blob = np.ascontiguousarray(blob, dtype=np.uint64)
    out = C.c_int()
    cname = name.encode() if name is not None else None
    if lookups is None:
        _chk(lib.starkhip_air_register(_p64(blob), blob.size, cname, default_rows, C.byref(out)))
    else:
        arr, nl = _lookup_array(lookups)
        _chk(lib.starkhip_air_register_lookups(_p64(blob), blob.size, cname, default_rows, arr, nl, C.byref(out)))
    return out.value


def air_check_lookups(blob, lookups):
    """The validator of register_air(lookups=...) (starkhip_air_check_lookups): None for a list it accepts for this program, else the reason."""
    blob = np.ascontiguousarray(blob, dtype=np.uint64)
    arr, nl = _lookup_array(lookups)
    why = C.create_string_buffer(512)
    rc = lib.starkhip_air_check_lookups(_p64(blob), blob.size, arr, nl, why, len(why))
    if rc == 0:
        return None
    if rc != ERR_BAD_AIR:
        raise StarkhipError(rc)
    return why.value.decode()


def air_lookups(air):
    """The lookups `air` was registered with, [(input, table, permuted_input, permuted_table), ...]; [] for a built-in AIR or a plain registration."""
    n = lib.starkhip_air_lookups(air, None, 0)
    arr = (_LookupStruct * max(1, n))()
    lib.starkhip_air_lookups(air, arr, n)
    return [(a.input, a.table, a.permuted_input, a.permuted_table) for a in arr[:n]]


lib.starkhip_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
lib.starkhip_quotient_plan_check.argtypes = [C.c_int, C.c_uint, C.c_uint64, _u64p]


class ProofLayout(C.Structure):
    """starkhip_proof_layout_t: word offsets of every field of a proof blob."""
    _fields_ = [(n, C.c_size_t) for n in (
        "n_columns", "n_quotient_polys", "degree_bits", "rate_bits", "cap_height", "n_fri_layers", "n_query_rounds", "final_poly_len",
        "n_public_inputs", "arity_bits", "off_trace_cap", "off_quotient_cap", "off_local_values", "off_next_values",
        "off_quotient_openings", "off_fri_caps", "off_query_rounds", "query_round_words", "off_final_poly", "off_pow_witness",
        "off_public_inputs", "total_words", "q_trace_leaf", "q_trace_siblings", "q_quotient_leaf", "q_quotient_siblings",
        "initial_sibling_count")] + [(n, C.c_size_t * 16) for n in ("q_step_evals", "q_step_siblings", "step_sibling_count")] + \
        [(n, C.c_size_t) for n in ("n_permutation_zs", "off_permutation_zs_cap", "off_permutation_zs", "off_permutation_zs_next",
                                   "q_permutation_zs_leaf", "q_permutation_zs_siblings", "n_logup_polys", "n_ctl_polys", "off_ctl_sums")]


lib.starkhip_proof_layout.argtypes = [_u64p, C.c_size_t, C.POINTER(ProofLayout)]


def proof_layout(proof):
    """Offsets of the fields of a proof blob (starkhip_proof_layout)."""
    proof = np.ascontiguousarray(proof, dtype=np.uint64)
    out = ProofLayout()
    _chk(lib.starkhip_proof_layout(_p64(proof), proof.size, C.byref(out)))
    return out


lib.starkhip_fri_geometry.argtypes = [C.POINTER(StarkConfig), C.c_uint, C.POINTER(C.c_uint), C.c_size_t, C.POINTER(C.c_size_t),
                                      C.POINTER(C.c_size_t)]


def fri_geometry(config, log_n):
    """starkhip_fri_geometry: (FRI reduction arity bits, final polynomial length) of `config` at 2^log_n rows -- the config rule of
    every prove and verify entry point.  A refused config raises StarkhipError(ERR_BAD_SHAPE)."""
    ar = (C.c_uint * 16)()
    n_layers, final_len = C.c_size_t(), C.c_size_t()
    _chk(lib.starkhip_fri_geometry(C.byref(config), log_n, ar, 16, C.byref(n_layers), C.byref(final_len)))
    return [int(a) for a in ar[:n_layers.value]], final_len.value


def quotient_plan_check(air, want_chunks=4, seed=1):
    """CPU replay of the tiled constraint plan against the plain fold; returns the plan statistics (see starkhip.h)."""
    stats = np.zeros(8, dtype=np.uint64)
    _chk(lib.starkhip_quotient_plan_check(air, want_chunks, seed, _p64(stats)))
    return dict(zip(("chunks", "supergroups", "pieces", "records", "lds_cell_records", "direct_loads", "tiles", "contributions"),
                    (int(x) for x in stats)))


lib.starkhip_quotient_classes.argtypes = [C.c_int, C.POINTER(C.c_uint8), C.c_size_t]
lib.starkhip_quotient_solve_table.argtypes = [C.c_uint, C.c_uint, _u64p, C.c_size_t]
lib.starkhip_quotient_class_plan_check.argtypes = [C.c_int, C.c_uint, C.c_uint64, _u64p]


def quotient_classes(air):
    """The class of every constraint: on how many cosets of n points the quotient evaluates it (starkhip_quotient_classes)."""
    out = np.zeros(air_num_constraints(air), dtype=np.uint8)
    _chk(lib.starkhip_quotient_classes(air, out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size))
    return out


def quotient_solve_table(log_rows, quotient_degree_bits):
    """(ginv[8], cpow[8][8], vinv[9][8][8]): the constants of the classes' recombination (starkhip_quotient_solve_table)."""
    out = np.zeros(8 + 64 + 9 * 64, dtype=np.uint64)
    _chk(lib.starkhip_quotient_solve_table(log_rows, quotient_degree_bits, _p64(out), out.size))
    return out[:8], out[8:72].reshape(8, 8), out[72:].reshape(9, 8, 8)


def quotient_class_plan_check(air, want_chunks=4, seed=1):
    """CPU replay of the per-class plans against the plain fold restricted to each class (starkhip_quotient_class_plan_check)."""
    st = np.zeros(32, dtype=np.uint64)
    _chk(lib.starkhip_quotient_class_plan_check(air, want_chunks, seed, _p64(st)))
    st = [int(x) for x in st]
    k, t = st[0], st[1]
    return {"classes": k, "cosets": t, "chunks": st[2], "work_rows": st[3], "records": st[4], "piece_ends": st[5], "tile_phases": st[6],
            "contributions": st[7], "class_constraints": st[8:8 + k], "coset_chunks": st[24:24 + t]}


lib.starkhip_air_eval_frame.argtypes = [C.c_int, _u64p, _u64p, _u64p, _u64p, _u64p, C.c_int, _u64p]


def air_eval_frame(air, local, nxt, pis, masks, alphas):
    """The ConstraintConsumer accumulators after one `eval_packed_generic` on an arbitrary frame over the quadratic
    extension (host evaluator of the verifier).  local / nxt: [columns, 2], masks: [4, 2], alphas: [k, 2] -> [k, 2]."""
    local, nxt, masks, alphas = (np.ascontiguousarray(x, dtype=np.uint64) for x in (local, nxt, masks, alphas))
    pis = np.ascontiguousarray(pis, dtype=np.uint64)
    cols = air_columns(air)
    if local.shape != (cols, 2) or nxt.shape != (cols, 2) or masks.shape != (4, 2) or alphas.ndim != 2 or alphas.shape[1] != 2 \
            or pis.size != air_public_inputs(air):
        raise StarkhipError(ERR_BAD_SHAPE)
    out = np.zeros_like(alphas)
    _chk(lib.starkhip_air_eval_frame(air, _p64(local), _p64(nxt), _p64(pis), _p64(masks), _p64(alphas), alphas.shape[0], _p64(out)))
    return out


lib.starkhip_air_eval_frame_full.argtypes = [C.c_int, _u64p, _u64p, _u64p, _u64p, _u64p, C.c_int, _u64p, _u64p, _u64p, _u64p]


def air_eval_frame_full(air, local, nxt, pis, masks, alphas, zs, zs_next, challenges):
    """air_eval_frame continued over the permutation constraints (COMPAT.md P4): zs / zs_next [nZ, 2] are the Z openings at zeta and
    g zeta, challenges the B x 2 x (beta, gamma) base-field words; the fold over all K + 2 nZ constraints, [k, 2]."""
    local, nxt, masks, alphas, zs, zs_next = (np.ascontiguousarray(x, dtype=np.uint64) for x in (local, nxt, masks, alphas, zs, zs_next))
    pis = np.ascontiguousarray(pis, dtype=np.uint64)
    challenges = np.ascontiguousarray(challenges, dtype=np.uint64).reshape(-1)
    cols, nz = air_columns(air), air_permutation_zs(air)
    if local.shape != (cols, 2) or nxt.shape != (cols, 2) or masks.shape != (4, 2) or alphas.ndim != 2 or alphas.shape[1] != 2 \
            or pis.size != air_public_inputs(air) or zs.shape != (nz, 2) or zs_next.shape != (nz, 2) \
            or challenges.size != 4 * max(1, air_constraint_degree(air) - 1):
        raise StarkhipError(ERR_BAD_SHAPE)
    out = np.zeros_like(alphas)
    _chk(lib.starkhip_air_eval_frame_full(air, _p64(local), _p64(nxt), _p64(pis), _p64(masks), _p64(alphas), alphas.shape[0], _p64(zs),
                                          _p64(zs_next), _p64(challenges), _p64(out)))
    return out


lib.starkhip_air_eval_frame_logup.argtypes = [C.c_int, _u64p, _u64p, _u64p, _u64p, _u64p, C.c_int, _u64p, _u64p, _u64p, _u64p]


def air_eval_frame_logup(air, local, nxt, pis, masks, alphas, aux, aux_next, challenges):
    """air_eval_frame continued over the LogUp constraints (COMPAT.md L4): aux / aux_next [nA, 2] are the auxiliary openings at zeta
    and g zeta, challenges the two base-field words chi_0, chi_1; the fold over all K + nL constraints, [k, 2]."""
    local, nxt, masks, alphas, aux, aux_next = (np.ascontiguousarray(x, dtype=np.uint64) for x in (local, nxt, masks, alphas, aux, aux_next))
    pis = np.ascontiguousarray(pis, dtype=np.uint64)
    challenges = np.ascontiguousarray(challenges, dtype=np.uint64).reshape(-1)
    cols, na = air_columns(air), air_logup_polys(air)
    if local.shape != (cols, 2) or nxt.shape != (cols, 2) or masks.shape != (4, 2) or alphas.ndim != 2 or alphas.shape[1] != 2 \
            or pis.size != air_public_inputs(air) or aux.shape != (na, 2) or aux_next.shape != (na, 2) or challenges.size != 2:
        raise StarkhipError(ERR_BAD_SHAPE)
    out = np.zeros_like(alphas)
    _chk(lib.starkhip_air_eval_frame_logup(air, _p64(local), _p64(nxt), _p64(pis), _p64(masks), _p64(alphas), alphas.shape[0], _p64(aux),
                                           _p64(aux_next), _p64(challenges), _p64(out)))
    return out


lib.starkhip_logup_polys.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _u64p, _u64p, _u64p, _u64p]
lib.starkhip_logup_polys_replay.argtypes = [C.c_int, _u64p, C.c_size_t, C.c_size_t, C.c_int, _u64p, _u64p, _u64p, _u64p]


def _logup_args(air, n_rows, challenges):
    challenges = np.ascontiguousarray(challenges, dtype=np.uint64).reshape(-1)
    if challenges.size != 2:
        raise StarkhipError(ERR_BAD_SHAPE)
    return (challenges, np.zeros((air_logup_polys(air), n_rows), dtype=np.uint64), np.zeros((2, air_logups(air)), dtype=np.uint64),
            np.zeros(1, dtype=np.uint64))


def logup_polys_replay(air, trace, challenges, layout=0):
    """The auxiliary polynomials of `trace` (row-major [n][C], or column-major [C][n] with layout=1) under the challenges (chi_0, chi_1),
    from plain loops on the host (starkhip_logup_polys_replay): (polys [nA, n], closing values [2, n_lookups], zero denominators)."""
    trace = np.ascontiguousarray(trace, dtype=np.uint64)
    if trace.ndim != 2 or layout not in (0, 1):
        raise StarkhipError(ERR_BAD_SHAPE)
    n_rows, n_cols = trace.shape if layout == 0 else trace.shape[::-1]
    challenges, polys, closing, zeros = _logup_args(air, n_rows, challenges)
    _chk(lib.starkhip_logup_polys_replay(air, _p64(trace), n_rows, n_cols, layout, _p64(challenges), _p64(polys), _p64(closing), _p64(zeros)))
    return polys, closing, int(zeros[0])


lib.starkhip_permutation_zs.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _u64p, _u64p, _u64p]
lib.starkhip_permutation_zs_replay.argtypes = [C.c_int, _u64p, C.c_size_t, C.c_size_t, C.c_int, _u64p, _u64p, _u64p]


def _perm_zs_args(air, n_rows, challenges):
    challenges = np.ascontiguousarray(challenges, dtype=np.uint64).reshape(-1)
    if challenges.size != 4 * max(1, air_constraint_degree(air) - 1):
        raise StarkhipError(ERR_BAD_SHAPE)
    nz = air_permutation_zs(air)
    return challenges, np.zeros((nz, n_rows), dtype=np.uint64), np.zeros(nz, dtype=np.uint64)


def permutation_zs_replay(air, trace, challenges, layout=0):
    """The Z polynomials of `trace` (row-major [n][C], or column-major [C][n] with layout=1) under `challenges` (B x 2 x (beta, gamma)),
    from plain loops on the host (starkhip_permutation_zs_replay): (zs [nZ, n], closing products [nZ])."""
    trace = np.ascontiguousarray(trace, dtype=np.uint64)
    if trace.ndim != 2 or layout not in (0, 1):
        raise StarkhipError(ERR_BAD_SHAPE)
    n_rows, n_cols = trace.shape if layout == 0 else trace.shape[::-1]
    challenges, zs, closing = _perm_zs_args(air, n_rows, challenges)
    _chk(lib.starkhip_permutation_zs_replay(air, _p64(trace), n_rows, n_cols, layout, _p64(challenges), _p64(zs), _p64(closing)))
    return zs, closing


PERM_CHECK_ATTEMPTS = 4  # STARKHIP_PERM_CHECK_ATTEMPTS
PERM_UNDECIDED = 0xFFFFFFFF  # per_pair of a pair whose keys collided under every attempt seed


class _PermCheckStruct(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("pairs", "pairs_violated", "pairs_undecided", "unmatched", "listed", "reseeds")]


lib.starkhip_check_trace_permutations.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_uint64, _u32p, _u64p,
                                                  _u64p, C.c_size_t, C.POINTER(_PermCheckStruct)]
lib.starkhip_check_trace_permutations_replay.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_uint64, _u32p, _u64p, _u64p,
                                                         C.c_size_t, C.POINTER(_PermCheckStruct)]
lib.starkhip_perm_check_seeds.argtypes = [C.c_uint64, _u64p]
lib.starkhip_perm_check_timings.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
# The seed of the sort keys when the caller names none: fixed, so that a run can be reproduced.  The result does not depend on it except
# for pairs reported undecided; a real audit should pass a random one, 2 <= seed < P.
DEFAULT_SEED = 0x9E3779B97F4A7C15


def perm_check_seeds(seed=DEFAULT_SEED):
    """The seeds check_trace_permutations tries for `seed`, in order (starkhip_perm_check_seeds): a list of PERM_CHECK_ATTEMPTS ints."""
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise StarkhipError(ERR_BAD_SHAPE)
    out = np.zeros(PERM_CHECK_ATTEMPTS, dtype=np.uint64)
    _chk(lib.starkhip_perm_check_seeds(seed, _p64(out)))
    return [int(x) for x in out]


class PermutationCheck:
    """What starkhip_check_trace_permutations found, pair by pair of the AIR: `pairs`, `pairs_violated`, `pairs_undecided`; `unmatched`:
    the flagged rows over all decided pairs, both sides; `reseeds`: reruns of a pair because two different tuples shared a sort key;
    `per_pair` (np.uint32[n_pairs]): the unmatched rows per side, PERM_UNDECIDED for an undecided pair; `masks` (bool[n_pairs, 2, n]):
    masks[q, side, r] is True when row r of pair q's lhs (side 0) or rhs (side 1) has no partner; `mask_words` (np.uint64[n_pairs, 2,
    (n + 63) // 64]): the same as the library wrote it; `list` (np.uint64[listed, 3]): the first min(cap, unmatched) flagged rows as
    (pair, side, row), by pair, side (lhs first), row."""

    def __init__(self, summary, per_pair, words, entries, n_rows):
        self.pairs, self.pairs_violated, self.pairs_undecided = int(summary.pairs), int(summary.pairs_violated), int(summary.pairs_undecided)
        self.unmatched, self.reseeds = int(summary.unmatched), int(summary.reseeds)
        self.per_pair, self.mask_words = per_pair, words
        self.list = entries[:int(summary.listed)].copy()
        self._n_rows, self._masks = n_rows, None

    @property
    def masks(self):  # unpacked on first use: eight times the words
        if self._masks is None:
            bits = np.unpackbits(self.mask_words.view(np.uint8).reshape(self.mask_words.shape[0], 2, -1), axis=2, bitorder="little")
            self._masks = np.ascontiguousarray(bits[:, :, :self._n_rows]).astype(bool)
        return self._masks

    def __repr__(self):
        return (f"PermutationCheck(pairs={self.pairs}, pairs_violated={self.pairs_violated}, pairs_undecided={self.pairs_undecided}, "
                f"unmatched={self.unmatched}, listed={len(self.list)}, reseeds={self.reseeds})")


def _check_trace_permutations(call, air, n_rows, seed, cap):
    """`call(seed, per_pair, masks, list, cap, summary)` -> rc: one of the two entry points with its leading arguments bound."""
    seed, cap = int(seed), int(cap)
    if cap < 0 or not 0 <= seed < 1 << 64:
        raise StarkhipError(ERR_BAD_SHAPE)
    n_pairs = air_permutation_pairs(air)
    per = np.zeros(n_pairs, dtype=np.uint32)
    words = np.zeros((n_pairs, 2, (n_rows + 63) // 64), dtype=np.uint64)
    entries = np.zeros((min(cap, CHECK_LIST_MAX), 3), dtype=np.uint64)  # a larger cap is the library's to refuse
    summary = _PermCheckStruct()
    _chk(call(seed, per.ctypes.data_as(_u32p), _p64(words) if n_pairs else None, _p64(entries) if cap else None, cap, C.byref(summary)))
    return PermutationCheck(summary, per, words, entries, n_rows)


def check_trace_permutations_replay(air, trace, layout=0, seed=DEFAULT_SEED, cap=1024):
    """starkhip_check_trace_permutations_replay (tests): Prover.check_trace_permutations' host driver with the device steps replaced by
    host loops -- the keys, std::stable_sort, the same classification.  No device needed."""
    trace = np.ascontiguousarray(trace, dtype=np.uint64)
    if trace.ndim != 2 or layout not in (0, 1):
        raise StarkhipError(ERR_BAD_SHAPE)
    n_rows, n_cols = trace.shape if layout == 0 else trace.shape[::-1]
    return _check_trace_permutations(lambda *a: lib.starkhip_check_trace_permutations_replay(air, trace.ctypes.data_as(C.c_void_p), n_rows, n_cols,
                                                                                            layout, *a), air, n_rows, seed, cap)


LOOKUPS_MAX = 64  # STARKHIP_LOOKUPS_MAX


class _LookupStruct(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("input", "table", "permuted_input", "permuted_table")]


class _LookupReportStruct(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("lookups", "lookups_failed", "missing_rows", "listed")]


lib.starkhip_lookup_columns.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.POINTER(_LookupStruct), C.c_size_t, _u32p,
                                        _u64p, _u64p, C.c_size_t, C.POINTER(_LookupReportStruct)]
lib.starkhip_lookup_columns_replay.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(_LookupStruct), C.c_size_t, _u32p, _u64p, _u64p,
                                               C.c_size_t, C.POINTER(_LookupReportStruct)]
lib.starkhip_lookup_timings.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
lib.starkhip_lookup_air_blob.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(_LookupStruct), C.c_size_t, _u64p, C.c_size_t, C.POINTER(C.c_size_t)]


class LookupReport:
    """What starkhip_lookup_columns did, lookup by lookup: `lookups`, `failed`: the lookups some of whose input values their table does
    not hold -- their two output columns were left as they were; `missing_rows`: those input rows over all lookups; `per_lookup`
    (np.uint32[n_lookups]): per lookup; `masks` (bool[n_lookups, n]): masks[q, r] is True when row r of lookup q's input is missing;
    `mask_words` (np.uint64[n_lookups, (n + 63) // 64]): the same as the library wrote it; `list` (np.uint64[listed, 2]): the first
    min(cap, missing_rows) missing rows as (lookup, row), by lookup, then row; `timings`: the call's milliseconds by phase on the
    device (None for the replay)."""

    def __init__(self, summary, per_lookup, words, entries, n_rows, timings=None):
        self.lookups, self.failed, self.missing_rows = int(summary.lookups), int(summary.lookups_failed), int(summary.missing_rows)
        self.per_lookup, self.mask_words = per_lookup, words
        self.list = entries[:int(summary.listed)].copy()
        self.timings = timings
        self._n_rows, self._masks = n_rows, None

    @property
    def masks(self):  # unpacked on first use: eight times the words
        if self._masks is None:
            bits = np.unpackbits(self.mask_words.view(np.uint8).reshape(self.mask_words.shape[0], -1), axis=1, bitorder="little")
            self._masks = np.ascontiguousarray(bits[:, :self._n_rows]).astype(bool)
        return self._masks

    def __repr__(self):
        return f"LookupReport(lookups={self.lookups}, failed={self.failed}, missing_rows={self.missing_rows}, listed={len(self.list)})"


lib.starkhip_air_check_lookups.argtypes = [_u64p, C.c_size_t, C.POINTER(_LookupStruct), C.c_size_t, C.c_char_p, C.c_size_t]
lib.starkhip_air_register_lookups.argtypes = [_u64p, C.c_size_t, C.c_char_p, C.c_uint32, C.POINTER(_LookupStruct), C.c_size_t, C.POINTER(C.c_int)]
lib.starkhip_air_lookups.argtypes = [C.c_int, C.POINTER(_LookupStruct), C.c_size_t]
lib.starkhip_air_lookups.restype = C.c_size_t
lib.starkhip_lookup_blob_layout.argtypes = [_u64p, C.c_size_t, C.POINTER(_LookupReportStruct), C.POINTER(_u64p)]
lib.starkhip_lookup_blob_replay.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.POINTER(_u64p), C.POINTER(C.c_size_t)]
lib.starkhip_lookup_air_register.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(_LookupStruct), C.c_size_t, C.c_char_p, C.c_uint32, C.POINTER(C.c_int)]


class LookupBlobReport:
    """A lookup blob read (parse_lookup_blob): `air`, `n_rows`, `lookups`, `failed`, `missing_rows` and `list` (np.uint64[listed, 2]):
    the first missing rows as (lookup, row), by lookup, then row, cut at the prover's "check_trace_list"."""

    def __init__(self, air, n_rows, summary, entries):
        self.air, self.n_rows = int(air), int(n_rows)
        self.lookups, self.failed, self.missing_rows = int(summary.lookups), int(summary.lookups_failed), int(summary.missing_rows)
        self.list = entries

    def __repr__(self):
        return f"LookupBlobReport(air={self.air}, n_rows={self.n_rows}, failed={self.failed}, missing_rows={self.missing_rows}, listed={len(self.list)})"


def parse_lookup_blob(blob):
    """starkhip_lookup_blob_layout on a lookup blob (np.uint64): its LookupBlobReport; StarkhipError(ERR_BAD_SHAPE) for anything else."""
    b = np.ascontiguousarray(blob, dtype=np.uint64).reshape(-1)
    summary = _LookupReportStruct()
    lst = _u64p()
    _chk(lib.starkhip_lookup_blob_layout(_p64(b), b.size, C.byref(summary), C.byref(lst)))
    listed = int(summary.listed)
    return LookupBlobReport(b[1], b[2], summary, b[8:8 + 2 * listed].reshape(listed, 2).copy())


def lookup_blob_replay(air, trace, layout=0, cap=16):
    """starkhip_lookup_blob_replay (tests, small shapes): the lookup blob a prove with "fill_lookups" must hand back for `trace` (only
    read) with "check_trace_list" = cap, or None when every lookup of the AIR holds; no device needed."""
    trace = np.ascontiguousarray(trace, dtype=np.uint64)
    if trace.ndim != 2 or layout not in (0, 1) or int(cap) < 0:
        raise StarkhipError(ERR_BAD_SHAPE)
    n_rows, n_cols = trace.shape if layout == 0 else trace.shape[::-1]
    out = _u64p()
    words = C.c_size_t()
    rc = lib.starkhip_lookup_blob_replay(air, trace.ctypes.data_as(C.c_void_p), n_rows, n_cols, layout, int(cap), C.byref(out), C.byref(words))
    if rc == 0:
        return None
    if rc != ERR_TRACE:
        raise StarkhipError(rc)
    blob = np.ctypeslib.as_array(out, shape=(words.value,)).copy()
    lib.starkhip_free(out)
    return blob


def lookup_air_register(n_cols, degree, lookups, name=None, default_rows=0):
    """tests: lookup_air_blob's program registered from the C++ AirBuilder with AirBuilder::lookups() as its list (starkhip_lookup_air_register)."""
    arr, nl = _lookup_array(lookups)
    out = C.c_int()
    _chk(lib.starkhip_lookup_air_register(n_cols, degree, arr, nl, name.encode() if name is not None else None, default_rows, C.byref(out)))
    return out.value


def _lookup_array(lookups):
    """lookups: [(input, table, permuted_input, permuted_table), ...] (AirBuilder.lookups) -> the C array"""
    lookups = [tuple(int(c) for c in lk) for lk in lookups]
    if any(len(lk) != 4 or not all(0 <= c < 1 << 32 for c in lk) for lk in lookups):
        raise StarkhipError(ERR_BAD_SHAPE)
    return (_LookupStruct * max(1, len(lookups)))(*[_LookupStruct(*lk) for lk in lookups]), len(lookups)


def _lookup_columns(call, lookups, n_rows, cap):
    """`call(lookups, n_lookups, per_lookup, masks, list, cap, summary)` -> rc: one of the two entry points with its leading arguments bound."""
    cap = int(cap)
    if cap < 0:
        raise StarkhipError(ERR_BAD_SHAPE)
    arr, nl = _lookup_array(lookups)
    per = np.zeros(max(1, nl), dtype=np.uint32)
    words = np.zeros((min(nl, LOOKUPS_MAX), (n_rows + 63) // 64), dtype=np.uint64)  # more lookups are the library's to refuse
    entries = np.zeros((min(cap, CHECK_LIST_MAX), 2), dtype=np.uint64)  # a larger cap is the library's to refuse
    summary = _LookupReportStruct()
    _chk(call(arr, nl, per.ctypes.data_as(_u32p) if nl <= LOOKUPS_MAX else None, _p64(words) if words.size else None, _p64(entries) if cap else None,
              cap, C.byref(summary)))
    return LookupReport(summary, per[:nl], words, entries, n_rows)


def _writable_trace(trace, layout):
    if not isinstance(trace, np.ndarray) or trace.dtype != np.uint64 or trace.ndim != 2 or not trace.flags.c_contiguous or not trace.flags.writeable \
            or layout not in (0, 1):
        raise StarkhipError(ERR_BAD_SHAPE)
    return trace.shape if layout == 0 else trace.shape[::-1]


def lookup_columns_replay(trace, lookups, layout=0, cap=1024):
    """starkhip_lookup_columns_replay (tests): Prover.lookup_columns' host driver with the device steps replaced by host loops that
    implement the rule literally.  Writes into `trace` (a C-contiguous writable np.uint64 array).  No device needed."""
    n_rows, n_cols = _writable_trace(trace, layout)
    return _lookup_columns(lambda *a: lib.starkhip_lookup_columns_replay(trace.ctypes.data_as(C.c_void_p), n_rows, n_cols, layout, *a), lookups,
                           n_rows, cap)


def lookup_air_blob(n_cols, degree, lookups):
    """tests: the program the C++ AirBuilder makes of `n_cols` columns and `degree` with one lookup() per entry (starkhip_lookup_air_blob)."""
    arr, nl = _lookup_array(lookups)
    words = C.c_size_t()
    blob = np.zeros(4096, dtype=np.uint64)
    _chk(lib.starkhip_lookup_air_blob(n_cols, degree, arr, nl, _p64(blob), blob.size, C.byref(words)))
    return blob[:words.value].copy()


# ---- LogUp frequencies (starkhip.h: "LogUp FREQUENCIES")
class _LogupReportStruct(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("lookups", "lookups_failed", "missing_cells", "missing_rows", "listed")]


lib.starkhip_air_logup_fillable.argtypes = [C.c_int]
lib.starkhip_logup_frequencies.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _u32p, _u32p, _u64p, _u64p, C.c_size_t,
                                           C.POINTER(_LogupReportStruct)]
lib.starkhip_logup_frequencies_replay.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, _u32p, _u32p, _u64p, _u64p, C.c_size_t,
                                                  C.POINTER(_LogupReportStruct)]
lib.starkhip_logup_frequency_timings.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
lib.starkhip_logup_blob_layout.argtypes = [_u64p, C.c_size_t, C.POINTER(_LogupReportStruct), C.POINTER(_u64p)]
lib.starkhip_logup_blob_replay.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.POINTER(_u64p), C.POINTER(C.c_size_t)]


def air_logup_fillable(air):
    """starkhip_air_logup_fillable: no frequencies column of the AIR's LogUp lookups is a looked-up or table column of any of them, or
    another lookup's frequencies column -- what logup_frequencies and "fill_frequencies" need."""
    r = lib.starkhip_air_logup_fillable(air)
    if r < 0:
        raise StarkhipError(r)
    return bool(r)


class LogupReport(LookupReport):
    """What starkhip_logup_frequencies did, lookup by lookup: `lookups`, `failed`: the lookups some cell of which their table does not
    hold -- their frequencies column was left as it was; `missing_cells`, `missing_rows`: those cells, and the rows that have one, over
    all lookups; `per_lookup` (np.uint32[n_lookups]): the missing cells of each lookup; `per_column` (np.uint32[sum m]): of each
    looked-up column, the lookups' columns back to back in declaration order; `masks`, `mask_words`, `list`, `timings` as LookupReport's."""

    def __init__(self, summary, per_lookup, per_column, words, entries, n_rows, timings=None):
        super().__init__(summary, per_lookup, words, entries, n_rows, timings)
        self.missing_cells, self.per_column = int(summary.missing_cells), per_column

    def __repr__(self):
        return (f"LogupReport(lookups={self.lookups}, failed={self.failed}, missing_cells={self.missing_cells}, missing_rows={self.missing_rows}, "
                f"listed={len(self.list)})")


def _logup_frequencies(call, n_lookups, n_columns, n_rows, cap):
    """`call(per_lookup, per_column, masks, list, cap, summary)` -> rc: one of the two entry points with its leading arguments bound."""
    cap = int(cap)
    if cap < 0:
        raise StarkhipError(ERR_BAD_SHAPE)
    per = np.zeros(max(1, n_lookups), dtype=np.uint32)
    per_col = np.zeros(max(1, n_columns), dtype=np.uint32)
    words = np.zeros((n_lookups, (n_rows + 63) // 64), dtype=np.uint64)
    entries = np.zeros((min(cap, CHECK_LIST_MAX), 2), dtype=np.uint64)  # a larger cap is the library's to refuse
    summary = _LogupReportStruct()
    _chk(call(per.ctypes.data_as(_u32p), per_col.ctypes.data_as(_u32p), _p64(words) if words.size else None, _p64(entries) if cap else None, cap,
              C.byref(summary)))
    return LogupReport(summary, per[:n_lookups], per_col[:n_columns], words, entries, n_rows)


def _logup_shape(air):
    """(lookups, looked-up columns over all of them) of an AIR's program; (0, 0) for an unknown AIR, which the library refuses"""
    nl, nc = lib.starkhip_air_logups(air), lib.starkhip_air_logup_columns(air)
    return (nl, nc) if nl >= 0 and nc >= 0 else (0, 0)


def logup_frequencies_replay(air, trace, layout=0, cap=1024):
    """starkhip_logup_frequencies_replay (tests): Prover.logup_frequencies' host driver with the device steps replaced by host loops
    that implement the rule literally.  Writes into `trace` (a C-contiguous writable np.uint64 array).  No device needed."""
    n_rows, n_cols = _writable_trace(trace, layout)
    nl, nc = _logup_shape(air)
    return _logup_frequencies(lambda *a: lib.starkhip_logup_frequencies_replay(air, trace.ctypes.data_as(C.c_void_p), n_rows, n_cols, layout, *a), nl, nc,
                              n_rows, cap)


class LogupBlobReport:
    """A LogUp blob read (parse_logup_blob): `air`, `n_rows`, `lookups`, `failed`, `missing_cells`, `missing_rows` and `list`
    (np.uint64[listed, 2]): the first missing rows as (lookup, row), by lookup, then row, cut at the prover's "check_trace_list"."""

    def __init__(self, air, n_rows, summary, entries):
        self.air, self.n_rows = int(air), int(n_rows)
        self.lookups, self.failed = int(summary.lookups), int(summary.lookups_failed)
        self.missing_cells, self.missing_rows = int(summary.missing_cells), int(summary.missing_rows)
        self.list = entries

    def __repr__(self):
        return (f"LogupBlobReport(air={self.air}, n_rows={self.n_rows}, failed={self.failed}, missing_cells={self.missing_cells}, "
                f"missing_rows={self.missing_rows}, listed={len(self.list)})")


def logup_blob_layout(blob):
    """starkhip_logup_blob_layout on a LogUp blob (np.uint64): its LogupBlobReport; StarkhipError(ERR_BAD_SHAPE) for anything else."""
    b = np.ascontiguousarray(blob, dtype=np.uint64).reshape(-1)
    summary = _LogupReportStruct()
    lst = _u64p()
    _chk(lib.starkhip_logup_blob_layout(_p64(b), b.size, C.byref(summary), C.byref(lst)))
    listed = int(summary.listed)
    return LogupBlobReport(b[1], b[2], summary, b[8:8 + 2 * listed].reshape(listed, 2).copy())


parse_logup_blob = logup_blob_layout


def logup_blob_replay(air, trace, layout=0, cap=16):
    """starkhip_logup_blob_replay (tests, small shapes): the LogUp blob a prove with "fill_frequencies" must hand back for `trace`
    (only read) with "check_trace_list" = cap, or None when every lookup of the AIR holds; no device needed."""
    trace = np.ascontiguousarray(trace, dtype=np.uint64)
    if trace.ndim != 2 or layout not in (0, 1) or int(cap) < 0:
        raise StarkhipError(ERR_BAD_SHAPE)
    n_rows, n_cols = trace.shape if layout == 0 else trace.shape[::-1]
    out = _u64p()
    words = C.c_size_t()
    rc = lib.starkhip_logup_blob_replay(air, trace.ctypes.data_as(C.c_void_p), n_rows, n_cols, layout, int(cap), C.byref(out), C.byref(words))
    if rc == 0:
        return None
    if rc != ERR_TRACE:
        raise StarkhipError(rc)
    blob = np.ctypeslib.as_array(out, shape=(words.value,)).copy()
    lib.starkhip_free(out)
    return blob


# ----------------------------------------------------------------------------- traces (generate_trace)
class CompactTrace:
    """A trace recorded as runs (starkhip_trace_log_*): the generator's limb vectors with the rows they
    repeat on, expanded on the device by `Prover.prove`.  `shape` is the shape of the dense trace it stands for."""

    def __init__(self, handle):
        self._h = handle
        v = [C.c_size_t() for _ in range(4)]
        _chk(lib.starkhip_trace_log_info(handle, *[C.byref(x) for x in v]))
        self.shape = (v[0].value, v[1].value)
        self.n_records, self.nbytes = v[2].value, 4 * (v[3].value + v[2].value)
        self._fin = weakref.finalize(self, lib.starkhip_trace_log_free, handle)

    def overwrites(self):
        """(records whose run a later clear took back to zero rows, cells cleared inside a longer run) -- the traces of the fillers'
        set-then-clear idiom (trace_log.h: TraceLog::set)."""
        e, z = C.c_size_t(), C.c_size_t()
        _chk(lib.starkhip_trace_log_overwrites(self._h, C.byref(e), C.byref(z)))
        return e.value, z.value

    def expand(self):
        """(dense row-major trace, number of cells two records disagree on) -- CPU replay, for tests."""
        out = np.empty(self.shape, dtype=np.uint64)
        bad = C.c_size_t()
        _chk(lib.starkhip_trace_log_expand_host(self._h, _p64(out), C.byref(bad)))
        return out, bad.value


class _Recording:
    """with _Recording() as r: <one starkhip_trace_* call with a null trace>;  r.trace is the CompactTrace."""

    def __enter__(self):
        self._h = C.c_void_p()
        _chk(lib.starkhip_trace_log_begin(C.byref(self._h)))
        self.trace = None
        return self

    def __exit__(self, et, ev, tb):
        rc = lib.starkhip_trace_log_end(self._h)
        if et is None and rc == 0:
            self.trace = CompactTrace(self._h)
        else:
            lib.starkhip_trace_log_free(self._h)
            if et is None:
                raise StarkhipError(rc)
        return False


def set_trace_threads(n):
    """Host threads one RECORDING generator call may use (starkhip_trace_set_threads; only trace_final_exp uses more than
    one).  Returns the previous setting.  The recorded trace does not depend on it."""
    return int(lib.starkhip_trace_set_threads(int(n)))


def _generate(air, n_rows, out, compact, call):
    """Run one generator: into a dense array (returned, or `out`), or recorded (compact=True)."""
    if compact:
        pis = np.zeros(air_public_inputs(air), dtype=np.uint64)
        with _Recording() as r:
            _chk(call(C.cast(None, _u64p), n_rows or air_default_rows(air), _p64(pis)))
        return r.trace, pis
    t, pis, n = _trace_alloc(air, n_rows, out)
    _chk(call(_p64(t), n, _p64(pis)))
    return t, pis


def _trace_alloc(air, n_rows, out=None):
    """`out`: optional C-contiguous uint64 [n_rows][columns] array to generate into (e.g. Prover.host_array); the
    generators clear it themselves."""
    n_rows = n_rows or air_default_rows(air)
    shape = (n_rows, air_columns(air))
    if out is None:
        out = np.zeros(shape, dtype=np.uint64)
    elif out.shape != shape or out.dtype != np.uint64 or not out.flags.c_contiguous:
        raise ValueError(f"trace buffer must be C-contiguous uint64 {shape}, got {out.dtype} {out.shape}")
    return out, np.zeros(air_public_inputs(air), dtype=np.uint64), n_rows


def trace_from_writes(n_rows, n_cols, writes):
    """A CompactTrace from explicit (row, col, value) writes applied in order through the recorder (tests of its corner cases)."""
    w = np.ascontiguousarray(writes, dtype=np.uint64).reshape(-1, 3)
    h = C.c_void_p()
    _chk(lib.starkhip_trace_log_from_writes(n_rows, n_cols, _p64(w), w.shape[0], C.byref(h)))
    return CompactTrace(h)


def trace_fibonacci(x0, x1, n_rows=None, out=None):
    t, pis, n = _trace_alloc(AIR_TEST_FIBONACCI, n_rows, out)
    _chk(lib.starkhip_trace_fibonacci(x0, x1, _p64(t), n, _p64(pis)))
    return t, pis


def trace_fp12_mul(x, y, n_rows=None, out=None, compact=False):
    """FP12MulStark::generate_trace + the public inputs of fp12_mul_main (src/aggregate_proof.rs:117-148).
    compact=True (every generator below): a CompactTrace instead of the dense rows."""
    xs, ys = _limbs(x, 144), _limbs(y, 144)
    return _generate(AIR_FP12_MUL, n_rows, out, compact, lambda t, n, p: lib.starkhip_trace_fp12_mul(_p32(xs), _p32(ys), t, n, p))


def trace_final_exp(x, n_rows=None, out=None, compact=False):
    xs = _limbs(x, 144)
    return _generate(AIR_FINAL_EXP, n_rows, out, compact, lambda t, n, p: lib.starkhip_trace_final_exp(_p32(xs), t, n, p))


def _ecc_inputs(points, bits):
    pts = np.ascontiguousarray(points, dtype=np.uint32).reshape(-1)
    b = np.ascontiguousarray(np.asarray(bits).astype(bool), dtype=np.uint8).reshape(-1)
    assert pts.size == 24 * ECC_NUM_POINTS and b.size == ECC_NUM_POINTS, (pts.size, b.size)
    return pts, b


def trace_ecc_aggregate(points, bits, n_rows=None, out=None, compact=False):
    """ECCAggStark::generate_trace + ec_aggregate_main's public inputs (src/ecc_aggregate.rs:39-84, src/aggregate_proof.rs:191-209).
    points: [512][24] u32 limbs (x then y); bits: 512 booleans.  The aggregate lands in the last 24 public inputs."""
    pts, b = _ecc_inputs(points, bits)
    return _generate(AIR_ECC_AGGREGATE, n_rows, out, compact,
                     lambda t, n, p: lib.starkhip_trace_ecc_aggregate(_p32(pts), b.ctypes.data_as(_u8p), t, n, p))


def native_g1_aggregate(points, bits):
    """Sum of the points whose bit is set, in the reference's order of operations; 24 limbs (x, y)."""
    pts, b = _ecc_inputs(points, bits)
    out = np.zeros(24, dtype=np.uint32)
    _chk(lib.starkhip_native_g1_aggregate(_p32(pts), b.ctypes.data_as(_u8p), _p32(out)))
    return out


def trace_miller_loop(px, py, qx, qy, qz, n_rows=None, out=None, compact=False):
    a = [_limbs(px, 12), _limbs(py, 12), _limbs(qx, 24), _limbs(qy, 24), _limbs(qz, 24)]
    return _generate(AIR_MILLER_LOOP, n_rows, out, compact, lambda t, n, p: lib.starkhip_trace_miller_loop(*[_p32(v) for v in a], t, n, p))


def trace_pairing_precomp(qx, qy, qz, n_rows=None, out=None, compact=False):
    a = [_limbs(qx, 24), _limbs(qy, 24), _limbs(qz, 24)]
    return _generate(AIR_PAIRING_PRECOMP, n_rows, out, compact, lambda t, n, p: lib.starkhip_trace_pairing_precomp(*[_p32(v) for v in a], t, n, p))


def native_fp12_mul(x, y):
    out = np.zeros(144, dtype=np.uint32)
    _chk(lib.starkhip_native_fp12_mul(_p32(_limbs(x, 144)), _p32(_limbs(y, 144)), _p32(out)))
    return out


def native_final_exponentiate(x):
    out = np.zeros(144, dtype=np.uint32)
    _chk(lib.starkhip_native_final_exponentiate(_p32(_limbs(x, 144)), _p32(out)))
    return out


def native_miller_loop(px, py, qx, qy, qz):
    out = np.zeros(144, dtype=np.uint32)
    _chk(lib.starkhip_native_miller_loop(_p32(_limbs(px, 12)), _p32(_limbs(py, 12)), _p32(_limbs(qx, 24)), _p32(_limbs(qy, 24)),
                                         _p32(_limbs(qz, 24)), _p32(out)))
    return out


def native_pairing_precomp(qx, qy, qz):
    out = np.zeros(68 * 72, dtype=np.uint32)
    _chk(lib.starkhip_native_pairing_precomp(_p32(_limbs(qx, 24)), _p32(_limbs(qy, 24)), _p32(_limbs(qz, 24)), _p32(out)))
    return out


def poseidon_permute_host(state):
    s = np.ascontiguousarray(state, dtype=np.uint64).copy()
    assert s.size == 12
    lib.starkhip_poseidon_permute_host(_p64(s))
    return s


def keccak256(data):
    """keccak256 (padding 0x01 .. 0x80) of `data` on the host: 32 bytes."""
    data = bytes(data)
    out = (C.c_uint8 * 32)()
    lib.starkhip_keccak256(data, len(data), out)
    return bytes(out)


def keccak_permute_host(state):
    """The challenger's permutation under the Keccak hasher (COMPAT.md K7) on one state of 12 canonical words."""
    s = np.ascontiguousarray(state, dtype=np.uint64).copy()
    assert s.size == 12
    lib.starkhip_keccak_permute_host(_p64(s))
    return s


def keccak_state_from_words(words):
    """K7's word filter: (state of 12, words consumed), or (partial state, -1) when `words` holds fewer than 12 words below p."""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    state = np.zeros(12, dtype=np.uint64)
    used = lib.starkhip_keccak_state_from_words(_p64(w), w.size, _p64(state))
    return state, used


def proof_hasher(proof):
    """HASHER_POSEIDON or HASHER_KECCAK: the hasher a proof's header names (every verify entry verifies under it)."""
    p = np.ascontiguousarray(proof, dtype=np.uint64)
    rc = lib.starkhip_proof_hasher(_p64(p), p.size)
    if rc < 0:
        raise StarkhipError(rc)
    return rc


def _column_table(columns):
    """(pointer table, the arrays it points into, n_rows) for starkhip_prove_columns / starkhip_pool_submit_columns."""
    keep = [np.ascontiguousarray(c, dtype=np.uint64) for c in columns]
    if not keep or any(c.ndim != 1 or c.size != keep[0].size for c in keep):
        raise StarkhipError(ERR_BAD_SHAPE)
    addrs = np.fromiter((c.ctypes.data for c in keep), dtype=np.uint64, count=len(keep))
    table = (C.c_void_p * len(keep)).from_buffer_copy(addrs.tobytes())
    return table, keep, keep[0].size


# ----------------------------------------------------------------------------- prover / verifier
class Prover:
    """One context per GPU (starkhip_init).  `prove` mirrors starky::prover::prove."""

    def __init__(self, device=0):
        self._ctx = C.c_void_p()
        _chk(lib.starkhip_init(device, C.byref(self._ctx)))

    def close(self):
        if self._ctx:
            lib.starkhip_shutdown(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def prove(self, air, config, trace, public_inputs, pow_witness=POW_SEARCH, layout=0):
        """trace: numpy uint64, row-major [n][C] (layout 0) or column-major [C][n] (layout 1), or a CompactTrace."""
        if isinstance(trace, CompactTrace):
            pis = np.ascontiguousarray(public_inputs, dtype=np.uint64)
            out = _u64p()
            words = C.c_size_t()
            t0 = time.perf_counter()
            rc = lib.starkhip_prove_compact(self._ctx, air, C.byref(config), trace._h, _p64(pis), pis.size, pow_witness, C.byref(out), C.byref(words))
            self.last_call_s = time.perf_counter() - t0  # the C call alone, without the copy into a numpy array below
            return _take_blob(rc, out, words)
        trace = np.ascontiguousarray(trace, dtype=np.uint64)
        if trace.ndim != 2 or layout not in (0, 1):
            raise StarkhipError(ERR_BAD_SHAPE)
        n_rows, n_cols = trace.shape if layout == 0 else trace.shape[::-1]
        pis = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        out = _u64p()
        words = C.c_size_t()
        t0 = time.perf_counter()
        rc = lib.starkhip_prove(self._ctx, air, C.byref(config), trace.ctypes.data_as(C.c_void_p), n_rows, n_cols, layout, 0, _p64(pis), pis.size,
                                pow_witness, C.byref(out), C.byref(words))
        self.last_call_s = time.perf_counter() - t0
        return _take_blob(rc, out, words)

    def prove_columns(self, air, config, columns, public_inputs, pow_witness=POW_SEARCH):
        """starky's literal `prove(stark, &config, trace_poly_values, ..)`: `columns` is a sequence of separately allocated 1-D uint64
        arrays, one per trace column (`Vec<PolynomialValues<F>>`, src/aggregate_proof.rs:168-175)."""
        table, keep, n_rows = _column_table(columns)
        pis = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        out = _u64p()
        words = C.c_size_t()
        rc = lib.starkhip_prove_columns(self._ctx, air, C.byref(config), table, n_rows, len(keep), _p64(pis), pis.size, pow_witness, C.byref(out),
                                        C.byref(words))
        return _take_blob(rc, out, words)

    def check_trace(self, air, trace, public_inputs, layout=0):
        """Every constraint of `air` on every row of `trace` (row-major [n][C], or column-major [C][n] with layout=1), on this context's
        device: (violations, (constraint, row, value) of the lowest violated constraint, on its lowest row).  No violation: (0, (0, 0, 0))."""
        trace = np.ascontiguousarray(trace, dtype=np.uint64)
        if trace.ndim != 2 or layout not in (0, 1):
            raise StarkhipError(ERR_BAD_SHAPE)
        n_rows, n_cols = trace.shape if layout == 0 else trace.shape[::-1]
        pis = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        if pis.size != air_public_inputs(air):
            raise StarkhipError(ERR_BAD_SHAPE)
        bad = C.c_uint64()
        first = np.zeros(3, dtype=np.uint64)
        t0 = time.perf_counter()
        rc = lib.starkhip_check_trace(self._ctx, air, trace.ctypes.data_as(C.c_void_p), n_rows, n_cols, layout, 0, _p64(pis), C.byref(bad),
                                      _p64(first))
        self.last_call_s = time.perf_counter() - t0
        _chk(rc)
        return bad.value, tuple(int(x) for x in first)

    def permutation_zs(self, air, trace, challenges, layout=0):
        """permutation_zs_replay's result from this context's device, through the kernels prove() uses (starkhip_permutation_zs)."""
        trace = np.ascontiguousarray(trace, dtype=np.uint64)
        if trace.ndim != 2 or layout not in (0, 1):
            raise StarkhipError(ERR_BAD_SHAPE)
        n_rows, n_cols = trace.shape if layout == 0 else trace.shape[::-1]
        challenges, zs, closing = _perm_zs_args(air, n_rows, challenges)
        _chk(lib.starkhip_permutation_zs(self._ctx, air, trace.ctypes.data_as(C.c_void_p), n_rows, n_cols, layout, 0, _p64(challenges), _p64(zs),
                                         _p64(closing)))
        return zs, closing

    def logup_polys(self, air, trace, challenges, layout=0):
        """logup_polys_replay's result from this context's device, through the kernels prove() uses (starkhip_logup_polys)."""
        trace = np.ascontiguousarray(trace, dtype=np.uint64)
        if trace.ndim != 2 or layout not in (0, 1):
            raise StarkhipError(ERR_BAD_SHAPE)
        n_rows, n_cols = trace.shape if layout == 0 else trace.shape[::-1]
        challenges, polys, closing, zeros = _logup_args(air, n_rows, challenges)
        _chk(lib.starkhip_logup_polys(self._ctx, air, trace.ctypes.data_as(C.c_void_p), n_rows, n_cols, layout, 0, _p64(challenges), _p64(polys),
                                      _p64(closing), _p64(zeros)))
        return polys, closing, int(zeros[0])

    def logup_polys_device(self, air, trace_ptr, n_rows, challenges, layout=1):
        """logup_polys on a trace already in this device's memory (trace_ptr: a device address, e.g. torch tensor.data_ptr())."""
        challenges, polys, closing, zeros = _logup_args(air, n_rows, challenges)
        _chk(lib.starkhip_logup_polys(self._ctx, air, C.c_void_p(trace_ptr), n_rows, air_columns(air), layout, 1, _p64(challenges), _p64(polys),
                                      _p64(closing), _p64(zeros)))
        return polys, closing, int(zeros[0])

    def permutation_zs_device(self, air, trace_ptr, n_rows, challenges, layout=1):
        """permutation_zs on a trace already in this device's memory (trace_ptr: a device address, e.g. torch tensor.data_ptr())."""
        challenges, zs, closing = _perm_zs_args(air, n_rows, challenges)
        _chk(lib.starkhip_permutation_zs(self._ctx, air, C.c_void_p(trace_ptr), n_rows, air_columns(air), layout, 1, _p64(challenges), _p64(zs),
                                         _p64(closing)))
        return zs, closing

    def check_trace_permutations(self, air, trace, layout=0, seed=DEFAULT_SEED, cap=1024):
        """Which rows of each permutation pair of `air` have no partner on the pair's other side (starkhip_check_trace_permutations): a
        PermutationCheck.  Exact and per pair -- a sort and a classification on this context's device -- where the closing products
        of permutation_zs speak of a whole batch under random challenges."""
        trace = np.ascontiguousarray(trace, dtype=np.uint64)
        if trace.ndim != 2 or layout not in (0, 1):
            raise StarkhipError(ERR_BAD_SHAPE)
        n_rows, n_cols = trace.shape if layout == 0 else trace.shape[::-1]
        return self._check_trace_permutations(air, trace.ctypes.data_as(C.c_void_p), n_rows, n_cols, layout, 0, seed, cap)

    def check_trace_permutations_device(self, air, trace_ptr, n_rows, layout=1, seed=DEFAULT_SEED, cap=1024):
        """check_trace_permutations on a trace already in this device's memory (trace_ptr: a device address, e.g. torch tensor.data_ptr())."""
        return self._check_trace_permutations(air, C.c_void_p(trace_ptr), n_rows, air_columns(air), layout, 1, seed, cap)

    def _check_trace_permutations(self, air, trace_arg, n_rows, n_cols, layout, on_device, seed, cap):
        t0 = time.perf_counter()
        try:
            return _check_trace_permutations(lambda *a: lib.starkhip_check_trace_permutations(self._ctx, air, trace_arg, n_rows, n_cols, layout,
                                                                                             on_device, *a), air, n_rows, seed, cap)
        finally:
            self.last_call_s = time.perf_counter() - t0

    def last_perm_check_timings(self):
        """Milliseconds of the last check_trace_permutations: {upload, sort, classify, read_back} (starkhip_perm_check_timings)."""
        ms = (C.c_float * 4)()
        _chk(lib.starkhip_perm_check_timings(self._ctx, ms))
        return dict(zip(("upload", "sort", "classify", "read_back"), (float(x) for x in ms)))

    def lookup_columns(self, trace, lookups, layout=0, cap=1024):
        """Fill the permuted columns of each lookup of `lookups` -- [(input, table, permuted_input, permuted_table), ...], e.g.
        AirBuilder.lookups -- in `trace` (starkhip_lookup_columns): a sort and a placement per lookup on this context's device, written
        into the array given (C-contiguous, writable, np.uint64; row-major [n][C], or column-major [C][n] with layout=1).  A lookup
        whose table lacks a value of its input keeps its columns as they were and reports the rows.  Returns a LookupReport."""
        n_rows, n_cols = _writable_trace(trace, layout)
        return self._lookup_columns(trace.ctypes.data_as(C.c_void_p), n_rows, n_cols, layout, 0, lookups, cap)

    def lookup_columns_device(self, trace_ptr, n_rows, n_cols, lookups, layout=1, cap=1024):
        """lookup_columns on a trace already in this device's memory (trace_ptr: a device address, e.g. torch tensor.data_ptr()),
        written in place."""
        return self._lookup_columns(C.c_void_p(trace_ptr), n_rows, n_cols, layout, 1, lookups, cap)

    def _lookup_columns(self, trace_arg, n_rows, n_cols, layout, on_device, lookups, cap):
        t0 = time.perf_counter()
        try:
            rep = _lookup_columns(lambda *a: lib.starkhip_lookup_columns(self._ctx, trace_arg, n_rows, n_cols, layout, on_device, *a), lookups,
                                  n_rows, cap)
        finally:
            self.last_call_s = time.perf_counter() - t0
        rep.timings = self.last_lookup_timings()
        return rep

    def last_lookup_timings(self):
        """Milliseconds of the last lookup_columns: {upload, sort, place, read_back} (starkhip_lookup_timings)."""
        ms = (C.c_float * 4)()
        _chk(lib.starkhip_lookup_timings(self._ctx, ms))
        return dict(zip(("upload", "sort", "place", "read_back"), (float(x) for x in ms)))

    def logup_frequencies(self, air, trace, layout=0, cap=1024):
        """Fill the frequencies column of each LogUp lookup of `air` in `trace` (starkhip_logup_frequencies): the tables sorted once
        each and one lane per looked-up cell on this context's device, written into the array given (C-contiguous, writable,
        np.uint64; row-major [n][C], or column-major [C][n] with layout=1).  A lookup some cell of which its table lacks keeps its
        column as it was and reports the rows and the columns.  Returns a LogupReport."""
        n_rows, n_cols = _writable_trace(trace, layout)
        return self._logup_frequencies(air, trace.ctypes.data_as(C.c_void_p), n_rows, n_cols, layout, 0, cap)

    def logup_frequencies_device(self, air, trace_ptr, n_rows, n_cols, layout=1, cap=1024):
        """logup_frequencies on a trace already in this device's memory (trace_ptr: a device address, e.g. torch tensor.data_ptr()),
        read and written in place."""
        return self._logup_frequencies(air, C.c_void_p(trace_ptr), n_rows, n_cols, layout, 1, cap)

    def _logup_frequencies(self, air, trace_arg, n_rows, n_cols, layout, on_device, cap):
        nl, nc = _logup_shape(air)
        t0 = time.perf_counter()
        try:
            rep = _logup_frequencies(lambda *a: lib.starkhip_logup_frequencies(self._ctx, air, trace_arg, n_rows, n_cols, layout, on_device, *a), nl, nc,
                                     n_rows, cap)
        finally:
            self.last_call_s = time.perf_counter() - t0
        rep.timings = self.last_logup_frequency_timings()
        return rep

    def last_logup_frequency_timings(self):
        """Milliseconds of the last fill of LogUp frequencies on this context: {upload, sort, count, write, read_back}
        (starkhip_logup_frequency_timings)."""
        ms = (C.c_float * 5)()
        _chk(lib.starkhip_logup_frequency_timings(self._ctx, ms))
        return dict(zip(("upload", "sort", "count", "write", "read_back"), (float(x) for x in ms)))

    def check_trace_device(self, air, trace_ptr, n_rows, public_inputs, layout=1):
        """check_trace on a trace already in this device's memory (trace_ptr: a device address, e.g. torch tensor.data_ptr())."""
        pis = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        if pis.size != air_public_inputs(air):
            raise StarkhipError(ERR_BAD_SHAPE)
        bad = C.c_uint64()
        first = np.zeros(3, dtype=np.uint64)
        t0 = time.perf_counter()
        rc = lib.starkhip_check_trace(self._ctx, air, C.c_void_p(trace_ptr), n_rows, air_columns(air), layout, 1, _p64(pis), C.byref(bad),
                                      _p64(first))
        self.last_call_s = time.perf_counter() - t0
        _chk(rc)
        return bad.value, tuple(int(x) for x in first)

    def check_trace_report(self, air, trace, public_inputs, layout=0, cap=1024):
        """check_trace in full (starkhip_check_trace_report): a CheckReport with the count of violated rows per constraint, the violated
        rows and the first `cap` violations (constraint, row, value) by constraint, then row."""
        trace = np.ascontiguousarray(trace, dtype=np.uint64)
        if trace.ndim != 2 or layout not in (0, 1):
            raise StarkhipError(ERR_BAD_SHAPE)
        n_rows, n_cols = trace.shape if layout == 0 else trace.shape[::-1]
        return self._check_trace_report(air, trace.ctypes.data_as(C.c_void_p), n_rows, n_cols, layout, 0, public_inputs, cap)

    def check_trace_report_device(self, air, trace_ptr, n_rows, public_inputs, layout=1, cap=1024):
        """check_trace_report on a trace already in this device's memory (trace_ptr: a device address, e.g. torch tensor.data_ptr())."""
        return self._check_trace_report(air, C.c_void_p(trace_ptr), n_rows, air_columns(air), layout, 1, public_inputs, cap)

    def _check_trace_report(self, air, trace_arg, n_rows, n_cols, layout, on_device, public_inputs, cap):
        pis = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        if pis.size != air_public_inputs(air):
            raise StarkhipError(ERR_BAD_SHAPE)
        t0 = time.perf_counter()
        try:
            return _check_trace_report(lambda *out: lib.starkhip_check_trace_report(self._ctx, air, trace_arg, n_rows, n_cols, layout, on_device,
                                                                                    _p64(pis), *out), air, n_rows, cap)
        finally:
            self.last_call_s = time.perf_counter() - t0

    def free_cells(self, air, trace, public_inputs, layout=0, delta=DEFAULT_DELTA, mask=True):
        """The cells of `trace` (as check_trace takes it) that no constraint of `air` notices when `delta` is added to them
        (starkhip_check_trace_free_cells): a FreeCells.  mask=False leaves the per-cell bitmap on the device.  DEFAULT_DELTA is a fixed
        constant; pass a random delta in 1 .. P - 1 for a real audit."""
        trace = np.ascontiguousarray(trace, dtype=np.uint64)
        if trace.ndim != 2 or layout not in (0, 1):
            raise StarkhipError(ERR_BAD_SHAPE)
        n_rows, n_cols = trace.shape if layout == 0 else trace.shape[::-1]
        return self._free_cells(air, trace.ctypes.data_as(C.c_void_p), n_rows, n_cols, layout, 0, public_inputs, delta, mask)

    def free_cells_device(self, air, trace_ptr, n_rows, public_inputs, layout=1, delta=DEFAULT_DELTA, mask=True):
        """free_cells on a trace already in this device's memory (trace_ptr: a device address, e.g. torch tensor.data_ptr())."""
        return self._free_cells(air, C.c_void_p(trace_ptr), n_rows, air_columns(air), layout, 1, public_inputs, delta, mask)

    def _free_cells(self, air, trace_arg, n_rows, n_cols, layout, on_device, public_inputs, delta, mask):
        pis, delta = _free_cells_args(air, public_inputs, delta)
        t0 = time.perf_counter()
        try:
            return _free_cells(lambda *out: lib.starkhip_check_trace_free_cells(self._ctx, air, trace_arg, n_rows, n_cols, layout, on_device,
                                                                                _p64(pis), delta, *out), n_rows, n_cols, mask)
        finally:
            self.last_call_s = time.perf_counter() - t0

    def free_cell_classes(self, air, trace, public_inputs, layout=0, delta=DEFAULT_DELTA, planes=True):
        """free_cells' free cells told apart (starkhip_check_trace_free_cell_classes): a FreeCellClasses -- unread, gated off, or read with
        the gates open and not noticed -- with the rows each constraint's gates were open on.  planes=False leaves the three bitmaps on
        the device."""
        trace = np.ascontiguousarray(trace, dtype=np.uint64)
        if trace.ndim != 2 or layout not in (0, 1):
            raise StarkhipError(ERR_BAD_SHAPE)
        n_rows, n_cols = trace.shape if layout == 0 else trace.shape[::-1]
        return self._free_cell_classes(air, trace.ctypes.data_as(C.c_void_p), n_rows, n_cols, layout, 0, public_inputs, delta, planes)

    def free_cell_classes_device(self, air, trace_ptr, n_rows, public_inputs, layout=1, delta=DEFAULT_DELTA, planes=True):
        """free_cell_classes on a trace already in this device's memory (trace_ptr: a device address, e.g. torch tensor.data_ptr())."""
        return self._free_cell_classes(air, C.c_void_p(trace_ptr), n_rows, air_columns(air), layout, 1, public_inputs, delta, planes)

    def _free_cell_classes(self, air, trace_arg, n_rows, n_cols, layout, on_device, public_inputs, delta, planes):
        pis, delta = _free_cells_args(air, public_inputs, delta)
        t0 = time.perf_counter()
        try:
            return _free_cell_classes(lambda *out: lib.starkhip_check_trace_free_cell_classes(self._ctx, air, trace_arg, n_rows, n_cols, layout,
                                                                                              on_device, _p64(pis), delta, *out),
                                      air, n_rows, n_cols, planes)
        finally:
            self.last_call_s = time.perf_counter() - t0

    def lde_bench(self, n_cols, log_n, rate_bits, reps=5, const_per_64=0, device_ptr=None, each=False):
        """starkhip_lde_bench: average milliseconds of one values -> LDE launch over `n_cols` synthetic columns."""
        ms = C.c_float()
        per = (C.c_float * 16)()
        _chk(lib.starkhip_lde_bench(self._ctx, n_cols, log_n, rate_bits, reps, const_per_64, C.c_void_p(device_ptr) if device_ptr else None, C.byref(ms), per))
        return [round(float(x), 2) for x in per[:max(1, min(reps, 16))]] if each else float(ms.value)

    def expand_trace(self, compact):
        """A CompactTrace through the device's expansion kernels; returns the dense row-major [n][C] matrix (tests)."""
        n, c = compact.shape
        out = np.empty((c, n), dtype=np.uint64)
        _chk(lib.starkhip_trace_log_expand_device(self._ctx, compact._h, _p64(out)))
        return np.ascontiguousarray(out.T)

    def set_option(self, name, value):
        """Tuning knob of this context (starkhip_set_option).  "check_trace" = 1: every prove* checks its trace against the AIR on the
        device before the LDE and raises TraceViolation for a violating one ("check_trace_list": the violations its report lists).
        "fill_lookups" = 1: every prove* of an AIR registered with its lookups (register_air(lookups=...)) fills their permuted columns
        in the prover's own copy of the trace first, and raises TraceViolation with a lookup blob when a lookup fails.
        "fill_frequencies" = 1: every prove* of a fillable AIR with LogUp lookups fills their frequencies columns likewise, and raises
        TraceViolation with a LogUp blob (`.logup_report`) when a cell misses its table.
        "leaf_hash_prefix" (default 1; 0: off): the lane and pair forms of the leaf hash start a trace whose first `rows` columns are
        e_0 .. e_{rows-1} (FinalExp's row selectors) from a saved state past them; same proof bytes either way.  The other names
        ("hasher", "leaf_hash_form", "lde_closed_forms", "lde_impl", "host_commit_leaves", "quotient_*", ...): include/starkhip.h."""
        _chk(lib.starkhip_set_option(self._ctx, name.encode(), int(value)))

    def check_stats(self):
        """starkhip_check_stats: {"checked", "rejected"} -- traces this context's proofs have checked / refused so far."""
        out = np.zeros(2, dtype=np.uint64)
        _chk(lib.starkhip_check_stats(self._ctx, _p64(out)))
        return {"checked": int(out[0]), "rejected": int(out[1])}

    def prove_device(self, air, config, trace_ptr, n_rows, public_inputs, pow_witness=POW_SEARCH, layout=1, keep=True):
        """trace_ptr: integer device address of a uint64 trace (n_rows x air_columns(air) words) already resident in HBM
        (benchmark path)."""
        pis = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        out = _u64p()
        words = C.c_size_t()
        t0 = time.perf_counter()
        rc = lib.starkhip_prove(self._ctx, air, C.byref(config), C.c_void_p(trace_ptr), n_rows, air_columns(air), layout, 1, _p64(pis), pis.size, pow_witness,
                                C.byref(out), C.byref(words))
        self.last_call_s = time.perf_counter() - t0
        return _take_blob(rc, out, words, keep)

    def host_array(self, shape, dtype=np.uint64):
        """Page-locked host array (starkhip_host_alloc) to generate traces into, again and again (`trace_*(…, out=buf)`):
        no 4.8 GB of first-touch page faults per FinalExp trace.  Freed when the array (and every view of it) is gone."""
        shape = tuple(int(s) for s in np.atleast_1d(shape))
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        _chk(lib.starkhip_host_alloc(self._ctx, nbytes, C.byref(p)))
        raw = (C.c_ubyte * nbytes).from_address(p.value)
        weakref.finalize(raw, lib.starkhip_host_free, p.value)
        return np.frombuffer(raw, dtype=dtype).reshape(shape)

    def last_timings(self):
        ms = (C.c_float * N_PHASES)()
        _chk(lib.starkhip_last_timings(self._ctx, ms))
        return dict(zip(PHASE_NAMES, [float(x) for x in ms]))

    def last_host_timings(self):
        ms = (C.c_float * 2)()
        _chk(lib.starkhip_last_host_timings(self._ctx, ms))
        return {"fiat_shamir": float(ms[0]), "other": float(ms[1])}

    def last_kernel_timings(self):
        ms = (C.c_float * 3)()
        _chk(lib.starkhip_last_kernel_timings(self._ctx, ms))
        return {"lde_columns": float(ms[0]), "leaf_hash": float(ms[1]), "quotient_eval": float(ms[2])}

    def ntt_long(self, vectors, inverse=False):
        """starkhip_ntt_long: the rows of `vectors` (2^16 .. 2^26 words each) through the multi-workgroup transform; returns the transforms."""
        v = np.ascontiguousarray(vectors, dtype=np.uint64).copy()
        n_vecs, n = v.shape
        _chk(lib.starkhip_ntt_long(self._ctx, _p64(v), n_vecs, n.bit_length() - 1, 1 if inverse else 0))
        return v

    def lde_batch(self, values_colmajor, rate_bits):
        v = np.ascontiguousarray(values_colmajor, dtype=np.uint64)
        ncols, n = v.shape
        log_n = n.bit_length() - 1
        coeffs = np.zeros_like(v)
        lde = np.zeros((ncols, n << rate_bits), dtype=np.uint64)
        _chk(lib.starkhip_lde_batch(self._ctx, _p64(v), ncols, log_n, rate_bits, _p64(coeffs), _p64(lde)))
        return coeffs, lde

    def merkle_cap(self, lde_colmajor, cap_height):
        v = np.ascontiguousarray(lde_colmajor, dtype=np.uint64)
        ncols, N = v.shape
        cap = np.zeros((1 << cap_height, 4), dtype=np.uint64)
        _chk(lib.starkhip_merkle_cap(self._ctx, _p64(v), ncols, N.bit_length() - 1, cap_height, _p64(cap)))
        return cap

    def merkle_tree(self, lde_colmajor, cap_height, hasher=HASHER_POSEIDON):
        """(leaf digests [N][4] in tree order, cap [2^cap_height][4]) of an LDE given column-major in natural order, under `hasher`."""
        v = np.ascontiguousarray(lde_colmajor, dtype=np.uint64)
        ncols, N = v.shape
        digests = np.zeros((N, 4), dtype=np.uint64)
        cap = np.zeros((1 << cap_height, 4), dtype=np.uint64)
        _chk(lib.starkhip_merkle_tree_hasher(self._ctx, hasher, _p64(v), ncols, N.bit_length() - 1, cap_height, _p64(digests), _p64(cap)))
        return digests, cap

    def hash_rows(self, rows, hasher=HASHER_POSEIDON):
        """Digests [n_leaves][4] of row-major leaves [n_leaves][width] under `hasher`, as the FRI layers are hashed."""
        r = np.ascontiguousarray(rows, dtype=np.uint64)
        assert r.ndim == 2
        out = np.zeros((r.shape[0], 4), dtype=np.uint64)
        _chk(lib.starkhip_hash_rows_hasher(self._ctx, hasher, _p64(r), r.shape[1], r.shape[0], _p64(out)))
        return out

    def keccak_permute_batch(self, states):
        """The Keccak hasher's challenger permutation of every row of `states` (n x 12) on the device."""
        s = np.ascontiguousarray(states, dtype=np.uint64).copy()
        assert s.ndim == 2 and s.shape[1] == 12
        _chk(lib.starkhip_keccak_permute_batch(self._ctx, _p64(s), s.shape[0]))
        return s

    def field_ops(self, op, a, b):
        """Device field arithmetic under test (kernels_selftest.hip): canonical(op(a[i], b[i]))."""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        b = np.ascontiguousarray(b, dtype=np.uint64)
        assert a.shape == b.shape and a.ndim == 1
        out = np.zeros_like(a)
        _chk(lib.starkhip_field_ops_batch(self._ctx, op, _p64(a), _p64(b), _p64(out), a.size))
        return out

    def leaf_hash_lane_group(self, mats, log_n, rate_bits=0, grouped=True, form=3, prefix_mask=0):
        """Leaf digests (segments x leaves x 4, tree order) of `mats` (segments x columns x leaves, coset-major) in the lane form of the leaf
        hash: as ONE grid over all segments (grouped, what a proof pool launches for a group) or one launch per segment -- those also in
        the pair form (form=4).  prefix_mask bit s: segment s gets the context's saved state past an identity prefix
        ("leaf_hash_prefix") and the counter the context's last lde_batch of this shape left."""
        m = np.ascontiguousarray(mats, dtype=np.uint64)
        assert m.ndim == 3
        out = np.zeros((m.shape[0], m.shape[2], 4), dtype=np.uint64)
        if m.shape[2] != 1 << (log_n + rate_bits):
            raise StarkhipError(ERR_BAD_SHAPE)
        _chk(lib.starkhip_leaf_hash_lane_group(self._ctx, _p64(m), m.shape[0], m.shape[1], log_n, rate_bits, 1 if grouped else 0, form, prefix_mask, _p64(out)))
        return out

    def leaf_prefix_table(self, log_n, rate_bits):
        """starkhip_leaf_prefix_table: cap[4][N], the sponge capacity of every leaf (coset-major index) after the columns e_0 .. e_{n-1}."""
        out = np.zeros((4, 1 << (log_n + rate_bits)), dtype=np.uint64)
        _chk(lib.starkhip_leaf_prefix_table(self._ctx, log_n, rate_bits, _p64(out)))
        return out

    def poseidon_permute_batch(self, states, form=0, variant=0):
        """The permutation of every row of `states` (n x 12).  form: 0 the generic device loop, 1 .. 4 the quad, row, lane and pair forms of
        the leaf hash, each through the function its leaf kernel calls; variant 1 (quad, lane, pair): the form with the capacity-only last
        round, which specifies words 8 .. 11 (pair: 2 .. 5 and 8 .. 11) and returns the other words unchanged."""
        s = np.ascontiguousarray(states, dtype=np.uint64).copy()
        assert s.ndim == 2 and s.shape[1] == 12
        if form == 0 and variant == 0:
            _chk(lib.starkhip_poseidon_permute_batch(self._ctx, _p64(s), s.shape[0]))
        else:
            _chk(lib.starkhip_poseidon_permute_batch_form(self._ctx, form, variant, _p64(s), s.shape[0]))
        return s

    def verify_batch(self, items):
        """starkhip_verify_batch: `items` = [(air, config, proof), ...] -> the code starkhip_verify gives each proof (0 = accepted),
        with the query rounds on this context's device.  A failed call (HIP, out of memory) raises StarkhipError."""
        return _verify_batch(items, self._ctx)

    def verify_stark_proof_device(self, air, config, proof):
        """verify_stark_proof with the query rounds on the device; raises StarkhipError on rejection, like verify_stark_proof."""
        _chk(self.verify_batch([(air, config, proof)])[0])

    def last_verify_timings(self):
        """The last verify_batch: {"prelude_ms", "upload_ms", "device_ms", "cpu_s"} (cpu_s: the process's CPU seconds in the call)."""
        out = (C.c_double * 4)()
        _chk(lib.starkhip_last_verify_timings(self._ctx, out))
        return dict(zip(("prelude_ms", "upload_ms", "device_ms", "cpu_s"), list(out)))


# ----------------------------------------------------------------------------- proof pool (submit / wait)
class PoolConfig(C.Structure):
    """starkhip_pool_config_t (0 = the library's default)."""
    _fields_ = [("device", C.c_int), ("big_contexts", C.c_uint), ("small_contexts", C.c_uint), ("generator_threads", C.c_uint),
                ("trace_threads", C.c_uint), ("commit_policy", C.c_uint), ("stream_priority", C.c_uint), ("warm_up", C.c_uint), ("gather_ms", C.c_float)]


class TicketInfo(C.Structure):
    _fields_ = [("phase_ms", C.c_float * N_PHASES), ("kernel_ms", C.c_float * 3), ("host_ms", C.c_float * 2), ("t_submit", C.c_double), ("t_generate_start", C.c_double),
                ("t_generate_end", C.c_double), ("t_prove_start", C.c_double), ("t_done", C.c_double), ("leaf_hash_form", C.c_int),
                ("leaf_hash_group", C.c_uint)]


class PoolStats(C.Structure):
    _fields_ = [(n, C.c_ulong) for n in ("big_commit_launches", "small_commit_launches", "small_commit_requests", "max_merged_commitments", "big_commit_grids")]


lib.starkhip_pool_create.argtypes = [C.POINTER(PoolConfig), C.POINTER(C.c_void_p)]
lib.starkhip_pool_destroy.argtypes = [C.c_void_p]
lib.starkhip_pool_destroy.restype = None
lib.starkhip_pool_submit.argtypes = [C.c_void_p, C.c_int, C.POINTER(StarkConfig), C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _u64p,
                                     C.c_size_t, C.c_uint64, C.POINTER(C.c_uint64)]
lib.starkhip_pool_submit_compact.argtypes = [C.c_void_p, C.c_int, C.POINTER(StarkConfig), C.c_void_p, _u64p, C.c_size_t, C.c_uint64,
                                             C.POINTER(C.c_uint64)]
lib.starkhip_pool_submit_witness.argtypes = [C.c_void_p, C.c_int, C.POINTER(StarkConfig), _u32p, C.c_size_t, C.c_uint64, C.POINTER(C.c_uint64)]
lib.starkhip_pool_wait.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(_u64p), C.POINTER(C.c_size_t), C.POINTER(TicketInfo)]
lib.starkhip_pool_stats.argtypes = [C.c_void_p, C.POINTER(PoolStats)]
lib.starkhip_pool_submit_columns.argtypes = [C.c_void_p, C.c_int, C.POINTER(StarkConfig), C.POINTER(C.c_void_p), C.c_size_t, C.c_size_t, _u64p, C.c_size_t,
                                             C.c_uint64, C.POINTER(C.c_uint64)]


class PoolReservation(C.Structure):
    _fields_ = [("device_bytes", C.c_uint64), ("pinned_host_bytes", C.c_uint64), ("big_context_device_bytes", C.c_uint64),
                ("small_context_device_bytes", C.c_uint64), ("big_contexts", C.c_uint), ("small_contexts", C.c_uint)]


lib.starkhip_pool_reservation.argtypes = [C.c_void_p, C.POINTER(PoolReservation)]
# a pool per device behind one handle (starkhip_multipool_*): the same submits with a `slot` argument after the handle
lib.starkhip_multipool_create.argtypes = [C.POINTER(C.c_int), C.c_size_t, C.POINTER(PoolConfig), C.POINTER(C.c_void_p)]
lib.starkhip_multipool_destroy.argtypes = [C.c_void_p]
lib.starkhip_multipool_destroy.restype = None
lib.starkhip_multipool_size.argtypes = [C.c_void_p]
lib.starkhip_multipool_size.restype = C.c_size_t
lib.starkhip_multipool_pool.argtypes = [C.c_void_p, C.c_size_t]
lib.starkhip_multipool_pool.restype = C.c_void_p
lib.starkhip_multipool_device.argtypes = [C.c_void_p, C.c_size_t]
lib.starkhip_multipool_submit.argtypes = [C.c_void_p, C.c_int] + lib.starkhip_pool_submit.argtypes[1:]
lib.starkhip_multipool_submit_compact.argtypes = [C.c_void_p, C.c_int] + lib.starkhip_pool_submit_compact.argtypes[1:]
lib.starkhip_multipool_submit_witness.argtypes = [C.c_void_p, C.c_int] + lib.starkhip_pool_submit_witness.argtypes[1:]
lib.starkhip_multipool_submit_columns.argtypes = [C.c_void_p, C.c_int] + lib.starkhip_pool_submit_columns.argtypes[1:]
lib.starkhip_multipool_submit_witness_batch.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(_u32p), C.POINTER(C.c_size_t), C.c_uint64,
                                                        C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
lib.starkhip_multipool_ticket_slot.argtypes = [C.c_void_p, C.c_uint64]
lib.starkhip_multipool_wait.argtypes = lib.starkhip_pool_wait.argtypes
lib.starkhip_plan_lpt.argtypes = [C.c_size_t, C.POINTER(C.c_int), C.c_size_t, C.POINTER(C.c_int)]
lib.starkhip_air_cost.argtypes = [C.c_int]
lib.starkhip_air_cost.restype = C.c_double
# the pool's verifier (starkhip_pool_set_option "verify_proofs", starkhip_pool_submit_verify)
class PoolVerifyStats(C.Structure):
    _fields_ = [(n, C.c_ulong) for n in ("proofs_checked", "verify_jobs", "rejected", "device_batches")] + \
               [(n, C.c_double) for n in ("upload_ms", "device_ms", "prelude_ms", "prelude_cpu_s")] + [("arena_bytes", C.c_uint64)]


lib.starkhip_pool_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
lib.starkhip_pool_submit_verify.argtypes = [C.c_void_p, C.c_int, C.POINTER(StarkConfig), _u64p, C.c_size_t, C.POINTER(C.c_uint64)]
lib.starkhip_pool_verify_stats.argtypes = [C.c_void_p, C.POINTER(PoolVerifyStats)]
lib.starkhip_multipool_set_option.argtypes = lib.starkhip_pool_set_option.argtypes
lib.starkhip_multipool_submit_verify.argtypes = [C.c_void_p, C.c_int] + lib.starkhip_pool_submit_verify.argtypes[1:]
lib.starkhip_multipool_verify_batch.argtypes = [C.c_void_p] + _verify_batch_args
lib.starkhip_plan_verify.argtypes = [C.c_size_t, C.POINTER(C.c_int), C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
lib.starkhip_air_verify_cost.argtypes = [C.c_int]
lib.starkhip_air_verify_cost.restype = C.c_double
lib.starkhip_hw_queues_status.argtypes = []
lib.starkhip_hw_queues_in_effect.argtypes = []


def plan_lpt(airs, n_pools):
    """starkhip_plan_lpt: the slot each job of a batch gets on `n_pools` idle pools (longest processing time first)."""
    a = (C.c_int * len(airs))(*[int(x) for x in airs])
    out = (C.c_int * len(airs))()
    _chk(lib.starkhip_plan_lpt(len(airs), a, n_pools, out))
    return [int(x) for x in out]


def air_cost(air):
    return float(lib.starkhip_air_cost(int(air)))


def hw_queues_late():
    """True when the HIP runtime was up before the first pool could ask for its hardware queues (starkhip_hw_queues_status)."""
    return bool(lib.starkhip_hw_queues_status())


def hw_queues_in_effect():
    """Hardware queues per stream priority class this process really has (starkhip_hw_queues_in_effect): GPU_MAX_HW_QUEUES as it was in the
    environment before the HIP runtime came up, 4 when it came late; 0 before the first pool of the process."""
    return int(lib.starkhip_hw_queues_in_effect())


class PoolHostInfo(C.Structure):
    _fields_ = [(n, C.c_uint) for n in ("cpu_budget", "generator_threads", "trace_threads_big", "trace_threads_small", "prover_threads")] + [("device", C.c_int), ("pools_on_device", C.c_uint)] + \
               [("hw_queues", C.c_uint), ("stream_budget", C.c_uint)]


lib.starkhip_pool_host_info.argtypes = [C.c_void_p, C.POINTER(PoolHostInfo)]
lib.starkhip_host_cpu_seconds.argtypes = [C.POINTER(C.c_double)]
lib.starkhip_host_cpu_seconds.restype = None
lib.starkhip_cpu_budget.argtypes = []
lib.starkhip_cpu_budget.restype = C.c_uint
lib.starkhip_proof_blob_stats.argtypes = [C.POINTER(C.c_uint64)]
lib.starkhip_proof_blob_stats.restype = None


def host_cpu_seconds():
    """starkhip_host_cpu_seconds: cumulative CPU seconds of the pools' host work -- {"recording", "proving"}."""
    out = (C.c_double * 3)()
    lib.starkhip_host_cpu_seconds(out)
    return {"recording": float(out[0]), "proving": float(out[1]), "of_proving_in_device_waits": float(out[2])}


def proof_blob_stats():
    """Process-wide counters of the recycled page-locked proof blobs (starkhip_proof_blob_stats)."""
    out = (C.c_uint64 * 5)()
    lib.starkhip_proof_blob_stats(out)
    return dict(zip(("blobs", "busy", "bytes", "taken", "missed"), [int(x) for x in out]))


def witness_operands(air, *args):
    """The packed u32 operand vector `starkhip_pool_submit_witness` takes for `air` from the arguments of its `trace_*`
    generator (starkhip.h has the layouts)."""
    if air == AIR_FP12_MUL:
        parts = [_limbs(args[0], 144), _limbs(args[1], 144)]
    elif air == AIR_FINAL_EXP:
        parts = [_limbs(args[0], 144)]
    elif air == AIR_MILLER_LOOP:
        parts = [_limbs(args[0], 12), _limbs(args[1], 12), _limbs(args[2], 24), _limbs(args[3], 24), _limbs(args[4], 24)]
    elif air == AIR_PAIRING_PRECOMP:
        parts = [_limbs(args[0], 24), _limbs(args[1], 24), _limbs(args[2], 24)]
    elif air == AIR_ECC_AGGREGATE:
        pts, b = _ecc_inputs(args[0], args[1])
        parts = [pts, b.astype(np.uint32)]
    elif air == AIR_TEST_FIBONACCI:
        x0, x1 = int(args[0]), int(args[1])
        parts = [np.array([x0 & 0xFFFFFFFF, x0 >> 32, x1 & 0xFFFFFFFF, x1 >> 32], dtype=np.uint32)]
    else:
        raise StarkhipError(ERR_BAD_AIR)
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.uint32)


class ProofPool:
    """starkhip_pool_*: the library's own scheduler of many proofs on one GPU -- prover contexts with a host thread each,
    generator threads, merged trace commitments for the small AIRs.  The caller side of the reference's six-proof sequence
    (src/aggregate_proof.rs:304-370) only submits and waits:

        t = pool.submit_witness(AIR_MILLER_LOOP, px, py, qx, qy, qz)     # generate_trace + prove, both inside the pool
        proof, info = pool.wait(t)
    """

    def __init__(self, device=0, big_contexts=0, small_contexts=0, generator_threads=0, trace_threads=0, commit_policy=0, gather_ms=0.0,
                 stream_priority=0, warm_up=0, devices=None, verify_proofs=False, verify_arena_mb=0):
        """`devices` (a list of ordinals, one pool each; an ordinal may repeat): ONE process on several GPUs through
        starkhip_multipool_* -- the submits then take `slot` (-1: the library places the job, longest processing time first).
        `verify_proofs`: every proof is checked by the pool's device verifier before wait returns it; `verify_arena_mb` (0: the
        library's default) sizes that verifier's device memory."""
        cfg = PoolConfig(device, big_contexts, small_contexts, generator_threads, trace_threads, commit_policy, stream_priority, warm_up, gather_ms)
        self._h = C.c_void_p()
        self._multi = devices is not None
        if self._multi:
            devs = (C.c_int * len(devices))(*[int(d) for d in devices])
            _chk(lib.starkhip_multipool_create(devs, len(devices), C.byref(cfg), C.byref(self._h)))
        else:
            _chk(lib.starkhip_pool_create(C.byref(cfg), C.byref(self._h)))
        self._keep = {}  # ticket -> inputs that must outlive the proof
        self._verify_tickets = set()
        try:
            if verify_arena_mb:
                self.set_option("verify_arena_mb", verify_arena_mb)
            if verify_proofs:
                self.set_option("verify_proofs", 1)
        except StarkhipError:
            self.close()
            raise

    def set_option(self, name, value):
        """starkhip_pool_set_option on every pool of the handle: "verify_proofs" (0 / 1), "verify_arena_mb", "check_traces" (0 / 1: wait
        raises TraceViolation for a trace that violates its AIR), "check_trace_list", "fill_lookups" (0 / 1: the permuted columns of an AIR
        registered with its lookups are filled by the proving context; wait raises TraceViolation with the lookup blob when one fails),
        "fill_frequencies" (0 / 1: the same for the frequencies columns of a fillable AIR's LogUp lookups; the LogUp blob), "hasher" (HASHER_POSEIDON / HASHER_KECCAK: the
        hasher of the proving tickets submitted from then on)."""
        if self._multi:
            _chk(lib.starkhip_multipool_set_option(self._h, name.encode(), int(value)))
        else:
            _chk(lib.starkhip_pool_set_option(self._h, name.encode(), int(value)))

    def submit_verify(self, air, proof, config=None, slot=-1):
        """A verification job for any proof (starkhip_pool_submit_verify); wait(ticket) returns starkhip_verify's code for it."""
        p = np.ascontiguousarray(proof, dtype=np.uint64)
        cfg = StarkConfig.from_buffer_copy(config) if config is not None else None
        t = C.c_uint64()
        _chk(self._call("submit_verify", slot, air, C.byref(cfg) if cfg is not None else None, _p64(p), p.size, C.byref(t)))
        self._keep[t.value] = (p, cfg)
        self._verify_tickets.add(t.value)
        return t.value

    def verify_batch(self, items):
        """`items` = [(air, config, proof), ...] -> the code starkhip_verify gives each proof.  On several devices
        starkhip_multipool_verify_batch (longest first over the devices); on one pool every proof is submitted, then waited for."""
        items = list(items)
        if self._multi:
            n = len(items)
            keep = [np.ascontiguousarray(p, dtype=np.uint64) for _, _, p in items]
            airs = (C.c_int * max(n, 1))(*[int(a) for a, _, _ in items])
            cfgs = (StarkConfig * max(n, 1))(*[c for _, c, _ in items])
            ptrs = (_u64p * max(n, 1))(*[_p64(p) for p in keep])
            words = (C.c_size_t * max(n, 1))(*[p.size for p in keep])
            res = (C.c_int * max(n, 1))()
            _chk(lib.starkhip_multipool_verify_batch(self._h, n, airs, cfgs, ptrs, words, res))
            return [int(r) for r in res[:n]]
        tickets = [self.submit_verify(a, p, c) for a, c, p in items]
        return [self.wait(t) for t in tickets]

    def verify_stats(self):
        """starkhip_pool_verify_stats summed over the handle's pools (arena_bytes too)."""
        out = None
        for h in self._pools():
            r = PoolVerifyStats()
            _chk(lib.starkhip_pool_verify_stats(h, C.byref(r)))
            one = {n: (float if t is C.c_double else int)(getattr(r, n)) for n, t in PoolVerifyStats._fields_}
            out = one if out is None else {n: out[n] + one[n] for n in out}
        return out

    def check_stats(self, per_pool=False):
        """starkhip_pool_check_stats: {"checked", "rejected"} summed over the handle's pools, or one dict per pool."""
        each = []
        for h in self._pools():
            out = np.zeros(2, dtype=np.uint64)
            _chk(lib.starkhip_pool_check_stats(h, _p64(out)))
            each.append({"checked": int(out[0]), "rejected": int(out[1])})
        return each if per_pool else {n: sum(e[n] for e in each) for n in each[0]}

    def _call(self, name, slot, *args):
        if self._multi:
            return getattr(lib, "starkhip_multipool_" + name)(self._h, slot, *args)
        return getattr(lib, "starkhip_pool_" + name)(self._h, *args)

    @property
    def n_pools(self):
        return int(lib.starkhip_multipool_size(self._h)) if self._multi else 1

    def slot_of(self, ticket):
        return int(lib.starkhip_multipool_ticket_slot(self._h, ticket)) if self._multi else 0

    def _pools(self):
        return [C.c_void_p(lib.starkhip_multipool_pool(self._h, k)) for k in range(self.n_pools)] if self._multi else [self._h]

    def close(self):
        if self._h:
            (lib.starkhip_multipool_destroy if self._multi else lib.starkhip_pool_destroy)(self._h)
            self._h = C.c_void_p()
            self._keep.clear()
            self._verify_tickets.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def submit(self, air, config, trace, public_inputs, pow_witness=POW_SEARCH, layout=0, slot=-1):
        """As Prover.prove, asynchronously: `trace` a host array or a CompactTrace.  Returns the ticket."""
        pis = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        cfg = StarkConfig.from_buffer_copy(config)
        t = C.c_uint64()
        if isinstance(trace, CompactTrace):
            _chk(self._call("submit_compact", slot, air, C.byref(cfg), trace._h, _p64(pis), pis.size, pow_witness, C.byref(t)))
        else:
            trace = np.ascontiguousarray(trace, dtype=np.uint64)
            if trace.ndim != 2 or layout not in (0, 1):
                raise StarkhipError(ERR_BAD_SHAPE)
            n_rows, n_cols = trace.shape if layout == 0 else trace.shape[::-1]
            _chk(self._call("submit", slot, air, C.byref(cfg), trace.ctypes.data_as(C.c_void_p), n_rows, n_cols, layout, 0, _p64(pis), pis.size,
                            pow_witness, C.byref(t)))
        self._keep[t.value] = (trace, pis, cfg)
        return t.value

    def submit_device(self, air, config, trace_ptr, n_rows, public_inputs, pow_witness=POW_SEARCH, layout=1, slot=0):
        """`trace_ptr`: device address of a uint64 trace already resident in HBM (benchmark path); on several devices `slot` names
        the pool of the device the trace lives on."""
        pis = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        cfg = StarkConfig.from_buffer_copy(config)
        t = C.c_uint64()
        _chk(self._call("submit", slot, air, C.byref(cfg), C.c_void_p(trace_ptr), n_rows, air_columns(air), layout, 1, _p64(pis), pis.size,
                        pow_witness, C.byref(t)))
        self._keep[t.value] = (pis, cfg)
        return t.value

    def submit_columns(self, air, config, columns, public_inputs, pow_witness=POW_SEARCH, slot=-1):
        """As Prover.prove_columns, asynchronously: one separately allocated array per trace column."""
        table, keep, n_rows = _column_table(columns)
        pis = np.ascontiguousarray(public_inputs, dtype=np.uint64)
        cfg = StarkConfig.from_buffer_copy(config)
        t = C.c_uint64()
        _chk(self._call("submit_columns", slot, air, C.byref(cfg), table, n_rows, len(keep), _p64(pis), pis.size, pow_witness, C.byref(t)))
        self._keep[t.value] = (keep, pis, cfg)  # the table itself was copied by the library
        return t.value

    def submit_witness(self, air, *generator_args, config=None, pow_witness=POW_SEARCH, slot=-1):
        """generate_trace + prove inside the pool, from the arguments of `trace_<air>`."""
        ops = witness_operands(air, *generator_args)
        t = C.c_uint64()
        cfgp = C.byref(StarkConfig.from_buffer_copy(config)) if config is not None else None
        _chk(self._call("submit_witness", slot, air, cfgp, _p32(ops), ops.size, pow_witness, C.byref(t)))
        return t.value

    def submit_witness_batch(self, jobs, pow_witness=POW_SEARCH):
        """jobs: [(air, generator args...)]; on several devices the batch is placed longest processing time first
        (starkhip_multipool_submit_witness_batch), on one pool in the given order.  Returns the tickets in the jobs' order."""
        ops = [witness_operands(j[0], *j[1:]) for j in jobs]
        if not self._multi:
            out = []
            for j, o in zip(jobs, ops):
                t = C.c_uint64()
                _chk(lib.starkhip_pool_submit_witness(self._h, j[0], None, _p32(o), o.size, pow_witness, C.byref(t)))
                out.append(t.value)
            return out
        n = len(jobs)
        airs = (C.c_int * n)(*[int(j[0]) for j in jobs])
        ptrs = (_u32p * n)(*[_p32(o) for o in ops])
        lens = (C.c_size_t * n)(*[o.size for o in ops])
        tickets = (C.c_uint64 * n)()
        rcs = (C.c_int * n)()
        rc = lib.starkhip_multipool_submit_witness_batch(self._h, n, airs, ptrs, lens, pow_witness, tickets, rcs)
        if rc != 0:
            # the call is not all-or-nothing: the jobs it accepted are running.  Wait for them and drop their proofs before the error
            # goes up (the Rust binding does the same by building its tickets first) -- a ticket nobody holds could never be freed
            for t in tickets:
                if int(t):
                    out, words, info = _u64p(), C.c_size_t(), TicketInfo()
                    if lib.starkhip_multipool_wait(self._h, int(t), C.byref(out), C.byref(words), C.byref(info)) == 0:
                        lib.starkhip_free(out)
            _chk(rc)
        return [int(t) for t in tickets]

    def wait(self, ticket, keep=True):
        """(proof, info) of `ticket`; raises StarkhipError with the proof's status if it failed (TraceViolation, with the report, for a
        trace the pool's "check_traces" refused).  info: phase_ms / kernel_ms
        dicts and the job's timeline in seconds since the pool was created."""
        out = _u64p()
        words = C.c_size_t()
        info = TicketInfo()
        rc = (lib.starkhip_multipool_wait if self._multi else lib.starkhip_pool_wait)(self._h, ticket, C.byref(out), C.byref(words), C.byref(info))
        self._keep.pop(ticket, None)
        if ticket in self._verify_tickets:  # a verify job: its verdict (a failure of the device work still raises)
            self._verify_tickets.discard(ticket)
            if rc in (ERR_HIP, ERR_OOM, ERR_NO_DEVICE):
                _chk(rc)
            return rc
        proof = _take_blob(rc, out, words, keep)
        return proof, {"phase_ms": dict(zip(PHASE_NAMES, [float(x) for x in info.phase_ms])),
                       "kernel_ms": {"lde_columns": float(info.kernel_ms[0]), "leaf_hash": float(info.kernel_ms[1]), "quotient_eval": float(info.kernel_ms[2])},
                       "host_ms": {"fiat_shamir": float(info.host_ms[0]), "other": float(info.host_ms[1])},
                       "timeline_s": [info.t_submit, info.t_generate_start, info.t_generate_end, info.t_prove_start, info.t_done],
                       "leaf_hash_form": ("quad", "row", "merged", "lane", "host", "pair", "keccak")[min(info.leaf_hash_form, 6)],
                       "leaf_hash_form_id": int(info.leaf_hash_form), "leaf_hash_group": int(info.leaf_hash_group)}

    def reservation(self):
        """starkhip_pool_reservation: what the pool's contexts hold (bytes; summed over the devices' pools, the per-context figures the largest)."""
        out = None
        for h in self._pools():
            r = PoolReservation()
            _chk(lib.starkhip_pool_reservation(h, C.byref(r)))
            one = {n: int(getattr(r, n)) for n, _ in PoolReservation._fields_}
            if out is None:
                out = one
            else:
                for n in one:
                    out[n] = max(out[n], one[n]) if n.endswith("context_device_bytes") else out[n] + one[n]
        return out

    def host_info(self):
        """starkhip_pool_host_info of every pool behind this handle: the CPUs it plans with and its host threads."""
        out = []
        for h in self._pools():
            r = PoolHostInfo()
            _chk(lib.starkhip_pool_host_info(h, C.byref(r)))
            out.append({n: int(getattr(r, n)) for n, _ in PoolHostInfo._fields_})
        return out

    def stats(self, per_pool=False):
        each = []
        for h in self._pools():
            s = PoolStats()
            _chk(lib.starkhip_pool_stats(h, C.byref(s)))
            each.append({n: int(getattr(s, n)) for n, _ in PoolStats._fields_})
        if per_pool:
            return each
        return {n: (max if n == "max_merged_commitments" else sum)(e[n] for e in each) for n in each[0]}


def verify_stark_proof(air, config, proof):
    """Mirror of starky::verifier::verify_stark_proof; raises StarkhipError on rejection."""
    p = np.ascontiguousarray(proof, dtype=np.uint64)
    _chk(lib.starkhip_verify(air, C.byref(config), _p64(p), p.size))


def _verify_batch(items, ctx=None, replay=False):
    items = list(items)
    n = len(items)
    keep = [np.ascontiguousarray(p, dtype=np.uint64) for _, _, p in items]
    airs = (C.c_int * max(n, 1))(*[int(a) for a, _, _ in items])
    cfgs = (StarkConfig * max(n, 1))(*[c for _, c, _ in items])
    ptrs = (_u64p * max(n, 1))(*[_p64(p) for p in keep])
    words = (C.c_size_t * max(n, 1))(*[p.size for p in keep])
    res = (C.c_int * max(n, 1))()
    if replay:
        _chk(lib.starkhip_verify_batch_replay(n, airs, cfgs, ptrs, words, res))
    else:
        _chk(lib.starkhip_verify_batch(ctx, n, airs, cfgs, ptrs, words, res))
    return [int(r) for r in res[:n]]


def verify_batch_replay(items):
    """starkhip_verify_batch_replay (tests): the device verifier's host side with its device part replayed on the CPU."""
    return _verify_batch(items, replay=True)


def check_trace_report_replay(air, trace, public_inputs, layout=0, cap=1024):
    """starkhip_check_trace_report_replay (tests, small shapes): Prover.check_trace_report's host side with the two device passes
    replayed on the CPU; no device needed."""
    trace = np.ascontiguousarray(trace, dtype=np.uint64)
    if trace.ndim != 2 or layout not in (0, 1):
        raise StarkhipError(ERR_BAD_SHAPE)
    n_rows, n_cols = trace.shape if layout == 0 else trace.shape[::-1]
    pis = np.ascontiguousarray(public_inputs, dtype=np.uint64)
    if pis.size != air_public_inputs(air):
        raise StarkhipError(ERR_BAD_SHAPE)
    return _check_trace_report(lambda *out: lib.starkhip_check_trace_report_replay(air, trace.ctypes.data_as(C.c_void_p), n_rows, n_cols, layout,
                                                                                   _p64(pis), *out), air, n_rows, cap)


def free_cells_replay(air, trace, public_inputs, layout=0, delta=DEFAULT_DELTA, mask=True):
    """starkhip_check_trace_free_cells_replay (tests, small shapes): Prover.free_cells' rule as host loops; no device needed."""
    trace = np.ascontiguousarray(trace, dtype=np.uint64)
    if trace.ndim != 2 or layout not in (0, 1):
        raise StarkhipError(ERR_BAD_SHAPE)
    n_rows, n_cols = trace.shape if layout == 0 else trace.shape[::-1]
    pis, delta = _free_cells_args(air, public_inputs, delta)
    return _free_cells(lambda *out: lib.starkhip_check_trace_free_cells_replay(air, trace.ctypes.data_as(C.c_void_p), n_rows, n_cols, layout,
                                                                               _p64(pis), delta, *out), n_rows, n_cols, mask)


def free_cell_classes_replay(air, trace, public_inputs, layout=0, delta=DEFAULT_DELTA, planes=True):
    """starkhip_check_trace_free_cell_classes_replay (tests, small shapes): Prover.free_cell_classes' rule as host loops; no device needed."""
    trace = np.ascontiguousarray(trace, dtype=np.uint64)
    if trace.ndim != 2 or layout not in (0, 1):
        raise StarkhipError(ERR_BAD_SHAPE)
    n_rows, n_cols = trace.shape if layout == 0 else trace.shape[::-1]
    pis, delta = _free_cells_args(air, public_inputs, delta)
    return _free_cell_classes(lambda *out: lib.starkhip_check_trace_free_cell_classes_replay(air, trace.ctypes.data_as(C.c_void_p), n_rows, n_cols,
                                                                                             layout, _p64(pis), delta, *out),
                              air, n_rows, n_cols, planes)


def trace_rows_to_poly_values(trace_rows):
    """starky::util::trace_rows_to_poly_values: row-major [n][C] -> column-major [C][n]."""
    return np.ascontiguousarray(np.asarray(trace_rows, dtype=np.uint64).T)


# ---- cross-table lookups: several registered AIRs proved and verified as one system (COMPAT.md §2d; air_builder.SystemBuilder makes the blob)
SYSTEM_PROOF_MAGIC = 0x31304650535953  # "SYSPF01"
SYSTEM_MAX_TABLES = 64  # STARKHIP_SYSTEM_MAX_TABLES
lib.starkhip_ctl_span_rows.restype = C.c_uint
lib.starkhip_ctl_span_rows.argtypes = []
CTL_SPAN_ROWS = int(lib.starkhip_ctl_span_rows())  # the rows one workgroup of the running sums' scan takes: the scan's own constant
_szp = C.POINTER(C.c_size_t)
_intp = C.POINTER(C.c_int)
lib.starkhip_system_check.argtypes = [_u64p, C.c_size_t, C.c_char_p, C.c_size_t]
lib.starkhip_system_register.argtypes = [_u64p, C.c_size_t, _intp]
lib.starkhip_system_tables.argtypes = [C.c_int]
lib.starkhip_system_ctls.argtypes = [C.c_int]
lib.starkhip_system_table_air.argtypes = [C.c_int, C.c_size_t]
lib.starkhip_system_table_endpoints.argtypes = [C.c_int, C.c_size_t]
lib.starkhip_system_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
lib.starkhip_system_destroy.argtypes = [C.c_void_p]
lib.starkhip_system_destroy.restype = None
lib.starkhip_system_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_long]
lib.starkhip_system_last_timings.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_float)]
lib.starkhip_system_prove.argtypes = [C.c_void_p, C.POINTER(StarkConfig), C.POINTER(C.c_void_p), _szp, _intp, _intp, C.POINTER(_u64p), _szp, C.c_uint64,
                                      C.POINTER(_u64p), _szp, _intp]
lib.starkhip_system_verify.argtypes = [C.c_int, C.POINTER(StarkConfig), _u64p, C.c_size_t]
lib.starkhip_system_proof_layout.argtypes = [_u64p, C.c_size_t, _szp, _szp, C.c_size_t]
lib.starkhip_ctl_polys.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _u64p, _u64p, _u64p, _u64p]
lib.starkhip_ctl_polys_replay.argtypes = [C.c_int, C.c_size_t, _u64p, C.c_size_t, C.c_size_t, C.c_int, _u64p, _u64p, _u64p, _u64p]
lib.starkhip_system_eval_frame_ctl.argtypes = [C.c_int, C.c_size_t, _u64p, _u64p, _u64p, _u64p, _u64p, C.c_int, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p]


class SystemRefused(StarkhipError):
    """SystemProver.prove: some CTL's sums do not balance, or a denominator was zero (ERR_QUOTIENT_NOT_DIVISIBLE); `.ctl` is the CTL."""

    def __init__(self, ctl):
        super().__init__(ERR_QUOTIENT_NOT_DIVISIBLE)
        self.ctl = ctl


def system_check(blob):
    """The validator starkhip_system_register runs: None for a system it accepts, else the reason it refuses it."""
    blob = np.ascontiguousarray(blob, dtype=np.uint64)
    why = C.create_string_buffer(512)
    rc = lib.starkhip_system_check(_p64(blob), blob.size, why, len(why))
    if rc == 0:
        return None
    if rc != ERR_BAD_AIR:
        raise StarkhipError(rc)
    return why.value.decode()


def register_system(blob):
    """Register a system blob (air_builder.SystemBuilder.finish()) and return its id; the same blob again returns the same id.  A system
    the validator refuses raises StarkhipError(ERR_BAD_AIR)."""
    blob = np.ascontiguousarray(blob, dtype=np.uint64)
    out = C.c_int()
    _chk(lib.starkhip_system_register(_p64(blob), blob.size, C.byref(out)))
    return out.value


def _nonneg(r):
    if r < 0:
        raise StarkhipError(r)
    return r


def system_tables(system):
    """the AIR ids of the system's tables, in table order"""
    return [_nonneg(lib.starkhip_system_table_air(system, t)) for t in range(_nonneg(lib.starkhip_system_tables(system)))]


def system_ctls(system):
    return _nonneg(lib.starkhip_system_ctls(system))


def system_table_endpoints(system, table):
    """E_t: the CTL endpoints table `table` carries; its proof has nC = 4 E_t polynomials and 2 E_t sums"""
    return _nonneg(lib.starkhip_system_table_endpoints(system, table))


def system_proof_tables(proof):
    """The table proofs of a system proof blob, in table order (views of `proof`); StarkhipError(ERR_BAD_SHAPE) for anything else."""
    p = np.ascontiguousarray(proof, dtype=np.uint64)
    n = C.c_size_t()
    off = (C.c_size_t * (SYSTEM_MAX_TABLES + 1))()
    _chk(lib.starkhip_system_proof_layout(_p64(p), p.size, C.byref(n), off, SYSTEM_MAX_TABLES + 1))
    return [p[off[t]:off[t + 1]] for t in range(n.value)]


def system_proof_join(table_proofs):
    """a system proof blob from table proofs (tests: tampered copies)"""
    T = len(table_proofs)
    offs, at = [], 3 + T
    for p in table_proofs:
        offs.append(at)
        at += len(p)
    return np.concatenate([np.array([SYSTEM_PROOF_MAGIC, T] + offs + [at], dtype=np.uint64)] + [np.asarray(p, dtype=np.uint64) for p in table_proofs])


def verify_system_proof(system, configs, proof):
    """starkhip_system_verify: the system transcript replayed from the table proofs' trace caps, every table proof from the copied state,
    every CTL's sum equation; raises StarkhipError on rejection.  configs: one StarkConfig per table (they may differ in rate_bits only)."""
    p = np.ascontiguousarray(proof, dtype=np.uint64)
    cfgs = (StarkConfig * len(configs))(*configs)
    _chk(lib.starkhip_system_verify(system, cfgs, _p64(p), p.size))


def _ctl_args(system, table, n_rows, challenges):
    challenges = np.ascontiguousarray(challenges, dtype=np.uint64).reshape(-1)
    if challenges.size != 4:
        raise StarkhipError(ERR_BAD_SHAPE)
    E = system_table_endpoints(system, table)
    return challenges, np.zeros((4 * E, n_rows), dtype=np.uint64), np.zeros(2 * E, dtype=np.uint64), np.zeros(1, dtype=np.uint64)


def ctl_polys_replay(system, table, trace, challenges, layout=0):
    """The CTL polynomials of table `table` on one trace under challenges [beta_0, gamma_0, beta_1, gamma_1], from plain loops on the
    host (starkhip_ctl_polys_replay): (polys [4 E, n] -- per (challenge, endpoint) h then Z --, sums [2 E], zero denominators)."""
    trace = np.ascontiguousarray(trace, dtype=np.uint64)
    if trace.ndim != 2 or layout not in (0, 1):
        raise StarkhipError(ERR_BAD_SHAPE)
    n_rows, n_cols = trace.shape if layout == 0 else trace.shape[::-1]
    challenges, polys, sums, zeros = _ctl_args(system, table, n_rows, challenges)
    _chk(lib.starkhip_ctl_polys_replay(system, table, _p64(trace), n_rows, n_cols, layout, _p64(challenges), _p64(polys), _p64(sums), _p64(zeros)))
    return polys, sums, int(zeros[0])


def ctl_polys(prover, system, table, trace, challenges, layout=0):
    """ctl_polys_replay's result from the Prover's device, through the kernels the system prover uses (starkhip_ctl_polys)."""
    trace = np.ascontiguousarray(trace, dtype=np.uint64)
    if trace.ndim != 2 or layout not in (0, 1):
        raise StarkhipError(ERR_BAD_SHAPE)
    n_rows, n_cols = trace.shape if layout == 0 else trace.shape[::-1]
    challenges, polys, sums, zeros = _ctl_args(system, table, n_rows, challenges)
    _chk(lib.starkhip_ctl_polys(prover._ctx, system, table, trace.ctypes.data_as(C.c_void_p), n_rows, n_cols, layout, 0, _p64(challenges), _p64(polys),
                                _p64(sums), _p64(zeros)))
    return polys, sums, int(zeros[0])


def system_eval_frame_ctl(system, table, local, nxt, pis, masks, alphas, aux, aux_next, logup_challenges, ctl_challenges, sums):
    """starkhip_system_eval_frame_ctl: the alpha fold of the table's AIR constraints, its LogUp constraints and its 8 E CTL constraints
    on one extension frame.  local / nxt [C, 2], masks [4, 2], alphas [n, 2], aux / aux_next [nA + nC, 2]; returns [n, 2]."""
    arr = lambda a: np.ascontiguousarray(a, dtype=np.uint64)  # noqa: E731
    local, nxt, pis, masks, alphas, aux, aux_next = (arr(a) for a in (local, nxt, pis, masks, alphas, aux, aux_next))
    lch, cch, sums = arr(logup_challenges), arr(ctl_challenges), arr(sums)
    air = _nonneg(lib.starkhip_system_table_air(system, table))
    want = air_logup_polys(air) + 4 * system_table_endpoints(system, table)
    if local.shape != (air_columns(air), 2) or nxt.shape != local.shape or masks.shape != (4, 2) or alphas.ndim != 2 or alphas.shape[1] != 2 or \
            aux.shape != (want, 2) or aux_next.shape != aux.shape or lch.size != 2 or cch.size != 4 or sums.size * 2 != 4 * system_table_endpoints(system, table):
        raise StarkhipError(ERR_BAD_SHAPE)
    acc = np.zeros_like(alphas)
    _chk(lib.starkhip_system_eval_frame_ctl(system, table, _p64(local), _p64(nxt), _p64(pis), _p64(masks), _p64(alphas), alphas.shape[0], _p64(aux),
                                            _p64(aux_next), _p64(lch), _p64(cch), _p64(sums), _p64(acc)))
    return acc


class SystemProver:
    """A system prover (starkhip_system_create): one context per table on one device.  prove() commits every table's trace once, draws
    the CTL challenges from all the trace caps, checks every CTL's balance before anything auxiliary is committed and returns one blob."""

    def __init__(self, system, device=0):
        self.system = system
        self._h = C.c_void_p()
        _chk(lib.starkhip_system_create(device, system, C.byref(self._h)))

    def close(self):
        if self._h:
            lib.starkhip_system_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name, value):
        """a context option ("hasher", ...) on every table's context"""
        _chk(lib.starkhip_system_set_option(self._h, name.encode(), int(value)))

    def last_timings(self, table):
        """{phase: ms} of table `table`'s last proof (starkhip_system_last_timings)"""
        ms = (C.c_float * N_PHASES)()
        _chk(lib.starkhip_system_last_timings(self._h, table, ms))
        return dict(zip(PHASE_NAMES, [float(x) for x in ms]))

    def prove(self, configs, traces, public_inputs, pow_witness=POW_SEARCH, layouts=None, device_ptrs=None):
        """configs, traces, public_inputs: one per table.  traces[t]: numpy uint64, row-major [n, C] (layouts[t] = 0, the default) or
        column-major [C, n] (1); with device_ptrs[t] = (address, n_rows) the table's trace is read from this device's memory instead.
        Raises SystemRefused (naming the CTL) when a CTL does not balance."""
        T = len(configs)
        layouts = list(layouts) if layouts is not None else [0] * T
        keep, ptrs, rows, on_dev = [], [], [], []
        for t in range(T):
            if device_ptrs is not None and device_ptrs[t] is not None:
                ptrs.append(C.c_void_p(device_ptrs[t][0]))
                rows.append(int(device_ptrs[t][1]))
                on_dev.append(1)
                continue
            tr = np.ascontiguousarray(traces[t], dtype=np.uint64)
            if tr.ndim != 2 or layouts[t] not in (0, 1):
                raise StarkhipError(ERR_BAD_SHAPE)
            keep.append(tr)
            ptrs.append(tr.ctypes.data_as(C.c_void_p))
            rows.append(tr.shape[0] if layouts[t] == 0 else tr.shape[1])
            on_dev.append(0)
        pis = [np.ascontiguousarray(p, dtype=np.uint64) for p in public_inputs]
        out, words, bad = _u64p(), C.c_size_t(), C.c_int(-1)
        rc = lib.starkhip_system_prove(self._h, (StarkConfig * T)(*configs), (C.c_void_p * T)(*ptrs), (C.c_size_t * T)(*rows), (C.c_int * T)(*layouts),
                                       (C.c_int * T)(*on_dev), (_u64p * T)(*[_p64(p) for p in pis]), (C.c_size_t * T)(*[p.size for p in pis]), pow_witness,
                                       C.byref(out), C.byref(words), C.byref(bad))
        if rc == ERR_QUOTIENT_NOT_DIVISIBLE and bad.value >= 0:
            raise SystemRefused(bad.value)
        return _take_blob(rc, out, words)

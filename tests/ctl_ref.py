"""Test-side reference for cross-table lookups (COMPAT.md §2d, C1 - C8), on Python integers and independent of the C++: the endpoints of a
table in system order, the CTL polynomials and sums of a trace, the four constraints on an extension frame, the system transcript, and a
mini-verifier of a system proof blob under either hasher.  Built on logup_columns_ref (Columns, Filters, the LogUp constraints of a table
that has lookups of its own) and keccak_ref (challenger, hashers, field helpers, Merkle paths), imported and unchanged.

A Column is (constant, [(column, coefficient)] on the local row, the same on the next row) and a Filter ([(A, B)], [C]), as in
logup_columns_ref; an endpoint is (table, [Column], Filter); a CTL is (looked endpoint, [looking endpoints]).  The named cases are at the
end, each with a trace generator."""
import copy

import numpy as np

import logup_columns_ref as G
import logup_ref as R
from keccak_ref import (HASHERS, P, PROOF_MAGIC, Challenger, Reject, _merkle, _need, bitrev, eadd, einv, emul, epow, escale, esub, finv,
                        reduction_arity_bits, root_of_unity)

SYSTEM_PROOF_MAGIC = int.from_bytes(b"SYSPF01", "little")
CHALLENGES = (0x0123456789ABCDEF % P, 0x0FEDCBA987654321 % P, 0x1122334455667788 % P, 0x8877665544332211 % P)  # beta_0, gamma_0, beta_1, gamma_1
KIND_PLAIN, KIND_TRANSITION, KIND_FIRST, KIND_LAST = 0, 1, 2, 3


def table_endpoints(ctls, t):
    """the endpoints of table t in system order: CTL after CTL, the looked endpoint first, then the looking ones as declared"""
    return [ep for looked, looking in ctls for ep in [looked] + list(looking) if ep[0] == t]


# ------------------------------------------------------------------------------------------------ base field: a trace
def combined(ep, row, nxt, beta, gamma):
    c, bp = gamma, 1
    for col in ep[1]:
        c = (c + bp * G.column_value(col, row, nxt)) % P
        bp = bp * beta % P
    return c


def polys_and_sums(eps, rows, challenges):
    """C3.  rows: the trace as rows of ints (any representative of a cell); the next row of the last is row 0.
    -> (polys [4 E][n]: per (challenge, endpoint) h then Z, sums [2 E] challenge-major, zero denominators)"""
    n, zeros, polys, sums = len(rows), 0, [], []
    for i in range(2):
        beta, gamma = int(challenges[2 * i]), int(challenges[2 * i + 1])
        for ep in eps:
            h, z, run = [], [], 0
            for r in range(n):
                row, nxt = rows[r], rows[(r + 1) % n]
                c = combined(ep, row, nxt, beta, gamma)
                zeros += c == 0
                h.append(G.filter_value(ep[2], row, nxt) * finv(c) % P)  # the inverse of 0 is 0
                z.append(run)
                run = (run + h[-1]) % P
            polys += [h, z]
            sums.append(run)
    return polys, sums, zeros


def first_unbalanced(ctls, sums_of):
    """-1, or the first CTL whose looking sums do not add up to its looked sum under some challenge; sums_of[t]: table t's 2 E_t sums"""
    at = {}
    for k, (looked, looking) in enumerate(ctls):
        diff = [0, 0]
        for side, ep in [(-1, looked)] + [(1, e) for e in looking]:
            t = ep[0]
            E = len(sums_of[t]) // 2
            for i in range(2):
                diff[i] = (diff[i] + side * sums_of[t][i * E + at.get(t, 0)]) % P
            at[t] = at.get(t, 0) + 1
        if diff != [0, 0]:
            return k
    return -1


# ------------------------------------------------------------------------------------------------ extension field: a frame
def ctl_constraints_ext(eps, local, nxt, aux, aux_next, challenges, sums):
    """C4 on an extension frame (canonical words), without masks, in the order of the fold: a list of (kind, value)."""
    out, E = [], len(eps)
    for i in range(2):
        beta, gamma = int(challenges[2 * i]), int(challenges[2 * i + 1])
        for e, ep in enumerate(eps):
            c, bp = (gamma, 0), 1
            for col in ep[1]:
                c = eadd(c, escale(G._ecolumn(col, local, nxt), bp))
                bp = bp * beta % P
            h, z, zn = aux[2 * (i * E + e)], aux[2 * (i * E + e) + 1], aux_next[2 * (i * E + e) + 1]
            out.append((KIND_PLAIN, esub(emul(h, c), G._efilter(ep[2], local, nxt))))
            out.append((KIND_FIRST, z))
            out.append((KIND_TRANSITION, esub(esub(zn, z), h)))
            out.append((KIND_LAST, esub(eadd(z, h), (int(sums[i * E + e]), 0))))
    return out


def fold_all(own_values, logup_values, ctl_values, masks, alpha):
    """acc = acc alpha + mask c over the AIR's own (already masked) values, the LogUp constraints, the CTL constraints"""
    acc = R.fold_full(own_values, logup_values, masks, alpha)
    for kind, v in ctl_values:
        acc = eadd(emul(acc, alpha), v if kind == KIND_PLAIN else emul(masks[kind], v))  # (a plain constraint has no mask, as in fold_full)
    return acc


# ------------------------------------------------------------------------------------------------ the transcript and the mini-verifier
def split_system_proof(blob):
    w = [int(x) for x in blob]
    _need(len(w) >= 3 and w[0] == SYSTEM_PROOF_MAGIC, "system header")
    T = w[1]
    _need(2 <= T <= 64 and len(w) >= 3 + T, "system header: tables")
    off = w[2:3 + T]
    _need(off[0] == 3 + T and off[T] == len(w) and all(off[t] + 16 <= off[t + 1] for t in range(T)), "system header: offsets")
    return [w[off[t]:off[t + 1]] for t in range(T)]


def system_transcript(hasher, trace_caps):
    """C1: (the challenger after it, [beta_0, gamma_0, beta_1, gamma_1])"""
    ch = Challenger(HASHERS[hasher])
    for cap in trace_caps:
        ch.observe_many(cap)
    return ch, [ch.get() for _ in range(4)]


def trace_cap(proof_words):
    ncap = 1 << proof_words[5]
    return proof_words[16:16 + 4 * ncap]


def verify_table_or_raise(program_blob, eps, cfg, proof, hasher, ch_initial, challenges):
    """One table proof of a system: C2 (the transcript starts from a copy of the system's and observes the sums behind the auxiliary
    cap), C3 / C5 (the middle matrix LogUp || CTL in every opening and query), C4 at zeta with the sums taken from the proof.
    Returns the table's sums.  Raises Reject with the first failure, naming it."""
    h = HASHERS[hasher]
    blob, lookups = G.split_program(program_blob)
    w = [int(x) for x in proof]
    _need(len(w) >= 16 and w[0] == PROOF_MAGIC, "header")
    C_, Q, log_n, rate, cap_h, L, nq, final_len, n_pis, arity, n_ch, hid, nZ, nA, nC = w[1:16]
    _need(hid == hasher, "header names another hasher")
    degree = int(blob[3])
    factor = max(degree - 1, 1)
    _need(nZ == 0 and nA == G.n_polys(lookups, degree) and nC == 4 * len(eps), "header words 13 - 15 (nZ, nA, nC)")
    _need(C_ == int(blob[1]) and n_pis == int(blob[2]) and n_ch == 2 == cfg.num_challenges and Q == 2 * factor, "shape")
    _need(rate == cfg.rate_bits and cap_h == cfg.cap_height and nq == cfg.num_query_rounds and arity == cfg.arity_bits, "config")
    arities = reduction_arity_bits(log_n, rate, cap_h, arity, cfg.final_poly_bits)
    _need(len(arities) == L and final_len == 1 << (log_n - sum(arities)), "FRI geometry")
    ncap, log_N, n = 1 << cap_h, log_n + rate, 1 << log_n
    N, nM = 1 << log_N, nA + nC
    n_mats = 3 if nM else 2
    o = 16
    off_tcap = o; o += 4 * ncap
    off_acap = o; o += 4 * ncap * (n_mats - 2)
    off_qcap = o; o += 4 * ncap
    off_local = o; o += 2 * C_
    off_next = o; o += 2 * C_
    off_aux = o; o += 2 * nM
    off_auxn = o; o += 2 * nM
    off_qopen = o; o += 2 * Q
    off_fcaps = o; o += L * 4 * ncap
    off_queries = o
    d0 = log_N - cap_h
    depths, lg = [], log_N
    for ab in arities:
        lg -= ab
        depths.append(lg - cap_h)
    qwords = C_ + nM + Q + 4 * n_mats * d0 + sum(2 * (1 << ab) + 4 * d for ab, d in zip(arities, depths))
    o += nq * qwords
    off_final = o; o += 2 * final_len
    off_pow = o; o += 1
    off_pis = o; o += n_pis
    off_sums = o; o += nC // 2
    _need(o == len(w), "length")
    _need(all(x < P for x in w[16:]), "a word is no field element")
    ext = lambda off, i: (w[off + 2 * i], w[off + 2 * i + 1])  # noqa: E731
    tcap, qcap = w[off_tcap:off_tcap + 4 * ncap], w[off_qcap:off_qcap + 4 * ncap]
    acap = w[off_acap:off_acap + 4 * ncap] if nM else []
    fcaps = [w[off_fcaps + 4 * ncap * l:off_fcaps + 4 * ncap * (l + 1)] for l in range(L)]
    for cap in [tcap, qcap] + ([acap] if nM else []) + fcaps:
        _need(all(h.digest_ok(cap[4 * i:4 * i + 4]) for i in range(ncap)), "cap entry is no digest")
    op_local = [ext(off_local, i) for i in range(C_)]
    op_next = [ext(off_next, i) for i in range(C_)]
    op_a = [ext(off_aux, i) for i in range(nM)]
    op_an = [ext(off_auxn, i) for i in range(nM)]
    op_q = [ext(off_qopen, i) for i in range(Q)]
    final_poly = [ext(off_final, i) for i in range(final_len)]
    pis = np.array(w[off_pis:off_pis + n_pis], dtype=np.uint64)
    sums = w[off_sums:off_sums + nC // 2]

    # 1. the transcript: a copy of the system's, which has observed every trace cap (this table's among them)
    ch = copy.deepcopy(ch_initial)
    chis = [ch.get(), ch.get()] if nA else [0, 0]
    if nM:
        ch.observe_many(acap)
    ch.observe_many(sums)
    alphas = [ch.get(), ch.get()]
    ch.observe_many(qcap)
    zeta = ch.get_ext()
    for group in (op_local, op_a, op_q, op_next, op_an):
        for e in group:
            ch.observe_many(e)
    fri_alpha = ch.get_ext()
    betas = []
    for l in range(L):
        ch.observe_many(fcaps[l])
        betas.append(ch.get_ext())
    for e in final_poly:
        ch.observe_many(e)
    ch.observe(w[off_pow])
    pow_response = ch.get()
    indices = [ch.get() % N for _ in range(nq)]
    bits = cfg.proof_of_work_bits
    _need(bits == 0 or pow_response >> (64 - bits) == 0, "proof of work")
    # 2. every Merkle path of every query
    rounds = []
    for qi in range(nq):
        p = off_queries + qi * qwords
        tleaf = w[p:p + C_]; p += C_
        tsib = w[p:p + 4 * d0]; p += 4 * d0
        aleaf, asib = [], []
        if nM:
            aleaf = w[p:p + nM]; p += nM
            asib = w[p:p + 4 * d0]; p += 4 * d0
        qleaf = w[p:p + Q]; p += Q
        qsib = w[p:p + 4 * d0]; p += 4 * d0
        x_index = indices[qi]
        _need(_merkle(h, tleaf, x_index, tcap, tsib), "trace path")
        _need(not nM or _merkle(h, aleaf, x_index, acap, asib), "auxiliary path")
        _need(_merkle(h, qleaf, x_index, qcap, qsib), "quotient path")
        steps = []
        for l, ab in enumerate(arities):
            ev = w[p:p + 2 * (1 << ab)]; p += 2 * (1 << ab)
            sib = w[p:p + 4 * depths[l]]; p += 4 * depths[l]
            x_index >>= ab
            _need(_merkle(h, ev, x_index, fcaps[l], sib), "FRI path")
            steps.append(ev)
        rounds.append((tleaf, aleaf, qleaf, steps))
    # 3. the quotient identity at zeta, over the AIR's, the LogUp and the CTL constraints
    g = root_of_unity(log_n)
    zeta_n = epow(zeta, n)
    z_h = esub(zeta_n, (1, 0))
    masks = [(1, 0), esub(zeta, (finv(g), 0)), emul(z_h, einv(escale(esub(zeta, (1, 0)), n))),
             emul(z_h, einv(escale(esub(escale(zeta, g), (1, 0)), n)))]
    own = R.own_values_ext(blob, op_local, op_next, pis, masks)
    lc = G.logup_constraints_ext(lookups, degree, op_local, op_next, op_a[:nA], op_an[:nA], chis) if nA else []
    cc = ctl_constraints_ext(eps, op_local, op_next, op_a[nA:], op_an[nA:], challenges, sums)
    _need(len(lc) == G.n_constraints(lookups, degree) and len(cc) == 8 * len(eps), "constraint count")
    for j in range(2):
        acc = fold_all(own, lc, cc, masks, (alphas[j], 0))
        s = (0, 0)
        for k in reversed(range(factor)):
            s = eadd(emul(s, zeta_n), op_q[j * factor + k])
        _need(acc == emul(z_h, s), "quotient identity")
    # 4. FRI
    gzeta = escale(zeta, g)

    def reduce(vals):
        acc = (0, 0)
        for v in reversed(vals):
            acc = eadd(emul(acc, fri_alpha), v)
        return acc
    red0, red1 = reduce(op_local + op_a + op_q), reduce(op_next + op_an)
    alpha_c = epow(fri_alpha, C_ + nM)
    wN = root_of_unity(log_N)
    for qi in range(nq):
        tleaf, aleaf, qleaf, steps = rounds[qi]
        x_index = indices[qi]
        x = 7 * pow(wN, bitrev(x_index, log_N), P) % P
        e0 = reduce([(v, 0) for v in tleaf + aleaf + qleaf])
        e1 = reduce([(v, 0) for v in tleaf + aleaf])
        old = eadd(emul(emul(esub(e0, red0), einv(esub((x, 0), zeta))), alpha_c), emul(esub(e1, red1), einv(esub((x, 0), gzeta))))
        for l, ab in enumerate(arities):
            ar = 1 << ab
            ev = steps[l]
            within = x_index & (ar - 1)
            _need((ev[2 * within], ev[2 * within + 1]) == old, "FRI coset value")
            ga = root_of_unity(ab)
            start = x * pow(ga, ar - bitrev(within, ab), P) % P
            beta = betas[l]
            acc = (0, 0)
            p_i = start
            for i in range(ar):
                k = bitrev(i, ab)
                e_i = (ev[2 * k], ev[2 * k + 1])
                den = escale(esub(beta, (p_i, 0)), pow(p_i, ar - 1, P))
                acc = eadd(acc, emul(e_i, einv(den)))
                p_i = p_i * ga % P
            old = escale(emul(esub(epow(beta, ar), (pow(start, ar, P), 0)), acc), finv(ar))
            x = pow(x, ar, P)
            x_index >>= ab
        fin = (0, 0)
        for c in reversed(final_poly):
            fin = eadd(escale(fin, x), c)
        _need(fin == old, "final polynomial")
    return sums


def verify_system_or_raise(program_blobs, ctls, cfgs, proof, hasher):
    """C7: the system transcript replayed from the table proofs' trace caps, every table proof from the copied state, every CTL's sums."""
    tables = split_system_proof(proof)
    _need(len(tables) == len(program_blobs), "tables")
    for w in tables:
        _need(w[0] == PROOF_MAGIC and w[5] <= 16 and len(w) >= 16 + 4 * (1 << w[5]), "table header")
    ch, challenges = system_transcript(hasher, [trace_cap(w) for w in tables])
    sums_of = [verify_table_or_raise(program_blobs[t], table_endpoints(ctls, t), cfgs[t], tables[t], hasher, ch, challenges) for t in range(len(tables))]
    _need(first_unbalanced(ctls, sums_of) < 0, "a CTL's sums do not balance")


def verify_system(program_blobs, ctls, cfgs, proof, hasher):
    try:
        verify_system_or_raise(program_blobs, ctls, cfgs, proof, hasher)
        return True
    except Reject:
        return False


# ------------------------------------------------------------------------------------------------ the named cases and their traces
def plain(col):
    return (0, [(int(col), 1)], [])


def sel(col):
    """the filter that is the value of one column"""
    return ([], [plain(col)])


class Table:
    """One table: G.own_constraints on columns 0 .. 2 at `degree`, then the columns its endpoints read; declare(b): its own LogUp lookups"""

    def __init__(self, n_cols, degree, declare=None):
        self.n_cols, self.degree, self.declare = n_cols, degree, declare

    def blob(self):
        from starky_bls12_381_amd.air_builder import AirBuilder
        b = AirBuilder(self.n_cols, 1, self.degree)
        G.own_constraints(b, self.degree)
        if self.declare:
            self.declare(b)
        return b.finish()


class Case:
    """tables, ctls (of this module's endpoints) and fill(traces, rng): the cells behind column 2 of every table's trace, such that every
    CTL balances"""

    def __init__(self, name, tables, ctls, fill):
        self.name, self.tables, self.ctls, self.fill = name, tables, ctls, fill


def own_rows(table, n, rng):
    t = [[0] * table.n_cols for _ in range(n)]
    start = int(rng.integers(1, 1 << 30))
    for r in range(n):
        x = (start + r) % P
        x2 = x * x % P
        t[r][0], t[r][1], t[r][2] = x, x2, (x2 * x % P if table.degree in (2, 3) else x2 * x2 % P * x % P)
    return t, start


def make_traces(case, rows, seed):
    """[(trace row-major uint64, public inputs)] per table, rows[t] rows each"""
    rng = np.random.default_rng(seed)
    traces, starts = [], []
    for table, n in zip(case.tables, rows):
        t, start = own_rows(table, n, rng)
        traces.append(t)
        starts.append(start)
    case.fill(traces, rng)
    return [(np.array(t, dtype=np.uint64), np.array([s], dtype=np.uint64)) for t, s in zip(traces, starts)]


def _lookup_fill(looker, looked, rng, n_values, write, count_col, selected):
    """every row r of `looker` takes the tuple of a random row k of `looked` (write(looker, r, k)); where selected(r) the multiplicity of
    the first looked row holding that tuple's value class k % n_values goes up by one"""
    for r in range(len(looker)):
        k = int(rng.integers(0, min(n_values, len(looked))))
        write(looker, r, k)
        if selected(r):
            looked[k][count_col] += 1


def _cases():
    out = {}

    # range: one column under a selector filter looked up in a table whose filter is its multiplicity column
    def range_fill(tr, rng):
        a, b = tr
        for r in range(len(b)):
            b[r][3] = r
        for r in range(len(a)):
            a[r][4] = int(rng.integers(0, 2))
        _lookup_fill(a, b, rng, len(b), lambda t, r, k: t[r].__setitem__(3, k), 4, lambda r: a[r][4] == 1)
    out["range"] = Case("range", [Table(5, 2), Table(5, 2)], [((1, [plain(3)], sel(4)), [(0, [plain(3)], sel(4))])], range_fill)

    # xor: width 3, (a, b, a ^ b) into a 2-bit table: the beta powers
    def xor_fill(tr, rng):
        a, b = tr
        for r in range(len(b)):
            x, y = (r >> 2) & 3, r & 3
            b[r][3], b[r][4], b[r][5] = x, y, x ^ y

        def write(t, r, k):
            t[r][3], t[r][4], t[r][5] = b[k][3], b[k][4], b[k][5]
        for r in range(len(a)):
            a[r][6] = int(rng.integers(0, 2))
        _lookup_fill(a, b, rng, 16, write, 6, lambda r: a[r][6] == 1)
    out["xor"] = Case("xor", [Table(7, 2), Table(7, 3)], [((1, [plain(3), plain(4), plain(5)], sel(6)), [(0, [plain(3), plain(4), plain(5)], sel(6))])], xor_fill)

    # two_lookers: two tables look into a third
    def two_fill(tr, rng):
        a, b, c = tr
        for r in range(len(c)):
            c[r][3] = 3 * r + 1
        for t in (a, b):
            for r in range(len(t)):
                t[r][4] = int(rng.integers(0, 2))
            _lookup_fill(t, c, rng, len(c), lambda u, r, k: u[r].__setitem__(3, c[k][3]), 4, lambda r, t=t: t[r][4] == 1)
    out["two_lookers"] = Case("two_lookers", [Table(5, 2), Table(5, 3), Table(5, 2)],
                              [((2, [plain(3)], sel(4)), [(0, [plain(3)], sel(4)), (1, [plain(3)], sel(4))])], two_fill)

    # chain: table 1 is looked in CTL 0 and looking in CTL 1, and has a LogUp lookup of its own: its auxiliary matrix is LogUp || CTL
    def chain_declare(b):
        b.logup([6], 3, 7)

    def chain_fill(tr, rng):
        a, b, c = tr
        for r in range(len(c)):
            c[r][3] = 7 * r + 2
        for r in range(len(b)):
            b[r][3] = r + 100  # what table 0 looks up, and the table of b's own LogUp lookup
            k = int(rng.integers(0, len(b)))
            b[r][6] = k + 100
        for r in range(len(b)):
            b[r][7] = sum(1 for q in range(len(b)) if b[q][6] == b[r][3])
        _lookup_fill(b, c, rng, len(c), lambda u, r, k: u[r].__setitem__(5, c[k][3]), 4, lambda r: True)  # every row of b looks into c
        for r in range(len(a)):
            a[r][4] = int(rng.integers(0, 2))
        _lookup_fill(a, b, rng, len(b), lambda u, r, k: u[r].__setitem__(3, b[k][3]), 4, lambda r: a[r][4] == 1)
    out["chain"] = Case("chain", [Table(5, 2), Table(8, 3, chain_declare), Table(5, 2)],
                        [((1, [plain(3)], sel(4)), [(0, [plain(3)], sel(4))]), ((2, [plain(3)], sel(4)), [(1, [plain(5)], ([], []))])], chain_fill)

    # next_row: a Column with a next-row term of coefficient p - 1, under a product filter
    def next_fill(tr, rng):
        a, b = tr
        n = len(a)
        for r in range(len(b)):
            b[r][3] = 5 * r + 3
        for r in range(n):
            a[r][4] = int(rng.integers(0, 1 << 16))
            a[r][5], a[r][6] = int(rng.integers(0, 2)), int(rng.integers(0, 2))

        def write(t, r, k):  # local[3] - next[4] = the table value
            t[r][3] = (b[k][3] + t[(r + 1) % n][4]) % P
        _lookup_fill(a, b, rng, len(b), write, 4, lambda r: a[r][5] * a[r][6] == 1)
    out["next_row"] = Case("next_row", [Table(7, 3), Table(5, 2)],
                           [((1, [plain(3)], sel(4)), [(0, [(0, [(3, 1)], [(4, P - 1)])], ([(plain(5), plain(6))], []))])], next_fill)
    return out


CASES = _cases()

"""Test-side reference for LogUp lookups (COMPAT.md L1 - L7), on Python integers and independent of the C++: the section of a program
blob, the auxiliary polynomials and closing values of a trace, the LogUp constraints on an extension frame, the full fold, and a
mini-verifier of proofs with nA > 0 under either hasher.  Built from keccak_ref's Challenger, hashers, field helpers and
constraints_ext (imported, not edited)."""
import numpy as np

from keccak_ref import (HASHERS, P, PROOF_MAGIC, Challenger, Reject, _merkle, _need, bitrev, constraints_ext, eadd, einv, emul, epow,
                        escale, esub, finv, reduction_arity_bits, root_of_unity)

AIR_LOGUP_MAGIC = 0x3130535055474F4C  # "LOGUPS01"
assert AIR_LOGUP_MAGIC.to_bytes(8, "little") == b"LOGUPS01"


def split_program(blob):
    """(the program without its LogUp section, the lookups as (columns, table, frequencies)) of a constraint-program blob."""
    w = [int(x) for x in blob]
    base = 8 + w[5] + (w[6] + 1) // 2 + w[7]
    if len(w) == base:
        return np.array(w, dtype=np.uint64), []
    assert w[base] == AIR_LOGUP_MAGIC
    lookups, at = [], base + 2
    for _ in range(w[base + 1]):
        m, tf = w[at], w[at + 1]
        lookups.append((w[at + 2:at + 2 + m], tf & 0xFFFFFFFF, tf >> 32))
        assert len(lookups[-1][0]) == m
        at += 2 + m
    assert at == len(w)
    return np.array(w[:base], dtype=np.uint64), lookups


def helper_batches(columns, degree):
    """a lookup's columns cut in declaration order into batches of degree - 1"""
    B = degree - 1
    return [columns[i:i + B] for i in range(0, len(columns), B)]


def n_polys(lookups, degree):
    return 2 * sum(len(helper_batches(cols, degree)) + 1 for cols, _, _ in lookups)


def n_constraints(lookups, degree):
    return 2 * sum(len(helper_batches(cols, degree)) + 2 for cols, _, _ in lookups)


def polys_and_closing(lookups, degree, rows, challenges):
    """L2.  rows: the trace as a list of rows of ints (any representative of a cell).
    -> (polys [nA][n] challenge-major, closing [2][n_lookups], zero denominators)"""
    zeros = 0
    polys, closing = [], []

    def inv0(x):
        nonlocal zeros
        zeros += x == 0
        return finv(x)  # the inverse of 0 is 0: pow(0, p - 2, p)
    for i in range(2):
        chi = int(challenges[i])
        closing.append([])
        for cols, t, f in lookups:
            batches = helper_batches(cols, degree)
            hs = [[] for _ in batches]
            z, run = [], 0
            for row in rows:
                z.append(run)
                for j, batch in enumerate(batches):
                    h = sum(inv0((chi + int(row[c])) % P) for c in batch) % P
                    hs[j].append(h)
                    run = (run + h) % P
                run = (run - int(row[f]) % P * inv0((chi + int(row[t])) % P)) % P
            polys += hs + [z]
            closing[i].append(run)
    return polys, closing, zeros


def logup_constraints_ext(lookups, degree, local, aux, aux_next, challenges):
    """L4 on an extension frame, without masks, in the order of the fold: a list of (is_first_row, value)."""
    out, at = [], 0
    for i in range(2):
        chi = (int(challenges[i]), 0)
        for cols, t, f in lookups:
            batches = helper_batches(cols, degree)
            hsum = (0, 0)
            for j, batch in enumerate(batches):
                xs = [eadd(chi, local[c]) for c in batch]
                prod = (1, 0)
                for x in xs:
                    prod = emul(prod, x)
                rest = (0, 0)
                for k in range(len(xs)):
                    term = (1, 0)
                    for k2, x in enumerate(xs):
                        if k2 != k:
                            term = emul(term, x)
                    rest = eadd(rest, term)
                out.append((False, esub(emul(aux[at + j], prod), rest)))
                hsum = eadd(hsum, aux[at + j])
            H = len(batches)
            z, zn = aux[at + H], aux_next[at + H]
            den = eadd(chi, local[t])
            out.append((True, z))
            out.append((False, eadd(esub(emul(esub(zn, z), den), emul(hsum, den)), local[f])))
            at += H + 1
    return out


def fold_full(own_values, logup_values, masks, alpha):
    """acc = acc alpha + mask c over the AIR's own (already masked) values, then the LogUp constraints."""
    acc = (0, 0)
    for v in own_values:
        acc = eadd(emul(acc, alpha), v)
    for first, v in logup_values:
        acc = eadd(emul(acc, alpha), emul(masks[2], v) if first else v)
    return acc


def own_values_ext(blob, local, nxt, pis, masks):
    """the AIR's own K constraints on an extension frame, each with its kind's mask"""
    per_kind = constraints_ext(blob, local, nxt, pis)
    own = []
    for k in range(int(blob[4])):
        val = (0, 0)
        for kind in range(4):
            val = eadd(val, emul(masks[kind], per_kind[kind][k]))
        own.append(val)
    return own


def verify_or_raise(program_blob, cfg, proof, hasher):
    """keccak_ref.verify_or_raise for a proof of a program with LogUp lookups: L1 (chi_0, chi_1 after the trace cap), L3 (the auxiliary
    cap, then the alphas), L5 (openings local, aux, quotient, next, aux_next), L4 at zeta, L6 / L7 (the auxiliary leaf's path and its
    share of fri_combine_initial in every query).  Raises Reject with the first failure, naming it."""
    h = HASHERS[hasher]
    blob, lookups = split_program(program_blob)
    w = [int(x) for x in proof]
    _need(len(w) >= 16 and w[0] == PROOF_MAGIC, "header")
    C_, Q, log_n, rate, cap_h, L, nq, final_len, n_pis, arity, n_ch, hid, nZ, nA = w[1:15]
    _need(hid == hasher, "header names another hasher")
    degree = int(blob[3])
    factor = max(degree - 1, 1)
    _need(nZ == 0 and nA == n_polys(lookups, degree) and nA > 0, "header words 13, 14 (nZ, nA)")
    _need(C_ == int(blob[1]) and n_pis == int(blob[2]) and n_ch == 2 == cfg.num_challenges and Q == 2 * factor, "shape")
    _need(rate == cfg.rate_bits and cap_h == cfg.cap_height and nq == cfg.num_query_rounds and arity == cfg.arity_bits, "config")
    arities = reduction_arity_bits(log_n, rate, cap_h, arity, cfg.final_poly_bits)
    _need(len(arities) == L and final_len == 1 << (log_n - sum(arities)), "FRI geometry")
    ncap, log_N, n = 1 << cap_h, log_n + rate, 1 << log_n
    N = 1 << log_N
    o = 16
    off_tcap = o; o += 4 * ncap
    off_acap = o; o += 4 * ncap
    off_qcap = o; o += 4 * ncap
    off_local = o; o += 2 * C_
    off_next = o; o += 2 * C_
    off_aux = o; o += 2 * nA
    off_auxn = o; o += 2 * nA
    off_qopen = o; o += 2 * Q
    off_fcaps = o; o += L * 4 * ncap
    off_queries = o
    d0 = log_N - cap_h
    depths, lg = [], log_N
    for ab in arities:
        lg -= ab
        depths.append(lg - cap_h)
    qwords = C_ + nA + Q + 12 * d0 + sum(2 * (1 << ab) + 4 * d for ab, d in zip(arities, depths))
    o += nq * qwords
    off_final = o; o += 2 * final_len
    off_pow = o; o += 1
    off_pis = o; o += n_pis
    _need(o == len(w), "length")
    _need(all(x < P for x in w[16:]), "a word is no field element")
    ext = lambda off, i: (w[off + 2 * i], w[off + 2 * i + 1])  # noqa: E731
    tcap, acap, qcap = (w[off:off + 4 * ncap] for off in (off_tcap, off_acap, off_qcap))
    fcaps = [w[off_fcaps + 4 * ncap * l:off_fcaps + 4 * ncap * (l + 1)] for l in range(L)]
    for cap in [tcap, acap, qcap] + fcaps:
        _need(all(h.digest_ok(cap[4 * i:4 * i + 4]) for i in range(ncap)), "cap entry is no digest")
    op_local = [ext(off_local, i) for i in range(C_)]
    op_next = [ext(off_next, i) for i in range(C_)]
    op_a = [ext(off_aux, i) for i in range(nA)]
    op_an = [ext(off_auxn, i) for i in range(nA)]
    op_q = [ext(off_qopen, i) for i in range(Q)]
    final_poly = [ext(off_final, i) for i in range(final_len)]
    pis = np.array(w[off_pis:off_pis + n_pis], dtype=np.uint64)

    # 1. the transcript
    ch = Challenger(h)
    ch.observe_many(tcap)
    challenges = [ch.get(), ch.get()]  # L1
    ch.observe_many(acap)
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
    # 2. proof of work
    bits = cfg.proof_of_work_bits
    _need(bits == 0 or pow_response >> (64 - bits) == 0, "proof of work")
    # 3. every Merkle path of every query
    rounds = []
    for qi in range(nq):
        p = off_queries + qi * qwords
        tleaf = w[p:p + C_]; p += C_
        tsib = w[p:p + 4 * d0]; p += 4 * d0
        aleaf = w[p:p + nA]; p += nA
        asib = w[p:p + 4 * d0]; p += 4 * d0
        qleaf = w[p:p + Q]; p += Q
        qsib = w[p:p + 4 * d0]; p += 4 * d0
        x_index = indices[qi]
        _need(_merkle(h, tleaf, x_index, tcap, tsib), "trace path")
        _need(_merkle(h, aleaf, x_index, acap, asib), "auxiliary path")
        _need(_merkle(h, qleaf, x_index, qcap, qsib), "quotient path")
        steps = []
        for l, ab in enumerate(arities):
            ev = w[p:p + 2 * (1 << ab)]; p += 2 * (1 << ab)
            sib = w[p:p + 4 * depths[l]]; p += 4 * depths[l]
            x_index >>= ab
            _need(_merkle(h, ev, x_index, fcaps[l], sib), "FRI path")
            steps.append(ev)
        rounds.append((tleaf, aleaf, qleaf, steps))
    # 4. the quotient identity at zeta, over all K + nL constraints
    g = root_of_unity(log_n)
    zeta_n = epow(zeta, n)
    z_h = esub(zeta_n, (1, 0))
    masks = [(1, 0), esub(zeta, (finv(g), 0)), emul(z_h, einv(escale(esub(zeta, (1, 0)), n))),
             emul(z_h, einv(escale(esub(escale(zeta, g), (1, 0)), n)))]
    own = own_values_ext(blob, op_local, op_next, pis, masks)
    lc = logup_constraints_ext(lookups, degree, op_local, op_a, op_an, challenges)
    _need(len(lc) == n_constraints(lookups, degree), "constraint count")
    for j in range(2):
        acc = fold_full(own, lc, masks, (alphas[j], 0))
        s = (0, 0)
        for k in reversed(range(factor)):
            s = eadd(emul(s, zeta_n), op_q[j * factor + k])
        _need(acc == emul(z_h, s), "quotient identity")
    # 5. FRI
    gzeta = escale(zeta, g)

    def reduce(vals):
        acc = (0, 0)
        for v in reversed(vals):
            acc = eadd(emul(acc, fri_alpha), v)
        return acc
    red0, red1 = reduce(op_local + op_a + op_q), reduce(op_next + op_an)
    alpha_c = epow(fri_alpha, C_ + nA)
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


def verify(program_blob, cfg, proof, hasher):
    try:
        verify_or_raise(program_blob, cfg, proof, hasher)
        return True
    except Reject:
        return False


# ------------------------------------------------------------------------------------------------ the test AIRs and their traces
OWN_COLS, TABLE_COL = 3, 3  # columns 0 .. 2 carry the AIR's own constraints, column 3 is the table every lookup shares


def air_columns(m, n_lookups, extra=0):
    return OWN_COLS + 1 + n_lookups * (m + 1) + extra


def lookup_columns(m, l):
    """(looked-up columns, frequencies column) of lookup l"""
    first = OWN_COLS + 1 + l * (m + 1)
    return list(range(first, first + m)), first + m


def make_air(degree, m, n_lookups, extra=0):
    """The AIR of the LogUp tests, of the given degree (2, 3 or 5): its own constraints are permutation_ref.make_air's -- col1 = col0^2,
    col2 = a power of col0 that reaches the degree, next(col0) = col0 + 1 and the first row's col0 = PI0 -- column 3 is the table, and
    lookup l looks its m columns up in it with its own frequencies column (lookup_columns).  `extra` free columns widen it.  Returns the blob."""
    from starky_bls12_381_amd.air_builder import AirBuilder
    b = AirBuilder(air_columns(m, n_lookups, extra), 1, degree)
    b.constraint(b.L(1) - b.L(0) * b.L(0))
    if degree == 2:
        b.constraint(b.L(2) - b.L(0) * b.L(1))
    elif degree == 3:
        b.constraint(b.L(2) - b.L(0) * b.L(0) * b.L(0))
    else:
        b.constraint(b.L(2) - b.L(1) * b.L(1) * b.L(0))
        b.constraint(b.L(0) * b.L(1) * (b.L(2) - b.L(1) * b.L(1) * b.L(0)))
    b.transition(b.N(0) - b.L(0) - 1)
    b.first_row(b.L(0) - b.PI(0))
    for l in range(n_lookups):
        cols, freq = lookup_columns(m, l)
        b.logup(cols, TABLE_COL, freq)
    return b.finish()


def make_trace(degree, m, n_lookups, n_rows, seed, noncanonical=False, extra=0):
    """A trace of make_air(degree, m, n_lookups, extra) (row-major uint64) and its public inputs: the table holds n_rows distinct small
    values, every looked-up cell is one of them, and the frequencies are counted with numpy.  noncanonical: some cells of every named
    column are written as value + p (they are small, so that fits 64 bits)."""
    rng = np.random.default_rng(seed)
    start = int(rng.integers(1, 1 << 30))
    n_cols = air_columns(m, n_lookups, extra)
    t = np.zeros((n_rows, n_cols), dtype=np.uint64)
    for r in range(n_rows):
        x = (start + r) % P
        x2 = x * x % P
        t[r, 0], t[r, 1], t[r, 2] = x, x2, (x2 * x % P if degree in (2, 3) else x2 * x2 % P * x % P)
    table = (rng.permutation(n_rows).astype(np.uint64) * np.uint64(5) + np.uint64(11))
    t[:, TABLE_COL] = table
    order = np.argsort(table)
    for l in range(n_lookups):
        cols, freq = lookup_columns(m, l)
        picks = rng.integers(0, n_rows, size=(n_rows, m))
        t[:, cols[0]:cols[0] + m] = table[picks]
        t[:, freq] = np.bincount(picks.reshape(-1), minlength=n_rows).astype(np.uint64)
        assert (np.searchsorted(table[order], t[:, cols[0]:cols[0] + m]) < n_rows).all()
    if extra:
        t[:, n_cols - extra:] = rng.integers(0, 1 << 62, size=(n_rows, extra), dtype=np.uint64)
    if noncanonical:
        for r in range(0, n_rows, 3):
            for c in range(OWN_COLS, n_cols - extra):
                if int(t[r, c]) + P < 1 << 64:
                    t[r, c] = int(t[r, c]) + P
    return t, np.array([start], dtype=np.uint64)

"""Test-side reference for permutation arguments (COMPAT.md P1 - P8), on Python integers and independent of the C++: the Z
polynomials and closing products of a trace, the permutation constraints on an extension frame, and a mini-verifier of proofs with
nZ > 0 under either hasher.  Built from keccak_ref's Challenger, hashers, field helpers and constraints_ext (imported, not edited)."""
import numpy as np

from keccak_ref import (HASHERS, P, PROOF_MAGIC, Challenger, Reject, _merkle, _need, bitrev, constraints_ext, eadd, einv, emul, epow,
                        escale, esub, finv, reduction_arity_bits, root_of_unity)

AIR_PERM_MAGIC = 0x3153524941504D50


def split_program(blob):
    """(the program without its permutation section, the pairs as lists of (lhs, rhs)) of a constraint-program blob."""
    w = [int(x) for x in blob]
    base = 8 + w[5] + (w[6] + 1) // 2 + w[7]
    if len(w) == base:
        return np.array(w, dtype=np.uint64), []
    assert w[base] == AIR_PERM_MAGIC
    pairs, at = [], base + 2
    for _ in range(w[base + 1]):
        ne = w[at]
        pairs.append([(e & 0xFFFFFFFF, e >> 32) for e in w[at + 1:at + 1 + ne]])
        at += 1 + ne
    assert at == len(w)
    return np.array(w[:base], dtype=np.uint64), pairs


def batch_size(degree):
    return max(1, degree - 1)


def batches(pairs, degree):
    B = batch_size(degree)
    return [pairs[i:i + B] for i in range(0, len(pairs), B)]


def _beta_gamma(challenges, b, i):
    return int(challenges[(b * 2 + i) * 2]), int(challenges[(b * 2 + i) * 2 + 1])


def zs_and_closing(pairs, degree, rows, challenges):
    """P2.  rows: the trace as a list of rows of ints (any representative of a cell).  -> (zs [nZ][n], closing [nZ])"""
    zs, closing = [], []
    for b, batch in enumerate(batches(pairs, degree)):
        for i in range(2):
            beta, gamma = _beta_gamma(challenges, b, i)
            run, z = 1, []
            for row in rows:
                z.append(run)
                num = den = 1
                for pair in batch:
                    rl = rr = gamma
                    bp = 1
                    for lhs, rhs in pair:
                        rl = (rl + bp * (int(row[lhs]) % P)) % P
                        rr = (rr + bp * (int(row[rhs]) % P)) % P
                        bp = bp * beta % P
                    num = num * rl % P
                    den = den * rr % P
                run = run * num % P * finv(den) % P  # the inverse of 0 is 0 (P8): pow(0, p - 2, p)
            zs.append(z)
            closing.append(run)
    return zs, closing


def perm_constraints_ext(pairs, degree, local, zs, zs_next, challenges):
    """P4 on an extension frame, without masks: (the nZ first-row values Z_i - 1, the nZ plain values)."""
    first = [esub(z, (1, 0)) for z in zs]
    plain = []
    for b, batch in enumerate(batches(pairs, degree)):
        for i in range(2):
            beta, gamma = _beta_gamma(challenges, b, i)
            num = den = (1, 0)
            for pair in batch:
                rl = rr = (gamma, 0)
                bp = 1
                for lhs, rhs in pair:
                    rl = eadd(rl, escale(local[lhs], bp))
                    rr = eadd(rr, escale(local[rhs], bp))
                    bp = bp * beta % P
                num, den = emul(num, rl), emul(den, rr)
            z = 2 * b + i
            plain.append(esub(emul(zs_next[z], den), emul(zs[z], num)))
    return first, plain


def fold_full(own_values, first, plain, masks, alpha):
    """acc = acc alpha + mask c over the AIR's own (already masked) values, then the first-row and the plain permutation constraints."""
    acc = (0, 0)
    for v in own_values:
        acc = eadd(emul(acc, alpha), v)
    for v in first:
        acc = eadd(emul(acc, alpha), emul(masks[2], v))
    for v in plain:
        acc = eadd(emul(acc, alpha), v)
    return acc


def verify_or_raise(program_blob, cfg, proof, hasher):
    """keccak_ref.verify_or_raise for a proof of a program with permutation pairs: P1 (B challenge sets after the trace cap), P3 (the Z
    cap, then the alphas), P5 (openings local, zs, quotient, next, zs_next), P4 at zeta, P6 / P7 (the Z leaf's path and its share of
    fri_combine_initial in every query).  Raises Reject with the first failure, naming it."""
    h = HASHERS[hasher]
    blob, pairs = split_program(program_blob)
    w = [int(x) for x in proof]
    _need(len(w) >= 16 and w[0] == PROOF_MAGIC, "header")
    C_, Q, log_n, rate, cap_h, L, nq, final_len, n_pis, arity, n_ch, hid, nZ = w[1:14]
    _need(hid == hasher, "header names another hasher")
    degree = int(blob[3])
    factor = B = max(degree - 1, 1)
    _need(nZ == 2 * len(batches(pairs, degree)) and nZ > 0, "header word 13 (nZ)")
    _need(C_ == int(blob[1]) and n_pis == int(blob[2]) and n_ch == 2 == cfg.num_challenges and Q == 2 * factor, "shape")
    _need(rate == cfg.rate_bits and cap_h == cfg.cap_height and nq == cfg.num_query_rounds and arity == cfg.arity_bits, "config")
    arities = reduction_arity_bits(log_n, rate, cap_h, arity, cfg.final_poly_bits)
    _need(len(arities) == L and final_len == 1 << (log_n - sum(arities)), "FRI geometry")
    ncap, log_N, n = 1 << cap_h, log_n + rate, 1 << log_n
    N = 1 << log_N
    o = 16
    off_tcap = o; o += 4 * ncap
    off_zcap = o; o += 4 * ncap
    off_qcap = o; o += 4 * ncap
    off_local = o; o += 2 * C_
    off_next = o; o += 2 * C_
    off_zs = o; o += 2 * nZ
    off_zsn = o; o += 2 * nZ
    off_qopen = o; o += 2 * Q
    off_fcaps = o; o += L * 4 * ncap
    off_queries = o
    d0 = log_N - cap_h
    depths, lg = [], log_N
    for ab in arities:
        lg -= ab
        depths.append(lg - cap_h)
    qwords = C_ + nZ + Q + 12 * d0 + sum(2 * (1 << ab) + 4 * d for ab, d in zip(arities, depths))
    o += nq * qwords
    off_final = o; o += 2 * final_len
    off_pow = o; o += 1
    off_pis = o; o += n_pis
    _need(o == len(w), "length")
    _need(all(x < P for x in w[16:]), "a word is no field element")
    ext = lambda off, i: (w[off + 2 * i], w[off + 2 * i + 1])  # noqa: E731
    tcap, zcap, qcap = (w[off:off + 4 * ncap] for off in (off_tcap, off_zcap, off_qcap))
    fcaps = [w[off_fcaps + 4 * ncap * l:off_fcaps + 4 * ncap * (l + 1)] for l in range(L)]
    for cap in [tcap, zcap, qcap] + fcaps:
        _need(all(h.digest_ok(cap[4 * i:4 * i + 4]) for i in range(ncap)), "cap entry is no digest")
    op_local = [ext(off_local, i) for i in range(C_)]
    op_next = [ext(off_next, i) for i in range(C_)]
    op_z = [ext(off_zs, i) for i in range(nZ)]
    op_zn = [ext(off_zsn, i) for i in range(nZ)]
    op_q = [ext(off_qopen, i) for i in range(Q)]
    final_poly = [ext(off_final, i) for i in range(final_len)]
    pis = np.array(w[off_pis:off_pis + n_pis], dtype=np.uint64)

    # 1. the transcript
    ch = Challenger(h)
    ch.observe_many(tcap)
    challenges = [ch.get() for _ in range(4 * B)]  # P1: B sets of 2 x (beta, gamma), set-major, beta first
    ch.observe_many(zcap)
    alphas = [ch.get(), ch.get()]
    ch.observe_many(qcap)
    zeta = ch.get_ext()
    for group in (op_local, op_z, op_q, op_next, op_zn):
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
        zleaf = w[p:p + nZ]; p += nZ
        zsib = w[p:p + 4 * d0]; p += 4 * d0
        qleaf = w[p:p + Q]; p += Q
        qsib = w[p:p + 4 * d0]; p += 4 * d0
        x_index = indices[qi]
        _need(_merkle(h, tleaf, x_index, tcap, tsib), "trace path")
        _need(_merkle(h, zleaf, x_index, zcap, zsib), "permutation Z path")
        _need(_merkle(h, qleaf, x_index, qcap, qsib), "quotient path")
        steps = []
        for l, ab in enumerate(arities):
            ev = w[p:p + 2 * (1 << ab)]; p += 2 * (1 << ab)
            sib = w[p:p + 4 * depths[l]]; p += 4 * depths[l]
            x_index >>= ab
            _need(_merkle(h, ev, x_index, fcaps[l], sib), "FRI path")
            steps.append(ev)
        rounds.append((tleaf, zleaf, qleaf, steps))
    # 4. the quotient identity at zeta, over all K + 2 nZ constraints
    g = root_of_unity(log_n)
    zeta_n = epow(zeta, n)
    z_h = esub(zeta_n, (1, 0))
    masks = [(1, 0), esub(zeta, (finv(g), 0)), emul(z_h, einv(escale(esub(zeta, (1, 0)), n))),
             emul(z_h, einv(escale(esub(escale(zeta, g), (1, 0)), n)))]
    per_kind = constraints_ext(blob, op_local, op_next, pis)
    K = int(blob[4])
    own = []
    for k in range(K):
        val = (0, 0)
        for kind in range(4):
            val = eadd(val, emul(masks[kind], per_kind[kind][k]))
        own.append(val)
    first, plain = perm_constraints_ext(pairs, degree, op_local, op_z, op_zn, challenges)
    for j in range(2):
        acc = fold_full(own, first, plain, masks, (alphas[j], 0))
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
    red0, red1 = reduce(op_local + op_z + op_q), reduce(op_next + op_zn)
    alpha_c = epow(fri_alpha, C_ + nZ)
    wN = root_of_unity(log_N)
    for qi in range(nq):
        tleaf, zleaf, qleaf, steps = rounds[qi]
        x_index = indices[qi]
        x = 7 * pow(wN, bitrev(x_index, log_N), P) % P
        e0 = reduce([(v, 0) for v in tleaf + zleaf + qleaf])
        e1 = reduce([(v, 0) for v in tleaf + zleaf])
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
def make_air(degree, n_cols=6):
    """The AIR of the permutation tests: n_cols >= 6 columns of the given degree (2, 3 or 5; B = degree - 1).  Its permutation pairs: the
    three-entry pair {(0, 3), (1, 4), (2, 5)} (beta^2), then singletons, B + 1 pairs in all for B >= 2 -- two batches, the second with one
    instance -- and the one pair for B = 1 (more would be refused: n_batches <= B).  Degree 3 is the golden AIR: three pairs, two batches.
    Its own constraints: col1 = col0^2, col2 = a power of col0 that reaches the degree, next(col0) = col0 + 1 and the first row's
    col0 = PI0.  Columns 6 and up are free.  Returns the blob (AirBuilder)."""
    from starky_bls12_381_amd.air_builder import AirBuilder
    b = AirBuilder(n_cols, 1, degree)
    b.constraint(b.L(1) - b.L(0) * b.L(0))
    if degree == 2:
        b.constraint(b.L(2) - b.L(0) * b.L(1))  # col2 = col0^3, in degree-2 steps
    elif degree == 3:
        b.constraint(b.L(2) - b.L(0) * b.L(0) * b.L(0))
    else:  # degree 5: col2 = col0^5 through col1 = col0^2
        b.constraint(b.L(2) - b.L(1) * b.L(1) * b.L(0))
        b.constraint(b.L(0) * b.L(1) * (b.L(2) - b.L(1) * b.L(1) * b.L(0)))  # 2 gates + 3 factors: degree 5
    b.transition(b.N(0) - b.L(0) - 1)
    b.first_row(b.L(0) - b.PI(0))
    B = max(1, degree - 1)
    pairs = [[(0, 3), (1, 4), (2, 5)], [(0, 3)], [(1, 4)], [(2, 5)], [(0, 3)]]
    for p in pairs[:B + 1 if B >= 2 else 1]:
        b.permutation_pair(p)
    return b.finish()


def make_trace(degree, n_rows, seed, n_cols=6, noncanonical=False):
    """A trace of make_air(degree, n_cols) (row-major uint64) and its public inputs: columns 3 .. 5 are columns 0 .. 2 under one row
    permutation.  noncanonical: some cells are written as value + p where that fits 64 bits."""
    rng = np.random.default_rng(seed)
    start = int(rng.integers(1, 1 << 30))
    rows = []
    for r in range(n_rows):
        x = (start + r) % P
        x2 = x * x % P
        x3 = x2 * x % P if degree in (2, 3) else x2 * x2 % P * x % P
        rows.append([x, x2, x3])
    perm = rng.permutation(n_rows)
    full = [rows[r] + rows[int(perm[r])] + [int(v) for v in rng.integers(0, 1 << 62, n_cols - 6)] for r in range(n_rows)]
    if noncanonical:
        for r in range(0, n_rows, 3):
            for c in range(6):
                if full[r][c] + P < 1 << 64:
                    full[r][c] += P
    return np.array(full, dtype=np.uint64), np.array([start], dtype=np.uint64)

"""Test-side reference for the Keccak hasher (COMPAT.md K1 - K8) and a Python mini-verifier of a proof blob under either hasher.
No product code: Keccak-f and the sponge on Python integers, the digest encoding, the challenger's permutation with its word filter,
and verify(program_blob, cfg, proof, hasher) built on the oracle's pieces (oracle_lib: the Poseidon permutation, hash_no_pad,
two_to_one, and oracle_eval_frame for the constraints).  Field arithmetic is Goldilocks and its quadratic extension on integers."""
import numpy as np

import oracle_lib as O

P = 0xFFFFFFFF00000001
M64 = (1 << 64) - 1
PROOF_MAGIC = 0x3130304652505353
POSEIDON, KECCAK = 0, 1

# ------------------------------------------------------------------------------------------------ Keccak-f[1600] and the sponge
_ROT = [[0, 36, 3, 41, 18], [1, 44, 10, 45, 2], [62, 6, 43, 15, 61], [28, 55, 25, 21, 56], [27, 20, 39, 8, 14]]  # [x][y]


def _round_constants():
    out, r = [], 1
    for _ in range(24):
        v = 0
        for j in range(7):
            if r & 1:
                v |= 1 << ((1 << j) - 1)
            r <<= 1
            if r & 0x100:
                r ^= 0x171
        out.append(v)
    return out


_RC = _round_constants()


def _rol(v, n):
    return ((v << n) | (v >> (64 - n))) & M64 if n else v


def keccak_f(a):
    """a: 25 lanes, lane (x, y) at a[x + 5 y]; returns the permuted lanes."""
    a = list(a)
    for rc in _RC:
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        d = [c[(x - 1) % 5] ^ _rol(c[(x + 1) % 5], 1) for x in range(5)]
        b = [0] * 25
        for x in range(5):
            for y in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = _rol(a[x + 5 * y] ^ d[x], _ROT[x][y])
        for y in range(0, 25, 5):
            for x in range(5):
                a[y + x] = b[y + x] ^ (~b[y + (x + 1) % 5] & M64 & b[y + (x + 2) % 5])
        a[0] ^= rc
    return a


def sponge256(data, pad_byte):
    """Rate 136, capacity 512, 32 bytes out; pad_byte 0x01 is Keccak's padding, 0x06 SHA-3's."""
    data = bytes(data)
    padded = bytearray(data) + bytearray(136 - len(data) % 136)
    padded[len(data)] ^= pad_byte
    padded[-1] ^= 0x80
    a = [0] * 25
    for off in range(0, len(padded), 136):
        for i in range(17):
            a[i] ^= int.from_bytes(padded[off + 8 * i:off + 8 * i + 8], "little")
        a = keccak_f(a)
    return b"".join(a[i].to_bytes(8, "little") for i in range(4))


def keccak256(data):  # K1
    return sponge256(data, 0x01)


# ------------------------------------------------------------------------------------------------ K2 - K7 on integers
def digest_words(d25):  # K6: chunks of 7, 7, 7 and 4 bytes, little-endian
    assert len(d25) == 25
    return [int.from_bytes(d25[0:7], "little"), int.from_bytes(d25[7:14], "little"), int.from_bytes(d25[14:21], "little"),
            int.from_bytes(d25[21:25], "little")]


def words_digest(w):
    """The 25 bytes of a digest's four words, or None for words outside the ranges K6 leaves them in."""
    w = [int(x) for x in w]
    if w[0] >> 56 or w[1] >> 56 or w[2] >> 56 or w[3] >> 32:
        return None
    return w[0].to_bytes(7, "little") + w[1].to_bytes(7, "little") + w[2].to_bytes(7, "little") + w[3].to_bytes(4, "little")


def _element_bytes(elements):
    out = bytearray()
    for e in elements:
        e = int(e)
        assert 0 <= e < P
        out += e.to_bytes(8, "little")
    return bytes(out)


def hash_no_pad(elements):  # K3 (K2: the first 25 bytes)
    return digest_words(keccak256(_element_bytes(elements))[:25])


def hash_or_noop(elements):  # K4: 8 len <= 25 is copied
    b = _element_bytes(elements)
    if len(b) <= 25:
        return digest_words(b + bytes(25 - len(b)))
    return digest_words(keccak256(b)[:25])


def two_to_one(l, r):  # K5; None when either input is no digest
    lb, rb = words_digest(l), words_digest(r)
    if lb is None or rb is None:
        return None
    return digest_words(keccak256(lb + rb)[:25])


def state_from_words(words):
    """K7's filter: (the first 12 words below p, how many words were read), or None when there are fewer than 12 such words."""
    state, used = [], 0
    for w in words:
        used += 1
        if int(w) < P:
            state.append(int(w))
            if len(state) == 12:
                return state, used
    return None


def permute(state):  # K7
    h = _element_bytes(state)
    assert len(h) == 96
    words = []
    while True:
        h = keccak256(h)
        words += [int.from_bytes(h[8 * i:8 * i + 8], "little") for i in range(4)]
        got = state_from_words(words)
        if got:
            return got[0]


# ------------------------------------------------------------------------------------------------ the two hashers of the mini-verifier
class KeccakHasher:
    hid = KECCAK
    permute = staticmethod(permute)
    hash_or_noop = staticmethod(hash_or_noop)
    two_to_one = staticmethod(two_to_one)

    @staticmethod
    def digest_ok(w):
        return words_digest(w) is not None


O.lib.oracle_two_to_one.restype = None


class PoseidonHasher:
    hid = POSEIDON

    @staticmethod
    def permute(state):
        return [int(x) for x in O.poseidon_permute(np.array(state, dtype=np.uint64))]

    @staticmethod
    def hash_or_noop(elements):
        e = [int(x) for x in elements]
        if len(e) <= 4:
            return e + [0] * (4 - len(e))
        return [int(x) for x in O.hash_no_pad(np.array(e, dtype=np.uint64))]

    @staticmethod
    def two_to_one(l, r):
        a, b, out = (np.array([int(x) for x in l], dtype=np.uint64), np.array([int(x) for x in r], dtype=np.uint64),
                     np.zeros(4, dtype=np.uint64))
        O.lib.oracle_two_to_one(O._p(a), O._p(b), O._p(out))
        return [int(x) for x in out]

    @staticmethod
    def digest_ok(w):
        return True


HASHERS = {POSEIDON: PoseidonHasher, KECCAK: KeccakHasher}


class Challenger:  # rate 8, inputs overwrite, outputs pop from the end (K8)
    def __init__(self, hasher):
        self.h, self.state, self.inp, self.out = hasher, [0] * 12, [], []

    def _duplex(self):
        self.state[:len(self.inp)] = self.inp
        self.inp = []
        self.state = self.h.permute(self.state)
        self.out = self.state[:8]

    def observe(self, x):
        self.out = []
        self.inp.append(int(x))
        if len(self.inp) == 8:
            self._duplex()

    def observe_many(self, xs):
        for x in xs:
            self.observe(x)

    def get(self):
        if self.inp or not self.out:
            self._duplex()
        return self.out.pop()

    def get_ext(self):
        a = self.get()
        return (a, self.get())


# ------------------------------------------------------------------------------------------------ Goldilocks and F[X] / (X^2 - 7)
def finv(a):
    return pow(a, P - 2, P)


def eadd(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def esub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def emul(a, b):
    return ((a[0] * b[0] + 7 * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def escale(a, k):
    return (a[0] * k % P, a[1] * k % P)


def einv(a):
    d = finv((a[0] * a[0] - 7 * a[1] * a[1]) % P)
    return (a[0] * d % P, (P - a[1]) * d % P)


def epow(a, n):
    r = (1, 0)
    while n:
        if n & 1:
            r = emul(r, a)
        a = emul(a, a)
        n >>= 1
    return r


def root_of_unity(bits):
    return pow(7, (P - 1) >> bits, P)


def bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def reduction_arity_bits(log_n, rate_bits, cap_height, arity_bits, final_poly_bits):
    """plonky2 ConstantArityBits(arity_bits, final_poly_bits)"""
    out, db = [], log_n
    while db > final_poly_bits and db + rate_bits - arity_bits >= cap_height:
        out.append(arity_bits)
        db -= arity_bits
    return out


# ------------------------------------------------------------------------------------------------ the constraints at an extension point
MAX_DEGREE = 8  # the most a constraint program can reach (STARKHIP_AIR_MAX_DEGREE)


def constraints_ext(blob, local, nxt, pis):
    """Per kind k (plain, transition, first row, last row): every constraint's value at the extension frame (local, nxt) where the
    constraint is of kind k, else 0.  oracle_eval_frame works over the base field, so the frame v0 + t v1 is evaluated at
    t = 0 .. MAX_DEGREE: each constraint is a polynomial of degree <= MAX_DEGREE in t, and its value at t = X (X^2 = 7) is its value at
    the extension frame v0 + X v1."""
    npts = MAX_DEGREE + 1
    v0l, v1l = [a for a, _ in local], [b for _, b in local]
    v0n, v1n = [a for a, _ in nxt], [b for _, b in nxt]
    # Lagrange basis over t = 0 .. MAX_DEGREE as coefficient lists
    basis = []
    for i in range(npts):
        coef, den = [1], 1
        for j in range(npts):
            if j == i:
                continue
            coef = [((coef[k - 1] if k else 0) - j * (coef[k] if k < len(coef) else 0)) % P for k in range(len(coef) + 1)]
            den = den * (i - j) % P
        dinv = finv(den)
        basis.append([c * dinv % P for c in coef])
    # X^k in the extension
    xp = [(1, 0)]
    for _ in range(MAX_DEGREE):
        xp.append(emul(xp[-1], (0, 1)))
    out = []
    for kind in range(4):
        masks = [1 if k == kind else 0 for k in range(4)]
        vals = []
        for t in range(npts):
            lt = np.array([(a + t * b) % P for a, b in zip(v0l, v1l)], dtype=np.uint64)
            nt = np.array([(a + t * b) % P for a, b in zip(v0n, v1n)], dtype=np.uint64)
            vals.append([int(x) for x in O.eval_frame(blob, lt, nt, pis, np.array(masks, dtype=np.uint64))])
        per = []
        for k in range(len(vals[0])):
            acc = (0, 0)
            for deg in range(npts):
                cdeg = sum(vals[t][k] * basis[t][deg] for t in range(npts)) % P
                acc = eadd(acc, escale(xp[deg], cdeg))
            per.append(acc)
        out.append(per)
    return out


# ------------------------------------------------------------------------------------------------ the mini-verifier
class Reject(Exception):
    pass


def _need(cond, why):
    if not cond:
        raise Reject(why)


def _merkle(h, leaf, index, cap, siblings):
    cur = h.hash_or_noop(leaf)
    for d in range(len(siblings) // 4):
        sib = siblings[4 * d:4 * d + 4]
        _need(h.digest_ok(sib), "sibling is no digest")
        cur = h.two_to_one(sib, cur) if index & 1 else h.two_to_one(cur, sib)
        index >>= 1
    return cur == cap[4 * index:4 * index + 4]


def verify_or_raise(program_blob, cfg, proof, hasher):
    """Checks, in this order: the transcript replay (alphas, zeta, the FRI alpha and betas, the query indices), proof of work, every
    Merkle path of every query at the replayed index, the quotient identity at zeta, and FRI (initial combination, each fold, the
    final polynomial).  Raises Reject with the first failure."""
    h = HASHERS[hasher]
    blob = np.ascontiguousarray(program_blob, dtype=np.uint64)
    w = [int(x) for x in proof]
    _need(len(w) >= 16 and w[0] == PROOF_MAGIC, "header")
    C_, Q, log_n, rate, cap_h, L, nq, final_len, n_pis, arity, n_ch, hid = w[1:13]
    _need(hid == hasher, "header names another hasher")
    degree = int(blob[3])
    factor = max(degree - 1, 1)
    _need(C_ == int(blob[1]) and n_pis == int(blob[2]) and n_ch == 2 == cfg.num_challenges and Q == 2 * factor, "shape")
    _need(rate == cfg.rate_bits and cap_h == cfg.cap_height and nq == cfg.num_query_rounds and arity == cfg.arity_bits, "config")
    arities = reduction_arity_bits(log_n, rate, cap_h, arity, cfg.final_poly_bits)
    _need(len(arities) == L and final_len == 1 << (log_n - sum(arities)), "FRI geometry")
    ncap, log_N, n = 1 << cap_h, log_n + rate, 1 << log_n
    N = 1 << log_N
    o = 16
    off_tcap = o; o += 4 * ncap
    off_qcap = o; o += 4 * ncap
    off_local = o; o += 2 * C_
    off_next = o; o += 2 * C_
    off_qopen = o; o += 2 * Q
    off_fcaps = o; o += L * 4 * ncap
    off_queries = o
    d0 = log_N - cap_h
    depths, lg = [], log_N
    for ab in arities:
        lg -= ab
        depths.append(lg - cap_h)
    qwords = C_ + Q + 8 * d0 + sum(2 * (1 << ab) + 4 * d for ab, d in zip(arities, depths))
    o += nq * qwords
    off_final = o; o += 2 * final_len
    off_pow = o; o += 1
    off_pis = o; o += n_pis
    _need(o == len(w), "length")
    _need(all(x < P for x in w[16:]), "a word is no field element")
    ext = lambda off, i: (w[off + 2 * i], w[off + 2 * i + 1])  # noqa: E731
    tcap, qcap = w[off_tcap:off_tcap + 4 * ncap], w[off_qcap:off_qcap + 4 * ncap]
    fcaps = [w[off_fcaps + 4 * ncap * l:off_fcaps + 4 * ncap * (l + 1)] for l in range(L)]
    for cap in [tcap, qcap] + fcaps:
        _need(all(h.digest_ok(cap[4 * i:4 * i + 4]) for i in range(ncap)), "cap entry is no digest")
    op_local = [ext(off_local, i) for i in range(C_)]
    op_next = [ext(off_next, i) for i in range(C_)]
    op_q = [ext(off_qopen, i) for i in range(Q)]
    final_poly = [ext(off_final, i) for i in range(final_len)]
    pis = np.array(w[off_pis:off_pis + n_pis], dtype=np.uint64)

    # 1. the transcript
    ch = Challenger(h)
    ch.observe_many(tcap)
    alphas = [ch.get(), ch.get()]
    ch.observe_many(qcap)
    zeta = ch.get_ext()
    for group in (op_local, op_q, op_next):
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
        qleaf = w[p:p + Q]; p += Q
        qsib = w[p:p + 4 * d0]; p += 4 * d0
        x_index = indices[qi]
        _need(_merkle(h, tleaf, x_index, tcap, tsib), "trace path")
        _need(_merkle(h, qleaf, x_index, qcap, qsib), "quotient path")
        steps = []
        for l, ab in enumerate(arities):
            ev = w[p:p + 2 * (1 << ab)]; p += 2 * (1 << ab)
            sib = w[p:p + 4 * depths[l]]; p += 4 * depths[l]
            x_index >>= ab
            _need(_merkle(h, ev, x_index, fcaps[l], sib), "FRI path")
            steps.append(ev)
        rounds.append((tleaf, qleaf, steps))
    # 4. the quotient identity at zeta
    g = root_of_unity(log_n)
    zeta_n = epow(zeta, n)
    z_h = esub(zeta_n, (1, 0))
    masks = [(1, 0), esub(zeta, (finv(g), 0)), emul(z_h, einv(escale(esub(zeta, (1, 0)), n))),
             emul(z_h, einv(escale(esub(escale(zeta, g), (1, 0)), n)))]
    per_kind = constraints_ext(blob, op_local, op_next, pis)
    K = int(blob[4])
    for j in range(2):
        acc = (0, 0)
        for k in range(K):
            val = (0, 0)
            for kind in range(4):
                val = eadd(val, emul(masks[kind], per_kind[kind][k]))
            acc = eadd(escale(acc, alphas[j]), val)
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
    red0, red1 = reduce(op_local + op_q), reduce(op_next)
    alpha_c = epow(fri_alpha, C_)
    wN = root_of_unity(log_N)
    for qi in range(nq):
        tleaf, qleaf, steps = rounds[qi]
        x_index = indices[qi]
        x = 7 * pow(wN, bitrev(x_index, log_N), P) % P
        e0 = reduce([(v, 0) for v in tleaf + qleaf])
        e1 = reduce([(v, 0) for v in tleaf])
        old = eadd(emul(emul(esub(e0, red0), einv(esub((x, 0), zeta))), alpha_c), emul(esub(e1, red1), einv(esub((x, 0), gzeta))))
        for l, ab in enumerate(arities):
            ar = 1 << ab
            ev = steps[l]
            within = x_index & (ar - 1)
            _need((ev[2 * within], ev[2 * within + 1]) == old, "FRI coset value")
            # the coset x g^(-rev(within)) <g>, values stored bit-reversed; barycentric form over a coset of roots of unity:
            # f(beta) = (beta^ar - s^ar) / ar * sum_i e_i / ((beta - p_i) p_i^(ar - 1))
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

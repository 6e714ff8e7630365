"""What the generators of the leaf hash's scheduled asm blocks share (tools/gen_row_round_asm.py, gen_lane_round_asm.py,
gen_pair_round_asm.py): the instruction model, the table of gfx950 wait states and latencies, ONE list scheduler and ONE hazard checker
driven by that table, ONE interpreter of the instructions used (any number of lanes), the Poseidon round in Python integers to compare
against, and the instruction sequences every form is built from (multiply, multiply-add, fold, LDS load).  A generator holds its form's
register map, block builders, form-specific semantics and testers; it passes its table and lane count in -- nothing here is configured
by assigning to this module.
"""
import dataclasses
import random

P = 0xFFFFFFFF00000001
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
CIRC = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20]
SINK = 42            # s[42:43] in every form: takes the carry-outs nobody reads
MFMA_PIPE = 9999     # a pseudo register that chains the MFMAs (they share one pipe: issued closer than its occupancy they would stall the wave)

# ---------------------------------------------------------------- instruction model
VALU, DPP, SWAP, LOAD, MFMA, WAIT, NOP = "valu", "dpp", "swap", "load", "mfma", "wait", "nop"   # Ins.kind; SWAP: v_permlane32_swap, LOAD: ds_read


class Ins:
    """text; VGPRs / SGPR pairs read and written; kind; sem: what the interpreter executes; boost: scheduled as early as possible;
    junk: registers an MFMA fills with rows nobody may read"""

    def __init__(self, text, reads=(), writes=(), sreads=(), swrites=(), kind=VALU, sem=None, boost=False, junk=()):
        self.text, self.reads, self.writes, self.sreads, self.swrites = text, set(reads), set(writes), set(sreads), set(swrites)
        self.kind, self.sem, self.boost, self.junk = kind, sem, boost, set(junk)


def v(n):
    return "v%d" % n


def vp(n):
    assert n % 2 == 0, "64-bit VGPR operands are even-aligned on gfx950"
    return "v[%d:%d]" % (n, n + 1)


def sp(n):
    return "s[%d:%d]" % (n, n + 1)


# ---------------------------------------------------------------- hazard table
@dataclasses.dataclass(frozen=True)
class Hazards:
    """issue slots a consumer stays behind its producer.  Every form builds its own; one whose blocks never read what they load, or hold no
    MFMA, leaves those distances out (None: using one fails loudly)"""
    valu_raw: int        # VALU result -> VALU read
    sgpr_raw: int        # W1: VALU-written SGPR (carry / borrow) -> VALU read
    dpp_read: int        # W2: VGPR write -> DPP move or lane swap reading it
    war: int             # W3: VGPR read -> overwrite
    war_load: int        # ... by an LDS load (it lands much later anyway)
    load_latency: int = None    # LDS load -> first use the scheduler aims for (s_waitcnt keeps it correct)
    mfma_result: int = None     # MFMA -> first read or overwrite of its result
    mfma_spacing: int = None    # MFMA -> next MFMA
    mfma_operand: int = None    # VALU write -> MFMA reading it
    mfma_war: int = None        # MFMA operand read -> overwrite

    def raw(self, producer, consumer, reg):
        if producer.kind == LOAD:
            return self.load_latency
        if producer.kind == MFMA:
            return self.mfma_spacing if reg == MFMA_PIPE else self.mfma_result
        if consumer.kind == MFMA:
            return self.mfma_operand
        return self.dpp_read if consumer.kind in (DPP, SWAP) else self.valu_raw

    def waw(self, first, reg):
        return self.mfma_result if first.kind == MFMA and reg != MFMA_PIPE else 1

    def war_of(self, reader, writer):
        return self.mfma_war if reader.kind == MFMA else self.war_load if writer.kind == LOAD else self.war


# ---------------------------------------------------------------- list scheduler
def schedule(prog, t):
    """orders prog under the distances of Hazards t: critical path first, loads (boost) as early as they can go, s_nop where nothing is ready"""
    n = len(prog)
    preds = [[] for _ in range(n)]
    last_w, last_sw, readers, sreaders = {}, {}, {}, {}
    for i, ins in enumerate(prog):
        for r in ins.reads:
            if r in last_w:
                preds[i].append((last_w[r], t.raw(prog[last_w[r]], ins, r)))
        for r in ins.sreads:
            if r in last_sw:
                preds[i].append((last_sw[r], t.sgpr_raw))
        for w in ins.writes:
            if w in last_w:
                preds[i].append((last_w[w], t.waw(prog[last_w[w]], w)))
            for j in readers.get(w, []):
                if j != i:
                    preds[i].append((j, t.war_of(prog[j], ins)))
        for w in ins.swrites:
            if w in last_sw:
                preds[i].append((last_sw[w], 1))
            for j in sreaders.get(w, []):
                if j != i:
                    preds[i].append((j, 1))
        for r in ins.reads:
            readers.setdefault(r, []).append(i)
        for r in ins.sreads:
            sreaders.setdefault(r, []).append(i)
        for w in ins.writes:
            last_w[w] = i
            readers[w] = [i] if w in ins.reads else []
        for w in ins.swrites:
            last_sw[w] = i
            sreaders[w] = []
    succs = [[] for _ in range(n)]
    for i in range(n):
        for j, d in preds[i]:
            succs[j].append((i, d))
    prio = [0] * n
    for i in reversed(range(n)):
        prio[i] = 1 + max([prio[k] + d - 1 for k, d in succs[i]] + [0]) + (1000 if prog[i].boost else 0)
    pos, order, slot, remaining = {}, [], 0, set(range(n))
    while remaining:
        ready = [i for i in remaining if all(j in pos and pos[j] + d <= slot for j, d in preds[i])]
        if ready:
            i = max(ready, key=lambda k: (prio[k], -k))
            pos[i] = slot
            order.append(prog[i])
            remaining.discard(i)
        else:
            order.append(Ins("s_nop 0", kind=NOP))
        slot += 1
    return order


def count_waits(order, load_latency):
    """a pass after schedule(): the s_waitcnt in front of every first use of a loaded register, COUNTED (LDS returns in order: lgkmcnt(k)
    with k = the loads issued since the one needed).  The scheduler kept that use load_latency slots behind the load where it could."""
    out, pending = [], []          # pending: loads in issue order: (registers, position of issue)
    for ins in order:
        if ins.kind == LOAD:
            pending.append((set(ins.writes), len(out)))
            assert len(pending) <= 15
            out.append(ins)
            continue
        need = -1
        touched = ins.reads | ins.writes
        for i, (regs, _) in enumerate(pending):
            if regs & touched:
                need = i
        if need >= 0:
            # the wait also covers the later loads that were issued long enough ago to be back: one wait per row instead of one per load
            while need + 1 < len(pending) and pending[need + 1][1] <= len(out) - load_latency:
                need += 1
            left = len(pending) - 1 - need
            out.append(Ins("s_waitcnt lgkmcnt(%d)" % left, kind=WAIT))
            pending = pending[need + 1:]
        out.append(ins)
    return out


# ---------------------------------------------------------------- hazard checker
def check_hazards(order, t, inputs=frozenset()):
    """the final order (waits and s_nop included) keeps every distance of Hazards t; inputs: registers the caller's code may have written
    right before the block"""
    last_mfma_write, last_mfma_read, last_valu_write, last_mfma = {}, {}, {}, None
    junk_since = {}   # registers an MFMA fills with junk rows: dead until something writes them again
    for i, ins in enumerate(order):
        for back in range(1, t.sgpr_raw):
            assert i - back < 0 or not (ins.sreads & order[i - back].swrites), ("W1", i, ins.text)
        if ins.kind in (DPP, SWAP):
            for back in range(1, t.dpp_read):
                assert not (ins.reads & (order[i - back].writes if i - back >= 0 else inputs)), ("W2", i, ins.text)
        if ins.kind not in (LOAD, WAIT):
            for back in range(1, t.war):
                assert i - back < 0 or not (ins.writes & (order[i - back].reads - order[i - back].writes)), ("W3", i, ins.text)
        m = ins.kind == MFMA
        for r in ins.reads:
            assert r not in junk_since, ("reads an MFMA's junk row", i, ins.text)
            if r in last_mfma_write and r != MFMA_PIPE:
                assert i - last_mfma_write[r] >= t.mfma_result, ("MFMA result read too early", i, ins.text)
            if m and r in last_valu_write and r != MFMA_PIPE:
                assert i - last_valu_write[r] >= t.mfma_operand, ("MFMA operand written too late", i, ins.text)
        for w in ins.writes - {MFMA_PIPE}:
            if w in junk_since:
                assert m or i - junk_since[w] >= t.mfma_result, ("writes where an MFMA's junk row is still to land", i, ins.text)
                del junk_since[w]
            if w in last_mfma_read and ins.kind != LOAD:
                assert i - last_mfma_read[w] >= t.mfma_war, ("MFMA operand overwritten too early", i, ins.text)
            if w in last_mfma_write:
                assert i - last_mfma_write[w] >= t.mfma_result, ("MFMA result overwritten too early", i, ins.text)
        if m:
            assert last_mfma is None or i - last_mfma >= t.mfma_spacing, ("MFMAs too close", i)
            last_mfma = i
            junk_since.update((w, i) for w in ins.junk)
            last_mfma_read.update((r, i) for r in ins.reads)
            last_mfma_write.update((w, i) for w in ins.writes)
        else:
            for w in ins.writes:
                last_valu_write[w] = i
                last_mfma_write.pop(w, None)


# ---------------------------------------------------------------- interpreter
class Machine:
    """register files of `lanes` lanes: vregs / sregs map a register number to a list of per-lane values; vregs["mem"][key] is what an
    LDS load with that key returns (a list of per-lane lists, one per register)"""

    def __init__(self, vregs, sregs, lanes):
        self.vregs, self.sregs, self.n = vregs, sregs, lanes

    def V(self, r):
        return self.vregs.setdefault(r, [0] * self.n)

    def S(self, r):
        return self.sregs.setdefault(r, [0] * self.n)

    def V64(self, r):
        return [lo | (hi << 32) for lo, hi in zip(self.V(r), self.V(r + 1))]

    def set64(self, d, xs):
        self.vregs[d], self.vregs[d + 1] = [x & M32 for x in xs], [(x >> 32) & M32 for x in xs]


def _opt(m, r):
    return [0] * m.n if r is None else m.V(r)


def _ldsload(m, ins, first, count, key):
    for q in range(count):
        m.vregs[first + q] = list(m.vregs["mem"][key][q])


def _mad(m, ins, d, cout, a, b, c):
    """d (pair) = a * b + c (pair); b: a register, "eps" = 2^32 - 1 or ("const", k); cout: the SGPR pair of the carry-out or None"""
    bs = [M32] * m.n if b == "eps" else [b[1]] * m.n if isinstance(b, tuple) else m.V(b)
    x = [ai * bi + ci for ai, bi, ci in zip(m.V(a), bs, [0] * m.n if c is None else m.V64(c))]
    m.set64(d, x)
    if cout is not None:
        m.sregs[cout] = [t >> 64 for t in x]
    else:
        assert not any(t >> 64 for t in x), ("a multiply-add whose carry-out nobody reads overflowed", ins.text)


def _mov(m, ins, d, s):
    m.vregs[d] = m.V(s)[:]


def _mov64(m, ins, d, s):
    m.vregs[d], m.vregs[d + 1] = m.V(s)[:], m.V(s + 1)[:]


def _subb(m, ins, d, bout, a, b, bin_):
    x = [ai - bi - ci for ai, bi, ci in zip(_opt(m, a), _opt(m, b), m.S(bin_))]
    m.vregs[d] = [t & M32 for t in x]
    if bout is not None:
        m.sregs[bout] = [1 if t < 0 else 0 for t in x]


def _addc(m, ins, d, _cout, a, _b, cin):
    m.vregs[d] = [(ai + ci) & M32 for ai, ci in zip(_opt(m, a), m.S(cin))]


def _addco(m, ins, d, cout, a, b):
    x = [ai + bi for ai, bi in zip(m.V(a), m.V(b))]
    m.vregs[d], m.sregs[cout] = [t & M32 for t in x], [t >> 32 for t in x]


def _madi(m, ins, d, t):
    """d (pair) -= t read as a signed dword"""
    m.set64(d, [(x - (tv - (1 << 32) if tv >> 31 else tv)) & M64 for x, tv in zip(m.V64(d), m.V(t))])


def _add(m, ins, d, a, b):
    m.vregs[d] = [(ai + bi) & M32 for ai, bi in zip(m.V(a), m.V(b))]


def _add64(m, ins, d, a, b):
    m.set64(d, [(x + y) & M64 for x, y in zip(m.V64(a), m.V64(b))])


def _dpp(m, ins, d, s, kind, bank, bound):
    assert m.n == 16, "a DPP move works on a row of 16 lanes"
    src, out = m.V(s)[:], m.V(d)[:]
    for l in range(16):
        if not (bank >> (l // 4)) & 1:
            continue
        j = {"shl": lambda k: l + k, "shr": lambda k: l - k, "ror": lambda k: (l - k) % 16, "quad": lambda sel: (l & ~3) + sel[l & 3]}[kind[0]](kind[1])
        if 0 <= j < 16:
            out[l] = src[j]
        elif bound:
            out[l] = 0
    m.vregs[d] = out


def _cnd(m, ins, d, a, b, mask):
    m.vregs[d] = [bi if mi else ai for ai, bi, mi in zip(_opt(m, a), _opt(m, b), m.S(mask))]


def _perm(m, ins, d, s0, s1, selector):
    """v_perm_b32: byte i of d = byte selector.byte[i] of (s0 : s1)"""
    m.vregs[d] = [sum(((((hi << 32) | lo) >> (8 * ((selector >> (8 * i)) & 0xFF))) & 0xFF) << (8 * i) for i in range(4)) for hi, lo in zip(m.V(s0), m.V(s1))]


def _xor80(m, ins, d):
    m.vregs[d] = [x ^ 0x80808080 for x in m.V(d)]


def _lshladd(m, ins, d, a, sh, b):
    m.vregs[d] = [((ai << sh) + bi) & M32 for ai, bi in zip(m.V(a), m.V(b))]


def _swap32(m, ins, a, b):
    """v_permlane32_swap_b32: the upper half-wave's a <-> the lower half-wave's b"""
    h, va, vb = m.n // 2, m.V(a), m.V(b)
    assert m.n % 2 == 0
    m.vregs[a], m.vregs[b] = va[:h] + vb[:h], va[h:] + vb[h:]


SEMANTICS = {"ldsload": _ldsload, "mad": _mad, "mov": _mov, "mov64": _mov64, "subb": _subb, "addc": _addc, "addco": _addco,
             "madi": _madi, "add": _add, "add64": _add64, "dpp": _dpp, "cnd": _cnd, "perm": _perm, "xor80": _xor80, "lshladd": _lshladd, "swap32": _swap32}


def run(order, vregs, sregs, lanes, extra=None):
    """executes order on `lanes` lanes; extra: {sem kind: f(machine, ins, *sem[1:])} for a form's own instructions (its MFMA)"""
    m = Machine(vregs, sregs, lanes)
    sems = dict(SEMANTICS, **(extra or {}))
    for ins in order:
        if ins.sem is not None:
            sems[ins.sem[0]](m, ins, *ins.sem[1:])


# ---------------------------------------------------------------- the rounds in Python integers
def edge_value():
    return random.choice([0, 1, P - 1, P, M64, random.getrandbits(64), random.getrandbits(64)])


def mds_coef(r, j):
    return CIRC[(j - r) % 12] + (8 if r == 0 and j == 0 else 0)


def reference_round(state, rc_next, partial):
    s = [pow(x, 7, P) if (not partial or e == 0) else x % P for e, x in enumerate(state)]
    return [(sum(mds_coef(e, j) * s[j] for j in range(12)) + rc_next[e]) % P for e in range(12)]


def merged_tables(cs):
    """poseidon_merged.h on Python integers for n = len(cs) merged partial rounds with the following rounds' constants cs = [c1 .. cn]:
    ([M, N2 .. Nn], [k1 .. kn]) with N_k = M Mz^(k-1), k1 .. k(n-1) scalars and kn a vector (the formulas: gen_lane_round_asm.py)"""
    M = [[mds_coef(i, j) for j in range(12)] for i in range(12)]
    Mz = [[0] * 12 if i == 0 else M[i][:] for i in range(12)]
    N = [M]
    for _ in cs[1:]:
        N.append([[sum(N[-1][i][k] * Mz[k][j] for k in range(12)) for j in range(12)] for i in range(12)])

    def k(i, g):   # element g of  c_i + sum_{m < i} N_(i-m) c_m with element 0 zeroed
        return (cs[i][g] + sum(N[i - m - 1][g][j] * cs[m][j] for m in range(i) for j in range(1, 12))) % P
    n = len(cs)
    return N, [k(i, 0) for i in range(n - 1)] + [[k(n - 1, g) for g in range(12)]]


# ---------------------------------------------------------------- instruction builders
class Slot:
    """a multiply's temporaries: eight VGPRs from `base`, the addend pair (ad, a register the caller keeps zero), four SGPR pairs from `flags`"""

    def __init__(self, base, ad, flags):
        self.P0, self.M, self.P3, self.t, self.AD = base, base + 2, base + 4, base + 6, ad
        self.CM, self.BR, self.BR2, self.CY = flags, flags + 2, flags + 4, flags + 6


def mul(prog, dst, a, b, s):
    """dst = a * b mod p (any representative): gl_dev.h's gl_mul_nc, 13 instructions.  a, b: (lo, hi) registers; dst: even pair."""
    a0, a1 = a
    b0, b1 = b
    R, AD = dst, s.AD
    prog += [
        Ins("v_mad_u64_u32 %s, %s, %s, %s, 0" % (vp(s.P0), sp(SINK), v(a0), v(b0)), [a0, b0], [s.P0, s.P0 + 1], sem=("mad", s.P0, None, a0, b0, None)),
        Ins("v_mov_b32 %s, %s" % (v(AD), v(s.P0 + 1)), [s.P0 + 1], [AD], sem=("mov", AD, s.P0 + 1)),
        Ins("v_mad_u64_u32 %s, %s, %s, %s, %s" % (vp(s.M), sp(SINK), v(a0), v(b1), vp(AD)), [a0, b1, AD, AD + 1], [s.M, s.M + 1], sem=("mad", s.M, None, a0, b1, AD)),
        Ins("v_mad_u64_u32 %s, %s, %s, %s, %s" % (vp(s.M), sp(s.CM), v(a1), v(b0), vp(s.M)), [a1, b0, s.M, s.M + 1], [s.M, s.M + 1], swrites=[s.CM],
            sem=("mad", s.M, s.CM, a1, b0, s.M)),
        Ins("v_mov_b32 %s, %s" % (v(AD), v(s.M + 1)), [s.M + 1], [AD], sem=("mov", AD, s.M + 1)),
        Ins("v_mad_u64_u32 %s, %s, %s, %s, %s" % (vp(s.P3), sp(SINK), v(a1), v(b1), vp(AD)), [a1, b1, AD, AD + 1], [s.P3, s.P3 + 1], sem=("mad", s.P3, None, a1, b1, AD)),
        # D = (l1 : l0) - h1 - cin, in place over P0
        Ins("v_subb_co_u32 %s, %s, %s, %s, %s" % (v(s.P0), sp(s.BR), v(s.P0), v(s.P3 + 1), sp(s.CM)), [s.P0, s.P3 + 1], [s.P0], sreads=[s.CM], swrites=[s.BR],
            sem=("subb", s.P0, s.BR, s.P0, s.P3 + 1, s.CM)),
        Ins("v_subb_co_u32 %s, %s, %s, 0, %s" % (v(s.P0 + 1), sp(s.BR2), v(s.M), sp(s.BR)), [s.M], [s.P0 + 1], sreads=[s.BR], swrites=[s.BR2],
            sem=("subb", s.P0 + 1, s.BR2, s.M, None, s.BR)),
        Ins("v_mad_u64_u32 %s, %s, %s, -1, %s" % (vp(R), sp(s.CY), v(s.P3), vp(s.P0)), [s.P3, s.P0, s.P0 + 1], [R, R + 1], swrites=[s.CY],
            sem=("mad", R, s.CY, s.P3, "eps", s.P0)),
        Ins("v_subb_co_u32 %s, %s, 0, 0, %s" % (v(s.t), sp(SINK), sp(s.BR2)), [], [s.t], sreads=[s.BR2], sem=("subb", s.t, None, None, None, s.BR2)),
        Ins("v_addc_co_u32 %s, %s, %s, 0, %s" % (v(s.t), sp(SINK), v(s.t), sp(s.CY)), [s.t], [s.t], sreads=[s.CY], sem=("addc", s.t, None, s.t, None, s.CY)),
        Ins("v_mad_i64_i32 %s, %s, %s, -1, %s" % (vp(R), sp(SINK), v(s.t), vp(R)), [s.t, R, R + 1], [R, R + 1], sem=("madi", R, s.t)),
        Ins("v_add_u32 %s, %s, %s" % (v(R + 1), v(s.t), v(R + 1)), [s.t, R + 1], [R + 1], sem=("add", R + 1, s.t, R + 1)),
    ]


def madc(prog, acc, src, coef, seed=None):
    """acc (pair) = src * coef + (seed or acc); coef: an inline constant or ('v', register)"""
    add = acc if seed is None else seed
    if isinstance(coef, tuple):
        prog.append(Ins("v_mad_u64_u32 %s, %s, %s, %s, %s" % (vp(acc), sp(SINK), v(src), v(coef[1]), vp(add)), [src, coef[1], add, add + 1], [acc, acc + 1],
                        sem=("mad", acc, None, src, coef[1], add)))
    else:
        prog.append(Ins("v_mad_u64_u32 %s, %s, %s, %d, %s" % (vp(acc), sp(SINK), v(src), coef, vp(add)), [src, add, add + 1], [acc, acc + 1],
                        sem=("mad", acc, None, src, ("const", coef), add)))


def mad_eps(prog, dst, src, add, cout=None):
    """dst (pair) = src * (2^32 - 1) + add (pair)"""
    prog.append(Ins("v_mad_u64_u32 %s, %s, %s, -1, %s" % (vp(dst), sp(SINK if cout is None else cout), v(src), vp(add)), [src, add, add + 1], [dst, dst + 1],
                    swrites=[] if cout is None else [cout], sem=("mad", dst, cout, src, "eps", add)))


def addc(prog, dst, src, cin):
    """dst = (src or 0) + the carry in SGPR pair cin"""
    prog.append(Ins("v_addc_co_u32 %s, %s, %s, 0, %s" % (v(dst), sp(SINK), "0" if src is None else v(src), sp(cin)), [] if src is None else [src], [dst], sreads=[cin],
                    sem=("addc", dst, None, src, None, cin)))


def addco(prog, reg, src, cout):
    prog.append(Ins("v_add_co_u32 %s, %s, %s, %s" % (v(reg), sp(cout), v(reg), v(src)), [reg, src], [reg], swrites=[cout], sem=("addco", reg, cout, reg, src)))


def fold(prog, dst, A, B, FT, CV, FC):
    """v[dst:dst+1] = A + B * 2^32 mod p (combine_lohi_nc) for accumulators below 2^57; temporaries: the pair FT, CV, the SGPR pair FC"""
    mad_eps(prog, FT, B + 1, A)
    addco(prog, FT + 1, B, FC)
    addc(prog, CV, None, FC)
    mad_eps(prog, dst, CV, FT)


def fold_big(prog, dst, A, B, FT, CV, FC, C2):
    """dst = A + B 2^32 mod p (some representative) for 64-bit A and B with B < 2^64 - 2^32:
        A + B 2^32 = A_lo + (A_hi + B_lo) 2^32 + B_hi 2^64 = (s : A_lo) + (B_hi + c) eps   mod p,   s + c 2^32 = A_hi + B_lo
    -- one addition with carry-out in place, the carry into B_hi (which cannot wrap), one multiply-add whose own carry-out (into C2) is
    worth eps once more (after it the sum is below (B_hi + c) eps < 2^64 - 2^32, so that last correction cannot overflow).  Five
    instructions; A is consumed."""
    addco(prog, A + 1, B, FC)
    addc(prog, CV, B + 1, FC)
    mad_eps(prog, FT, CV, A, cout=C2)
    addc(prog, CV, None, C2)
    mad_eps(prog, dst, CV, FT)


def load(prog, first, count, addr, off, key):
    """v[first .. first + count - 1] = LDS at v[addr] + off (a number, or an asm operand such as "%[off]"); the interpreter takes vregs["mem"][key]"""
    op = {4: "ds_read_b128", 2: "ds_read_b64", 1: "ds_read_b32"}[count]
    rng = "v[%d:%d]" % (first, first + count - 1) if count > 1 else v(first)
    prog.append(Ins("%s %s, %s offset:%s" % (op, rng, v(addr), off), [addr], range(first, first + count), kind=LOAD, sem=("ldsload", first, count, key), boost=True))


def mov64(prog, dst, src):
    prog.append(Ins("v_mov_b64 %s, %s" % (vp(dst), vp(src)), [src, src + 1], [dst, dst + 1], sem=("mov64", dst, src)))


def add64(prog, dst, a, b):
    prog.append(Ins("v_lshl_add_u64 %s, %s, 0, %s" % (vp(dst), vp(a), vp(b)), [a, a + 1, b, b + 1], [dst, dst + 1], sem=("add64", dst, a, b)))


def cndmask(prog, dst, a, b, mask):
    """dst = mask ? b : a; a, b: register numbers or None for the literal 0"""
    prog.append(Ins("v_cndmask_b32 %s, %s, %s, %s" % (v(dst), "0" if a is None else v(a), "0" if b is None else v(b), sp(mask)), [r for r in (a, b) if r is not None], [dst],
                    sem=("cnd", dst, a, b, mask)))


# ---------------------------------------------------------------- output
def emit(name, order, what, loads=False):
    count = {k: sum(1 for o in order if o.kind == k) for k in (LOAD, WAIT, NOP)}
    detail = "%d LDS loads, %d s_waitcnt, %d s_nop" % (count[LOAD], count[WAIT], count[NOP]) if loads else "%d s_nop" % count[NOP]
    print("// %s: %d instructions (%s)" % (what, len(order), detail))
    print("#define %s \\" % name)
    for i, o in enumerate(order):
        last = i == len(order) - 1
        print('    "%s%s"%s' % (o.text, "" if last else "\\n\\t", "" if last else " \\"))


def define(name, operand):
    print('#define %s "%s"' % (name, operand))


def clobbers(name, vregs, sregs=()):
    print("#define %s %s" % (name, ", ".join(['"v%d"' % r for r in vregs] + ['"s%d"' % r for r in sregs])))

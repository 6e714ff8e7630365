#!/usr/bin/env python3
"""Generates csrc/row_round_asm.inc: one whole round of the ROW form of the Poseidon permutation (poseidon_dev.h:
poseidon_permute_row) as ONE scheduled inline-asm block on fixed physical registers -- S-box, circulant layer, fold.

The row form exists for commitments too small to fill the chip: a lone wave issues one instruction per ~5 cycles whatever it
depends on, and every wait state that hipcc fills with s_nop is a lost slot.  The wait states this code meets on gfx950:
  W1  a VALU may read an SGPR (carry / borrow flag) two instructions after the VALU that wrote it, not earlier;
  W2  a DPP move may read a VGPR two instructions after it was written;
  W3  a VGPR may not be written in the slot right after an instruction that read it.
A list scheduler orders each block under those rules.  What makes the difference is what it is given to fill the slots with:
  * full round: x^3 and x^4 of the S-box are independent multiplies;
  * partial round: only lane 0's element passes the S-box, and  M s' = M (s with element 0 zeroed) + (column 0 of M) x0^7, so the
    whole circulant layer over the other eleven elements is issued UNDER lane 0's three dependent multiplies, and x0^7 enters at
    the end as one broadcast (three DPP moves per half) and two multiply-adds with a per-lane coefficient.
Inline asm cannot name the halves of an operand pair, so every operand is bound to a physical register ("{v231}") and the text
uses register names; temporaries are clobbers.  Every block is executed here by an interpreter of the instructions used, on random
16-lane rows, against the round computed with Python integers.

The instruction model, the scheduler, the hazard checker, the interpreter and the multiply / multiply-add / fold sequences are
tools/asm_blocks.py, shared with the lane and pair forms' generators; here are the row form's register map, its DPP moves, blocks and testers.

    python tools/gen_row_round_asm.py > starky_bls12_381_amd/csrc/row_round_asm.inc
"""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import asm_blocks as AB  # noqa: E402
from asm_blocks import CIRC, M32, P, SINK, Ins, add64, cndmask, madc, mul, v  # noqa: E402

NL = 16
HAZARDS = AB.Hazards(valu_raw=1, sgpr_raw=3, dpp_read=3, war=2, war_load=1)   # no block reads what it loads (the wait opens the next block)

# ---------------------------------------------------------------- register map (VGPRs 176 .. 255, SGPRs 40 .. 99)
ADDR = 175                     # in: LDS address of this lane's round-constant row (RcPair rc[32])
S_LO, S_HI = 176, 177          # in: the lane's state word; out: the new one (v[176:177])
SEED_A, SEED_B = 178, 180      # in: the next round's constant, low half and high half, as 64-bit addends; out: the same for the round
                               # after (the block reloads v[178:181] from LDS as soon as it has consumed them: the load's latency
                               # passes under the rest of the round instead of in front of the next one)
C0, COL0 = 182, 183            # in: 17 (+ 8 on lane 0); column 0 of the MDS matrix at this lane (partial rounds)
ZA, ZB = 185, 187              # in: zero (upper halves of the two multiply slots' addend pairs v[184:185], v[186:187])
ACC_A, ACC_B = 188, 190        # the layer's two accumulators
FT, CV = 192, 194              # fold: T pair, carry value
X2, X3, X4, X7, SEL, YN, BC = 196, 198, 200, 202, 204, 206, 208   # S-box values (pairs)
SZ = 210                       # the state with lane 0 zeroed (pair)
ROT = 212                      # rotated operands of the layer: 24 registers 212 .. 235 (+ z, w copies 236 .. 239)
ZC, WC = 236, 238
SLOT = [240, 248]              # two multiply slots of eight registers
MASK0 = 40                     # in: lane-0 mask (bit 0 of every row)
FLAG = [44, 52]                # per slot: CM, BR, BR2, CY pairs
FC = 60
MASKE = 62                     # in: even lanes (the uniform S-box of the merged triple)
# the merged triple's operands and extra temporaries
N3K = 140                      # in: 12 registers, coefficient of the operand rotated by k: N3[e][(e + k) mod 12]
R1, R2, B2, B3 = 152, 153, 154, 155      # in: M[0][e], N2[0][e], N2[e][0], M[e][0]
N3C0, L0M, L0N = 156, 157, 158           # in: N3[e][0]; M[0][0] and N2[0][0] on lane 0, 0 elsewhere
K1, K2, K3 = 160, 164, 168     # in / out: the triple's constants, each (low half, high half) as two 64-bit addends; k1, k2 on lane 0 only
D1A, D1B, D2A, D2B = 122, 124, 126, 128  # the two dot products' accumulators
RT = 130                       # all-reduce: rotated copies (two pairs)
YY, XS2, XS3 = 134, 136, 138   # y (folded), x2, x3
SEEDS = [SEED_A, SEED_A + 1, SEED_B, SEED_B + 1]


def slot(k):
    return AB.Slot(SLOT[k], (184, 186)[k], FLAG[k])


def dpp(prog, dst, src, ctrl, bank=0xF, bound=True, kind=None):
    text = "v_mov_b32_dpp %s, %s %s row_mask:0xf bank_mask:0x%x%s" % (v(dst), v(src), ctrl, bank, " bound_ctrl:1" if bound else "")
    reads = [src] if bound and bank == 0xF else [src, dst]   # lanes that are not written keep the old value
    prog.append(Ins(text, reads, [dst], kind=AB.DPP, sem=("dpp", dst, src, kind, bank, bound)))


def shl(prog, dst, src, k):
    dpp(prog, dst, src, "row_shl:%d" % k, kind=("shl", k))


def mirror(prog, reg):  # lanes 12 .. 15 <- lanes 0 .. 3
    dpp(prog, reg, reg, "row_shr:12", bank=0x8, bound=False, kind=("shr", 12))


def quad(prog, dst, src, sel):
    dpp(prog, dst, src, "quad_perm:[%d,%d,%d,%d]" % tuple(sel), kind=("quad", tuple(sel)))


def fold(prog, dst, acc_a, acc_b):
    AB.fold(prog, dst, acc_a, acc_b, FT, CV, FC)


def layer(prog, lo, hi, coef, seed_a, seed_b, reload_seeds):
    """ACC_A / ACC_B = seeds + sum_k coef[k] * (halves of element (e + k) mod 12); coef[k]: an inline constant or ('v', register of per-lane
    coefficients).  lo / hi are mirrored IN PLACE.  reload_seeds: the seeds' registers are loaded again (the next round's) once consumed."""
    r = ROT
    madc(prog, ACC_A, lo, coef[0], seed=seed_a)
    madc(prog, ACC_B, hi, coef[0], seed=seed_b)
    if reload_seeds:
        AB.load(prog, SEED_A, 4, ADDR, "%[off]", "next_seeds")
    mirror(prog, lo)
    mirror(prog, hi)
    base = (lo, hi)
    for group, copy in ((0, (ZC, ZC + 1)), (1, (WC, WC + 1)), (2, None)):
        ks = (1, 2, 3, 4) if group < 2 else (1, 2, 3)
        for k in ks:
            kk = 4 * group + k
            dl, dh = (copy if k == 4 else (r, r + 1))
            if k != 4:
                r += 2
            shl(prog, dl, base[0], k)
            shl(prog, dh, base[1], k)
            madc(prog, ACC_A, dl, coef[kk])
            madc(prog, ACC_B, dh, coef[kk])
        if copy is not None:
            mirror(prog, copy[0])
            mirror(prog, copy[1])
            base = copy


def layer_circulant(prog, lo, hi):
    layer(prog, lo, hi, [("v", C0)] + CIRC[1:], SEED_A, SEED_B, True)


def loads_landed(prog, regs):
    """the previous block's (or the caller's) load of these registers has landed"""
    prog.append(Ins("s_waitcnt lgkmcnt(0)", [], regs, kind=AB.WAIT))


def allreduce(prog, acc):
    """the row's sum of a 64-bit accumulator, in every lane"""
    for k in (8, 4, 2, 1):
        for h in (0, 1):
            dpp(prog, RT + h, acc + h, "row_ror:%d" % k, kind=("ror", k))
        add64(prog, acc, acc, RT)


def sbox_lane0(prog, s):
    """X7 = x^7 of the state word on lane 0: lane 1 forms x^4 while lane 0 forms x^3"""
    x = (S_LO, S_HI)
    mul(prog, X2, x, x, s)
    for h in (0, 1):
        quad(prog, X3 + h, X2 + h, (0, 0, 2, 3))          # lanes 0 and 1 read lane 0's x^2
        cndmask(prog, SEL + h, X3 + h, x[h], MASK0)        # lane 0: x, others: x^2
    mul(prog, X4, (X3, X3 + 1), (SEL, SEL + 1), s)         # lane 0: x^3, lane 1: x^4
    for h in (0, 1):
        quad(prog, YN + h, X4 + h, (1, 1, 2, 3))           # lane 0 reads lane 1
    mul(prog, X7, (X4, X4 + 1), (YN, YN + 1), s)           # lane 0: x^7


def broadcast_x7(prog):
    """BC = lane 0's X7 in lanes 0 .. 11 (X7's values in lanes 1 .. 3 are not x^7: take lane 0 explicitly)"""
    for h in (0, 1):
        quad(prog, BC + h, X7 + h, (0, 0, 0, 0))
        dpp(prog, BC + h, BC + h, "row_shr:4", bank=0x2, bound=False, kind=("shr", 4))
        dpp(prog, BC + h, BC + h, "row_shr:8", bank=0x4, bound=False, kind=("shr", 8))


def sbox_uniform(prog, dst, y, s):
    """dst = y^7 for a value every lane holds: even lanes form x^3, odd lanes x^4, each takes the other factor from its neighbour"""
    yy = (y, y + 1)
    mul(prog, X2, yy, yy, s)
    for h in (0, 1):
        cndmask(prog, SEL + h, X2 + h, y + h, MASKE)            # even lanes: y, odd lanes: y^2
    mul(prog, X4, (X2, X2 + 1), (SEL, SEL + 1), s)               # even: y^3, odd: y^4
    for h in (0, 1):
        quad(prog, YN + h, X4 + h, (1, 0, 3, 2))
    mul(prog, dst, (X4, X4 + 1), (YN, YN + 1), s)


def block_triple():
    """three partial rounds (poseidon_merged.h): in: the state with the first round's constants added; out: the state three rounds
    later with the following round's constants added"""
    prog = []
    loads_landed(prog, range(K1, K3 + 4))
    a, b = slot(0), slot(1)
    cndmask(prog, SZ, S_LO, None, MASK0)
    cndmask(prog, SZ + 1, S_HI, None, MASK0)
    # the parts of both dot products and of the dense layer that do not wait for x1
    madc(prog, D1A, SZ, ("v", R1), seed=K1)
    madc(prog, D1B, SZ + 1, ("v", R1), seed=K1 + 2)
    madc(prog, D2A, SZ, ("v", R2), seed=K2)
    madc(prog, D2B, SZ + 1, ("v", R2), seed=K2 + 2)
    layer(prog, SZ, SZ + 1, [("v", N3K + k) for k in range(12)], K3, K3 + 2, False)   # any 12 x 12 layer: N3, per-lane coefficients
    for j, K in enumerate((K1, K2, K3)):
        AB.load(prog, K, 4, ADDR, "%%[off%d]" % (j + 1), ("next_k", j))
    sbox_lane0(prog, a)                                    # x1 = u0^7 on lane 0
    # y1 = (M ut)[0] + k1
    madc(prog, D1A, X7, ("v", L0M))
    madc(prog, D1B, X7 + 1, ("v", L0M))
    allreduce(prog, D1A)
    allreduce(prog, D1B)
    fold(prog, YY, D1A, D1B)
    broadcast_x7(prog)                                     # x1 to every lane for the dense layer
    madc(prog, ACC_A, BC, ("v", N3C0))
    madc(prog, ACC_B, BC + 1, ("v", N3C0))
    # y2 = (N2 ut)[0] + M00 x2 + k2: everything but the x2 term is summed over the row while x2 is being computed
    madc(prog, D2A, X7, ("v", L0N))
    madc(prog, D2B, X7 + 1, ("v", L0N))
    allreduce(prog, D2A)
    allreduce(prog, D2B)
    sbox_uniform(prog, XS2, YY, b)
    madc(prog, D2A, XS2, 25)
    madc(prog, D2B, XS2 + 1, 25)
    fold(prog, YY, D2A, D2B)
    madc(prog, ACC_A, XS2, ("v", B2))
    madc(prog, ACC_B, XS2 + 1, ("v", B2))
    sbox_uniform(prog, XS3, YY, b)
    madc(prog, ACC_A, XS3, ("v", B3))
    madc(prog, ACC_B, XS3 + 1, ("v", B3))
    fold(prog, S_LO, ACC_A, ACC_B)
    return prog


def block_full():
    prog = []
    loads_landed(prog, SEEDS)
    a, b = slot(0), slot(1)
    x = (S_LO, S_HI)
    mul(prog, X2, x, x, a)
    mul(prog, X4, (X2, X2 + 1), (X2, X2 + 1), a)
    mul(prog, X3, (X2, X2 + 1), x, b)
    mul(prog, X7, (X3, X3 + 1), (X4, X4 + 1), a)
    layer_circulant(prog, X7, X7 + 1)
    fold(prog, S_LO, ACC_A, ACC_B)
    return prog


def block_partial():
    prog = []
    loads_landed(prog, SEEDS)
    # the layer over the state with lane 0 zeroed: independent of the S-box
    cndmask(prog, SZ, S_LO, None, MASK0)
    cndmask(prog, SZ + 1, S_HI, None, MASK0)
    layer_circulant(prog, SZ, SZ + 1)
    sbox_lane0(prog, slot(0))
    # x^7 of lane 0 to lanes 0 .. 11, times column 0 of the matrix
    broadcast_x7(prog)
    madc(prog, ACC_A, BC, ("v", COL0))
    madc(prog, ACC_B, BC + 1, ("v", COL0))
    fold(prog, S_LO, ACC_A, ACC_B)
    return prog


# ---------------------------------------------------------------- testers (one row of 16 lanes)
def row_words(values, pad):
    """twelve 64-bit values on lanes 0 .. 11 as (low dwords, high dwords); pad(): what lanes 12 .. 15 hold"""
    return [x & M32 for x in values] + [pad() for _ in range(4)], [x >> 32 for x in values] + [pad() for _ in range(4)]


def junk():
    return random.getrandbits(32)


def check_state(vregs, want, what):
    for e in range(12):
        assert (vregs[S_LO][e] | (vregs[S_HI][e] << 32)) % P == want[e], (what, e)


def random_round():
    return [AB.edge_value() for _ in range(12)], [random.getrandbits(64) % P for _ in range(12)]


def random_triple():
    return [AB.edge_value() for _ in range(12)], [[random.getrandbits(64) % P for _ in range(12)] for _ in range(3)]


def drawn(cases, draw, count):
    """the testers' inputs: `cases` where the caller brings its own round-entry states (tests/test_poseidon_steering_cpu.py), else
    `count` random draws"""
    return cases if cases is not None else (draw() for _ in range(count))


def test(order, partial, cases=None):
    for state, rc in drawn(cases, random_round, 100):
        vregs = {r: [junk() for _ in range(NL)] for r in range(176, 256)}
        vregs[S_LO], vregs[S_HI] = row_words(state, junk)
        vregs[SEED_A], vregs[SEED_B] = row_words(rc, int)
        vregs[SEED_A + 1] = vregs[SEED_B + 1] = vregs[ZA] = vregs[ZB] = [0] * NL
        vregs[C0] = [25] + [17] * 15
        vregs[COL0] = [25] + [CIRC[(12 - e) % 12] for e in range(1, 12)] + [0] * 4
        nxt = [[junk() for _ in range(NL)] for _ in range(4)]
        vregs["mem"] = {"next_seeds": nxt}
        AB.run(order, vregs, {MASK0: [1] + [0] * 15}, NL)
        assert [vregs[r] for r in SEEDS] == nxt
        check_state(vregs, AB.reference_round(state, rc, partial), partial)


def test_triple(order, cases=None):
    for state, cs in drawn(cases, random_triple, 60):
        (M, N2, N3), (k1, k2, k3) = AB.merged_tables(cs)
        assert max(max(r) for r in N3) < 1 << 21
        # reference: three plain partial rounds
        want = state
        for c in cs:
            want = AB.reference_round(want, c, True)
        vregs = {r: [junk() for _ in range(NL)] for r in range(120, 256)}
        vregs[S_LO], vregs[S_HI] = row_words(state, junk)
        for k in range(12):
            vregs[N3K + k] = [N3[e][(e + k) % 12] for e in range(12)] + [0] * 4
        for reg, column in ((R1, M[0]), (R2, N2[0]), (B2, [N2[e][0] for e in range(12)]), (B3, [M[e][0] for e in range(12)]), (N3C0, [N3[e][0] for e in range(12)])):
            vregs[reg] = column + [0] * 4
        vregs[L0M] = [M[0][0]] + [0] * 15
        vregs[L0N] = [N2[0][0]] + [0] * 15
        for K, val in ((K1, [k1] + [0] * 11), (K2, [k2] + [0] * 11), (K3, k3)):
            vregs[K], vregs[K + 2] = row_words(val, int)
            vregs[K + 1] = vregs[K + 3] = [0] * NL
        vregs[ZA] = vregs[ZB] = [0] * NL
        nxt = [[[junk() for _ in range(NL)] for _ in range(4)] for _ in range(3)]
        vregs["mem"] = {("next_k", j): nxt[j] for j in range(3)}
        AB.run(order, vregs, {MASK0: [1] + [0] * 15, MASKE: [1, 0] * 8}, NL)
        check_state(vregs, want, "triple")
        for j, K in enumerate((K1, K2, K3)):
            assert [vregs[K + q] for q in range(4)] == nxt[j]


def main():
    random.seed(11)
    print("// generated by tools/gen_row_round_asm.py -- do not edit.  Physical registers: state v[%d:%d] (in and out), seeds v[%d:%d] v[%d:%d]," %
          (S_LO, S_HI, SEED_A, SEED_A + 1, SEED_B, SEED_B + 1))
    print("// c0 v%d, column 0 v%d, zeros v%d v%d, lane-0 mask s[%d:%d]; v184 .. v255 and s%d .. s%d are clobbered." % (C0, COL0, ZA, ZB, MASK0, MASK0 + 1, SINK, FC + 1))
    inputs = {S_LO, S_HI} | set(SEEDS)
    for name, prog, written, tester, what in (
            ("FULL_ROUND", block_full(), inputs, lambda o: test(o, False), "full round: x^7 of every element, circulant layer, fold"),
            ("PARTIAL_ROUND", block_partial(), inputs, lambda o: test(o, True), "partial round: x^7 of element 0 under the layer of the other eleven, fold"),
            ("TRIPLE", block_triple(), inputs | set(range(K1, K3 + 4)), test_triple,
             "three partial rounds at once (poseidon_merged.h): three S-boxes, two dot products summed over the row, one dense layer")):
        order = AB.schedule(prog, HAZARDS)
        AB.check_hazards(order, HAZARDS, written)
        tester(order)
        AB.emit("STARKHIP_ROW_%s_ASM" % name, order, what)
    for name, operand in [(name, "{v[%d:%d]}" % (r, r + 3)) for name, r in (("N3K0", N3K), ("N3K1", N3K + 4), ("N3K2", N3K + 8), ("MISC0", R1), ("MISC1", N3C0))] + \
                         [(name, "+{v[%d:%d]}" % (r, r + 3)) for name, r in (("K1", K1), ("K2", K2), ("K3", K3))] + [("MASKE", "{%s}" % AB.sp(MASKE))]:
        AB.define("STARKHIP_ROW_" + name, operand)
    AB.clobbers("STARKHIP_ROW_TRIPLE_CLOBBERS", range(D1A, XS3 + 2))
    for name, operand in (("STATE_OUT", "={v[%d:%d]}" % (S_LO, S_HI)), ("STATE_LO", "{v%d}" % S_LO), ("STATE_HI", "{v%d}" % S_HI), ("SEED_A", "+{%s}" % AB.vp(SEED_A)),
                          ("SEED_B", "+{%s}" % AB.vp(SEED_B)), ("ADDR", "{v%d}" % ADDR), ("C0", "{v%d}" % C0), ("COL0", "{v%d}" % COL0), ("ZA", "{v%d}" % ZA), ("ZB", "{v%d}" % ZB),
                          ("MASK0", "{%s}" % AB.sp(MASK0))):
        AB.define("STARKHIP_ROW_" + name, operand)
    bound = {S_LO, S_HI, C0, COL0, ZA, ZB} | set(SEEDS)
    AB.clobbers("STARKHIP_ROW_CLOBBERS", [r for r in range(184, 256) if r not in bound], range(SINK, FC + 2))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generates csrc/lane_round_asm.inc: the rounds of the LANE form of the Poseidon permutation (one lane per leaf, the whole state in
the lane's registers; poseidon_dev.h) as scheduled inline-asm blocks on fixed physical registers.

The lane form costs the fewest instructions per permutation -- nothing is repeated across lanes: ~ 12.8 K slots against the quad
form's 4346 x 4 lane-slots -- but from C++ hipcc makes 14.4 K VALU + 4.7 K wait states + 335 s_waitcnt of it.  Here
the twelve independent S-boxes of a full round fill each other's flag hand-offs, round constants and the merged layers' coefficients
(uniform over the wave) come from one LDS image by broadcast loads issued a row ahead, and the waits are COUNTED (LDS returns in
order: s_waitcnt lgkmcnt(k) with k = the loads issued since the one needed).

The instruction model, the scheduler, the hazard checker, the interpreter and the multiply / multiply-add / fold sequences are
tools/asm_blocks.py, shared with the row and pair forms' generators; here are the lane form's register map, blocks, the MFMA as one lane
sees it and the testers.  tools/gen_pair_round_asm.py builds its blocks from this file's pieces (S-box, byte permutes, MFMA, folds).

    python tools/gen_lane_round_asm.py > starky_bls12_381_amd/csrc/lane_round_asm.inc
"""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import asm_blocks as AB  # noqa: E402
from asm_blocks import CIRC, M32, P, SINK, Ins, load, madc, mds_coef, mul, v, vp  # noqa: E402

# issue slots (asm_blocks.Hazards says what each distance is); load_latency is what the scheduler aims for, the counted waits keep a shorter
# distance correct.  The pair form's generator schedules with a copy of this table that its experiment knobs change, and checks against this one.
HAZARDS = AB.Hazards(valu_raw=1, sgpr_raw=3, dpp_read=3, war=2, war_load=1, load_latency=16, mfma_result=20, mfma_spacing=9, mfma_operand=3, mfma_war=6)

# ---------------------------------------------------------------- register map (VGPRs 76 .. 255)
A_K3, A_K12, A_COEF, A_SEED = 76, 77, 78, 79   # in: LDS addresses (k3[t], k12[t], coefficient rows, rc[r + 1])
T = 80            # state: 12 pairs v[80:103] (in and out)
S = 104           # S-box outputs / u': 12 pairs
SEEDR = 128       # seed ring: 4 x (lo64, hi64) = 16 registers
COEFR = 144       # coefficient ring: 2 rows x 16
O = 176           # dense layer outputs: 12 pairs
ACC = 200         # two outputs in flight: (A, B) pairs each
FOLD = 208        # two folds in flight: FT pair + CV each (208:209, 210 / 212:213, 214)
XT = 216          # S-box temporaries: 2 sets x (x2, x3, x4) pairs
SLOTS = [228, 236]
AD = [244, 246]   # addend pairs (ad, zero): 245 and 247 hold zero (inputs)
YY = 248          # folded dot products, x2, x3 (pairs 248, 250, 252)
FLAGS, FCS = [44, 52], [60, 62]


def slot(k):
    return AB.Slot(SLOTS[k], AD[k], FLAGS[k])


def fold_to(prog, dst, A, B, k, base=FOLD):
    """v[dst:dst+1] = A + B * 2^32 mod p with fold temporaries set k"""
    AB.fold(prog, dst, A, B, base + 4 * k, base + 4 * k + 2, FCS[k])


def sbox(prog, dst, x, k):
    """dst = x^7; temporaries set k, both multiply slots (x^3 and x^4 side by side)"""
    a, b = slot(0), slot(1)
    x2, x3, x4 = XT + 6 * k, XT + 6 * k + 2, XT + 6 * k + 4
    xx = (x, x + 1)
    mul(prog, x2, xx, xx, a if k == 0 else b)
    mul(prog, x4, (x2, x2 + 1), (x2, x2 + 1), a)
    mul(prog, x3, (x2, x2 + 1), xx, b)
    mul(prog, dst, (x3, x3 + 1), (x4, x4 + 1), a if k == 0 else b)


def circulant(prog, first_out, in_base, out_base):
    """out[r] = seed[r] + sum_i CIRC[i] in[(i + r) % 12] (+ 8 in[0] for r = 0), r = first_out .. 11; seeds from LDS at A_SEED"""
    for r in range(first_out, 12):
        sd = SEEDR + 4 * (r % 4)
        load(prog, sd, 4, A_SEED, 16 * r, ("seed", r))
        A, B = ACC + 4 * (r % 2), ACC + 4 * (r % 2) + 2
        for i in range(12):
            j = (i + r) % 12
            k = CIRC[i] + (8 if r == 0 and i == 0 else 0)
            madc(prog, A, in_base + 2 * j, k, seed=sd if i == 0 else None)
            madc(prog, B, in_base + 2 * j + 1, k, seed=sd + 2 if i == 0 else None)
        fold_to(prog, out_base + 2 * r, A, B, r % 2)


def block_full(first_out=0):
    prog = []
    for e in range(12):
        sbox(prog, S + 2 * e, T + 2 * e, e % 2)
    circulant(prog, first_out, S, T)
    return prog


def outputs_to_state(prog, n):
    for e in range(n):
        AB.mov64(prog, T + 2 * e, O + 2 * e)


def block_partial():
    prog = []
    sbox(prog, T, T, 0)     # element 0 in place
    # the layer reads T and must not overwrite it while later outputs still need it: outputs go to O, then back
    circulant(prog, 0, T, O)
    outputs_to_state(prog, 12)
    return prog


def dot(prog, A, B, coef_off, seed_regs, key):
    """A / B = seed + sum_j coef[j] * halves of T[j]; coefficient row (12 words) from LDS at A_COEF + coef_off"""
    cr = COEFR + 16 * (key[1] % 2)
    for q in range(3):
        load(prog, cr + 4 * q, 4, A_COEF, coef_off + 16 * q, (key, q))
    if key[0] == "row":
        load(prog, cr + 12, 4, A_COEF, coef_off + 48, (key, 3))
    for j in range(12):
        madc(prog, A, T + 2 * j, ("v", cr + j), seed=seed_regs if j == 0 else None)
        madc(prog, B, T + 2 * j + 1, ("v", cr + j), seed=seed_regs + 2 if j == 0 else None)
    return cr


ROW_OFF, M0_OFF, N20_OFF = 0, 12 * 64, 12 * 64 + 48   # LaneTables: row[12][16], m0[12], n20[12] contiguous


# ---------------------------------------------------------------- FOUR partial rounds at once
# With M the MDS matrix, Mz = M with row 0 zeroed, N_k = M Mz^(k-1), u the state at the start of partial round r (constants added),
# x1 = u0^7, ut = (x1, u1 .. u11), c1 .. c4 the constants of rounds r + 1 .. r + 4 (c?z: element 0 zeroed):
#     y1  = (M ut)[0] + k1                                          x2 = y1^7      k1 = c1[0]
#     y2  = (N2 ut)[0] + M[0][0] x2 + k2                             x3 = y2^7      k2 = (M c1z)[0] + c2[0]
#     y3  = (N3 ut)[0] + N2[0][0] x2 + M[0][0] x3 + k3               x4 = y3^7      k3 = (N2 c1z)[0] + (M c2z)[0] + c3[0]
#     out = N4 ut + N3[:,0] x2 + N2[:,0] x3 + M[:,0] x4 + k4                        k4 = N3 c1z + N2 c2z + M c3z + c4
# N4's entries are below 2^29 and a row of it, with its three x-coefficients, sums to less than 0.83 * 2^32: the two accumulators of
# an output (products with the 32-bit halves of the inputs) stay below 2^64 -- but no longer below 2^57, so their fold takes the
# multiply-add's carry (fold_big).  Five merges would need 37-bit coefficients.  Per round 825 / 4 slots against 732 / 3.
FC2 = [72, 74]    # scalar pairs: carry out of fold_big's first multiply-add
N30_OFF = N20_OFF + 48     # LaneTables: n30[16] = row 0 of N3, then N2[0][0]
KQ = S                     # the third scalar seed's registers (the S-box output area is idle in this block): v[104:107]


def four_tables(cs):
    """AB.merged_tables for four rounds, with what fold_big needs of them: B < 2^64 - 2^32 (B_hi + carry must not wrap)"""
    (M, N2, N3, N4), ks = AB.merged_tables(cs)
    for g in range(12):
        assert (sum(N4[g]) + N3[g][0] + N2[g][0] + M[g][0]) * M32 + M32 < (1 << 64) - (1 << 32)
    return (M, N2, N3, N4), ks


def fold_big(prog, dst, A, B, k):
    AB.fold_big(prog, dst, A, B, FOLD + 4 * k, FOLD + 4 * k + 2, FCS[k], FC2[k])


def block_four():
    prog = []
    sbox(prog, T, T, 0)                                       # x1 replaces element 0: T is ut
    load(prog, SEEDR, 4, A_K12, 0, ("kf", 0))
    load(prog, SEEDR + 4, 4, A_K12, 16, ("kf", 1))
    load(prog, KQ, 4, A_K12, 32, ("kf", 2))
    dot(prog, ACC, ACC + 2, M0_OFF, SEEDR, ("dot", 0))
    fold_to(prog, YY, ACC, ACC + 2, 0)
    sbox(prog, YY + 2, YY, 1)                                  # x2
    dot(prog, ACC + 4, ACC + 6, N20_OFF, SEEDR + 4, ("dot", 1))
    madc(prog, ACC + 4, YY + 2, 25)                            # M[0][0] x2
    madc(prog, ACC + 6, YY + 3, 25)
    fold_to(prog, YY, ACC + 4, ACC + 6, 1)
    sbox(prog, YY + 4, YY, 0)                                  # x3
    cr = dot(prog, ACC, ACC + 2, N30_OFF, KQ, ("dot", 2))
    load(prog, cr + 12, 1, A_COEF, N30_OFF + 48, (("dot", 2), 3))
    madc(prog, ACC, YY + 2, ("v", cr + 12))                    # N2[0][0] x2
    madc(prog, ACC + 2, YY + 3, ("v", cr + 12))
    madc(prog, ACC, YY + 4, 25)                                # M[0][0] x3
    madc(prog, ACC + 2, YY + 5, 25)
    fold_to(prog, YY, ACC, ACC + 2, 0)
    sbox(prog, YY + 6, YY, 1)                                  # x4
    for r in range(12):
        sd = SEEDR + 8 + 4 * (r % 2)
        load(prog, sd, 4, A_K3, 16 * r, ("k4", r))
        A, B = ACC + 4 * (r % 2), ACC + 4 * (r % 2) + 2
        cr = dot(prog, A, B, ROW_OFF + 64 * r, sd, ("row", r))
        for q in range(3):                                     # N3[r][0] x2 + N2[r][0] x3 + M[r][0] x4
            madc(prog, A, YY + 2 + 2 * q, ("v", cr + 12 + q))
            madc(prog, B, YY + 3 + 2 * q, ("v", cr + 12 + q))
        fold_big(prog, O + 2 * r, A, B, r % 2)
    outputs_to_state(prog, 12)
    return prog


# ---------------------------------------------------------------- the circulant layer on the matrix pipe
# One permutation per lane: the layer  out[i] = rc[i] + sum_j M[i][j] s[j]  over all 64 lanes IS a (12 x 12) x (12 x 64) product of a
# matrix of 6-bit weights with 64-bit words, i.e. eight products with the words' BYTE PLANES (bytes are exact in the i8 pipe, the
# 12-term sums stay below 2^17): v_mfma_i32_32x32x32_i8 with the weights as the A tile and byte plane b of the state as the B tile.
# Lane l of the B operand holds 16 K-values of column l & 31; lanes l and l + 32 are two different permutations here, so the weight
# tile is block diagonal: rows whose results land in the lower lane half (rows 0-3, 8-11, 16-19 = output g = (row & 3) + 4 (row >> 3))
# carry M[g][.] against the lower half's K-values and zeros against the upper half's, rows 4-7, 12-15, 20-23 the other way round
# (tools/experiments/mfma_mds_probe.hip checks this map with exact integer data on all 64 lanes).  Result register g of a lane is then
#   S_b[g] = sum_j M[g][j] sbyte_b(s[j]) + (what the four spare K-values add),
# sbyte = byte XOR 0x80 read as signed = byte - 128 (the pipe's operands are signed).  The spare K-values 12 .. 15 carry the constants:
# the B side holds (1, 64, 127, 127) in every lane, the A side -- per row, round and plane, one dword per lane from LDS -- holds
# (c7, 2 m + 40, 127, 127) with c7 + 128 m = byte b of a 64-bit constant RC[g]: together + RC byte + 34 818, which makes every S_b[g]
# non-negative (34 818 >= 128 * 272, the largest row sum) and lets the host fold the offsets into RC (poseidon_tables.cpp).
# Recombination: lo = S0 + S1 2^8 + S2 2^16 + S3 2^24 (two v_lshl_add_u32 and one multiply-add by 2^16), hi likewise from planes 4 .. 7,
# then the fold lo + hi 2^32 the multiply-add form already uses.  Per round 24 XORs + 48 byte permutes + 8 LDS dwords + 8 MFMA (which
# cost the vector issue < 1 slot each, measured by the probe) + 72 + 48 instead of 288 multiply-adds + 48 + 12 LDS rows.
AW = [52, 56]            # in: the weight tile's dwords 0 .. 2, twice (v52-54, v56-58); dword 3 (v55, v59) is loaded per plane
BP = [60, 64, 68, 72]    # the B tuples of planes b mod 4; dwords 0 .. 2 are written here, dword 3 (v63, v67, v71, v75) in: 0x7F7F4001
A_RCB = 79               # in: LDS address of this lane's dword in the round's constant table (plane b at byte offset 256 b)
DT = [128 + 12 * b for b in range(8)]   # result tiles, one per plane: sixteen registers are written, the first twelve are results; the four
                         # junk registers are the next tile's first four, which the next MFMA (issued later, one pipe: it completes later)
                         # overwrites with its results.  v128 .. v227
HIP = S                  # hi halves (12 pairs): the S-box outputs' registers in a full round (every permute has read them by then)
ST = 248                 # byte-transpose temporaries (8)
UT = [228, 229, 230, 231]     # 32-bit partial sums
MFOLD = 232              # the folds' temporaries here (the usual ones lie under the tiles): 232 .. 238
S_SEL = {"A": 64, "B": 65, "C": 66, "D": 67}   # SGPRs in: v_perm_b32 selectors
S_X80, S_64K = 68, 69    # SGPRs in: 0x80808080, 65536
SEL_VALUE = {"A": 0x05010400, "B": 0x07030602, "C": 0x05040100, "D": 0x07060302}
B_CONST = 0x7F7F4001
K_OFFSET = 2 * 127 * 127 + 64 * 40


def perm(prog, dst, s0, s1, sel):
    prog.append(Ins("v_perm_b32 %s, %s, %s, s%d" % (v(dst), v(s0), v(s1), S_SEL[sel]), [s0, s1], [dst], sem=("perm", dst, s0, s1, SEL_VALUE[sel])))


def xor80(prog, reg):
    prog.append(Ins("v_xor_b32 %s, s%d, %s" % (v(reg), S_X80, v(reg)), [reg], [reg], sem=("xor80", reg)))


def lshl_add(prog, dst, a, sh, b):
    prog.append(Ins("v_lshl_add_u32 %s, %s, %d, %s" % (v(dst), v(a), sh, v(b)), [a, b], [dst], sem=("lshladd", dst, a, sh, b)))


def mfma(prog, a, b, d, index, sem="mfma"):
    """tile d = weight tuple a x B tuple b; the weights' constant dword (a + 3) is entry `index` of the round's table at A_RCB"""
    load(prog, a + 3, 1, A_RCB, 256 * index, ("rcb", index))
    # (the junk registers d + 12 .. d + 15 are not listed as written: nothing reads them, and the MFMA that owns them is ordered behind
    # this one through the pipe's pseudo register)
    prog.append(Ins("v_mfma_i32_32x32x32_i8 v[%d:%d], v[%d:%d], v[%d:%d], 0" % (d, d + 15, a, a + 3, b, b + 3),
                    [a, a + 1, a + 2, a + 3, b, b + 1, b + 2, b + 3, AB.MFMA_PIPE], list(range(d, d + 12)) + [AB.MFMA_PIPE], kind=AB.MFMA,
                    sem=(sem, d, a, b, index), junk=range(d + 12, d + 16)))


def recombine(prog, dst, lo, lo8, hi, hi8, i, u):
    """dst (pair) = lo + lo8 2^8 + (hi + hi8 2^8) 2^16: four tiles' registers of one output to a 64-bit sum"""
    ad = AD[i % 2]
    lshl_add(prog, ad, lo8, 8, lo)
    lshl_add(prog, u, hi8, 8, hi)
    prog.append(Ins("v_mad_u64_u32 %s, %s, %s, s%d, %s" % (vp(dst), AB.sp(SINK), v(u), S_64K, vp(ad)), [u, ad, ad + 1], [dst, dst + 1],
                    sem=("mad", dst, None, u, ("const", 65536), ad)))


def circulant_mfma(prog, in_base, out_base):
    """out[i] = RC[i] + sum_j M[i][j] in[j] for all twelve outputs; RC comes in through the table at A_RCB.  The low dwords of the inputs
    make planes 0 .. 3, the high dwords planes 4 .. 7.  All eight products are issued before anything is recombined (a tile per plane),
    so the wait for the last one is filled with the recombination of the first ones; the low halves of the results go to `out_base`,
    the high halves to HIP, both only after every input has been read (in_base may be out_base or HIP)."""
    for half in range(2):
        for q in range(3):
            w = [in_base + 2 * (4 * q + k) + half for k in range(4)]
            t = ST + 4 * (q % 2)
            perm(prog, t + 0, w[1], w[0], "A")   # (w0.b0, w1.b0, w0.b1, w1.b1)
            perm(prog, t + 1, w[1], w[0], "B")   # (w0.b2, w1.b2, w0.b3, w1.b3)
            perm(prog, t + 2, w[3], w[2], "A")
            perm(prog, t + 3, w[3], w[2], "B")
            perm(prog, BP[0] + q, t + 2, t + 0, "C")   # byte 0 of w0 .. w3
            perm(prog, BP[1] + q, t + 2, t + 0, "D")   # byte 1
            perm(prog, BP[2] + q, t + 3, t + 1, "C")   # byte 2
            perm(prog, BP[3] + q, t + 3, t + 1, "D")   # byte 3
            for k in range(4):
                xor80(prog, BP[k] + q)
        for k in range(4):
            mfma(prog, AW[k % 2], BP[k], DT[4 * half + k], 4 * half + k)
    for half in range(2):
        for i in range(12):
            d0, d1, d2, d3 = (DT[4 * half + k] + i for k in range(4))
            recombine(prog, (out_base if half == 0 else HIP) + 2 * i, d0, d1, d2, d3, i, UT[(2 * half + i) % 4])
    for i in range(12):
        fold_to(prog, out_base + 2 * i, out_base + 2 * i, HIP + 2 * i, i % 2, MFOLD)


def block_full_mfma():
    prog = []
    for e in range(12):
        sbox(prog, S + 2 * e, T + 2 * e, e % 2)
    circulant_mfma(prog, S, T)
    return prog


def block_partial_mfma():
    prog = []
    sbox(prog, T, T, 0)       # element 0 in place; the layer reads T and writes T (every input is in the B tuples before any output exists)
    circulant_mfma(prog, T, T)
    return prog


def schedule(prog, hazards=HAZARDS):
    # a consumer of a loaded register is kept load_latency slots behind the load (there is other work); then the waits are counted
    return AB.count_waits(AB.schedule(prog, hazards), hazards.load_latency)


# ---------------------------------------------------------------- the MFMA for the interpreter
def mfma_results(by, plane_bytes, g):
    """what the pipe adds up for output g: the twelve signed bytes `by` against row g of the weights, and the constants' four K-values"""
    val = sum(mds_coef(g, j) * by[j] for j in range(12)) + (plane_bytes[g] & 0x7F) + 64 * (2 * (plane_bytes[g] >> 7) + 40) + 2 * 127 * 127
    assert 0 <= val < (1 << 17)
    return val


def signed_byte(x, i):
    x = (x >> (8 * i)) & 0xFF
    return x - 256 if x >= 128 else x


def sem_mfma(m, ins, d, a, b, plane):
    """the MFMA as ONE LANE sees it (its own twelve K-values against the weight rows that land in it; the cross-lane map itself is
    checked on the device, tools/experiments/mfma_mds_probe.hip)"""
    assert m.V(b + 3) == [B_CONST], "B tuple's constant dword"
    assert m.V(a + 3) == [0xC0DE00 + plane], ("A tuple holds another plane's constants", plane, m.V(a + 3))
    by = [signed_byte(m.V(b + q)[0], i) for q in range(3) for i in range(4)]
    for g in range(12):
        m.vregs[d + g] = [mfma_results(by, m.vregs["rcbytes"][plane], g)]
    for g in range(12, 16):  # the junk rows: anything
        m.vregs[d + g] = [0xDEAD0000 + g]


SEMS = {"mfma": sem_mfma}


# ---------------------------------------------------------------- testers (lanes = 1 here; the pair form's generator passes 2: lane l
# holds elements 12 / lanes * l ..)
def mfma_round_constants(rc):
    """the 64-bit constants whose bytes ride in the weight tile: RC[g] = rc[g] - (K - 128 rowsum[g]) * 0x0101010101010101 mod p"""
    ones = 0x0101010101010101
    return [(rc[g] - (K_OFFSET - 128 * sum(mds_coef(g, j) for j in range(12))) * ones) % P for g in range(12)]


def fresh(lanes=1):
    vregs = {r: [random.getrandbits(32) for _ in range(lanes)] for r in range(52, 256)}
    vregs[AD[0] + 1] = vregs[AD[1] + 1] = [0] * lanes
    for k in range(4):
        vregs[BP[k] + 3] = [B_CONST] * lanes
    vregs["mem"] = {}
    return vregs


def set_state(vregs, state, lanes=1):
    ne = 12 // lanes
    for e in range(ne):
        vregs[T + 2 * e] = [state[ne * l + e] & M32 for l in range(lanes)]
        vregs[T + 2 * e + 1] = [state[ne * l + e] >> 32 for l in range(lanes)]


def get_state(vregs, lanes=1):
    ne = 12 // lanes
    return [(vregs[T + 2 * e][l] | (vregs[T + 2 * e + 1][l] << 32)) % P for l in range(lanes) for e in range(ne)]


def pair4(*c):
    """a 64-bit constant per lane as two 64-bit addends (low half, 0, high half, 0)"""
    return [[x & M32 for x in c], [0] * len(c), [x >> 32 for x in c], [0] * len(c)]


def random_round():
    return [AB.edge_value() for _ in range(12)], [random.getrandbits(64) % P for _ in range(12)]


def drawn(cases, draw, count):
    """the testers' inputs: `cases` where the caller brings its own round-entry states (tests/test_poseidon_steering_cpu.py), else
    `count` random draws"""
    return cases if cases is not None else (draw() for _ in range(count))


def test_round(order, partial, first_out=0, cases=None):
    for state, rc in drawn(cases, random_round, 40):
        vregs = fresh()
        set_state(vregs, state)
        for r in range(12):
            vregs["mem"][("seed", r)] = pair4(rc[r])
        AB.run(order, vregs, {}, 1)
        assert get_state(vregs)[first_out:] == AB.reference_round(state, rc, partial)[first_out:], partial


def test_round_mfma(order, partial, lanes=1, sems=SEMS, sregs={}, first_out=0, cases=None):
    for state, rc in drawn(cases, random_round, 40):
        vregs = fresh(lanes)
        set_state(vregs, state, lanes)
        RC = mfma_round_constants(rc)
        vregs["rcbytes"] = [[(RC[g] >> (8 * b)) & 0xFF for g in range(12)] for b in range(8)]
        for b in range(8):
            vregs["mem"][("rcb", b)] = [[0xC0DE00 + b] * lanes]
        AB.run(order, vregs, dict(sregs), lanes, sems)
        got, want = get_state(vregs, lanes), AB.reference_round(state, rc, partial)
        for g in range(12):
            assert g % (12 // lanes) < first_out or got[g] == want[g], (partial, g)


def random_four():
    """state, the four rounds' constants"""
    state = [AB.edge_value() for _ in range(12)]
    cs = [[random.getrandbits(64) % P for _ in range(12)] for _ in range(4)]
    return state, cs


def four_later(state, cs):
    """the state len(cs) partial rounds later"""
    want = state
    for c in cs:
        want = AB.reference_round(want, c, True)
    return want


def test_four(order, cases=None):
    for state, cs in drawn(cases, random_four, 30):
        want = four_later(state, cs)
        (M, N2, N3, N4), (k1, k2, k3, k4) = four_tables(cs)
        vregs = fresh()
        set_state(vregs, state)
        mem = vregs["mem"]
        mem[("kf", 0)], mem[("kf", 1)], mem[("kf", 2)] = pair4(k1), pair4(k2), pair4(k3)
        for r in range(12):
            mem[("k4", r)] = pair4(k4[r])
            row = [N4[r][j] for j in range(12)] + [N3[r][0], N2[r][0], M[r][0], 0]
            for q in range(4):
                mem[(("row", r), q)] = [[x] for x in row[4 * q:4 * q + 4]]
        for q in range(3):
            mem[(("dot", 0), q)] = [[M[0][j]] for j in range(4 * q, 4 * q + 4)]
            mem[(("dot", 1), q)] = [[N2[0][j]] for j in range(4 * q, 4 * q + 4)]
            mem[(("dot", 2), q)] = [[N3[0][j]] for j in range(4 * q, 4 * q + 4)]
        mem[(("dot", 2), 3)] = [[N2[0][0]]]
        AB.run(order, vregs, {}, 1)
        assert get_state(vregs) == want


def main():
    random.seed(5)
    print("// generated by tools/gen_lane_round_asm.py -- do not edit.  Physical registers: state v[%d:%d] (in and out), LDS addresses v%d (k3) v%d (k12)" %
          (T, T + 23, A_K3, A_K12))
    print("// v%d (coefficient rows) v%d (next round's constants), zeros v%d v%d; v%d .. v255 and s%d .. s%d are clobbered." %
          (A_COEF, A_SEED, AD[0] + 1, AD[1] + 1, S, SINK, FCS[1] + 1))
    for name, prog, tester, what in (
            ("STARKHIP_LANE_FULL_ROUND_ASM", block_full(), lambda o: test_round(o, False), "full round: twelve S-boxes, circulant layer"),
            ("STARKHIP_LANE_LAST_ROUND_ASM", block_full(8), lambda o: test_round(o, False, 8), "last full round before an absorb: the capacity outputs only"),
            ("STARKHIP_LANE_PARTIAL_ROUND_ASM", block_partial(), lambda o: test_round(o, True), "partial round"),
            ("STARKHIP_LANE_FOUR_ASM", block_four(), test_four, "four partial rounds at once"),
            ("STARKHIP_LANE_FULL_ROUND_MFMA_ASM", block_full_mfma(), lambda o: test_round_mfma(o, False), "full round, circulant layer on the matrix pipe"),
            ("STARKHIP_LANE_PARTIAL_ROUND_MFMA_ASM", block_partial_mfma(), lambda o: test_round_mfma(o, True), "partial round, circulant layer on the matrix pipe")):
        order = schedule(prog)
        AB.check_hazards(order, HAZARDS)
        tester(order)
        AB.emit(name, order, what, loads=True)
    for i in range(3):
        AB.define("STARKHIP_LANE_STATE%d" % i, "+{v[%d:%d]}" % (T + 8 * i, T + 8 * i + 7))
    for name, reg in (("A_K3", A_K3), ("A_K12", A_K12), ("A_COEF", A_COEF), ("A_SEED", A_SEED), ("ZA", AD[0] + 1), ("ZB", AD[1] + 1)):
        AB.define("STARKHIP_LANE_" + name, "{v%d}" % reg)
    bound = set(range(T, T + 24)) | {AD[0] + 1, AD[1] + 1}
    AB.clobbers("STARKHIP_LANE_CLOBBERS", [r for r in range(S, 256) if r not in bound], list(range(SINK, FCS[1] + 2)) + list(range(FC2[0], FC2[1] + 2)))
    # the matrix-pipe blocks: weight tiles (dword 3 of each is loaded inside: in / out), the B tuples' constant dwords, the constant
    # table's address, the selectors and constants in scalar registers; the B tuples' other dwords are clobbered on top of the rest
    tile_operands("STARKHIP_LANE_")
    AB.define("STARKHIP_LANE_A_RCB", "{v%d}" % A_RCB)
    scalar_operands("STARKHIP_LANE_", "ABCD")
    for name, val in sorted(SEL_VALUE.items()):
        print("#define STARKHIP_LANE_SEL_%s_VALUE 0x%08xu" % (name, val))
    print("#define STARKHIP_LANE_B_CONST 0x%08xu" % B_CONST)
    print("#define STARKHIP_LANE_K_OFFSET %du" % K_OFFSET)
    AB.clobbers("STARKHIP_LANE_MFMA_CLOBBERS", [BP[k] + d for k in range(4) for d in range(3)])


def tile_operands(prefix):
    for k in range(2):
        for d in range(3):
            AB.define("%sAW%d%d" % (prefix, k, d), "{v%d}" % (AW[k] + d))
        AB.define("%sAW%d3" % (prefix, k), "+{v%d}" % (AW[k] + 3))
    for k in range(4):
        AB.define("%sBC%d" % (prefix, k), "{v%d}" % (BP[k] + 3))


def scalar_operands(prefix, selectors):
    for name, reg in [("SEL_" + s, S_SEL[s]) for s in selectors] + [("X80", S_X80), ("K64K", S_64K)]:
        AB.define("%sS_%s" % (prefix, name), "{s%d}" % reg)


if __name__ == "__main__":
    main()

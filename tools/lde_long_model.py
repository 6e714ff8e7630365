#!/usr/bin/env python3
"""Executable specification of the multi-workgroup transforms of csrc/kernels_lde_long.hip (2^14 .. 2^26 points).

A column of n = 2^log_n words is split n = A * B, A = 2^a, B = 2^b, a = log_n // 2, b = log_n - a (both 7 .. 13).  A tile is W words
wide: 16 for sub-transforms of up to 2^10 points (every length up to 2^20: every trace column), 8, 4, 2 for 2^11, 2^12, 2^13 points
(the other vectors of a proof of a long trace).  Below W = 16; with a narrower tile 16 becomes W and tid % 16, tid // 16 become
tid % W, tid // W.

    X[k1 + A k0] = sum_j0 w_B^(j0 k0) * ( w_n^(j0 k1) * sum_j1 w_A^(j1 k1) x[j1 B + j0] )

  pass 1: workgroup (tile t) owns j0 in [16 t, 16 t + 16); thread (q, w), w = tid % 16, q = tid // 16 < A / 16, holds the points
          p = q + i A/16 (i < 16) of the A-point transform of j0 = 16 t + w: word x[p B + j0], times the pre-scale.  Result k1 = q + i A/16
          goes out transposed to Y'[j0 A + k1].
  pass 2: workgroup (tile t) owns k1 in [16 t, 16 t + 16); thread (q, w) holds p = j0 = q + i B/16 of k1 = 16 t + w: word Y'[p A + k1]
          times the inter-pass twiddle tw[p A + k1] = w_n^(p k1).  Result k0 = q + i B/16 goes to X[k0 A + k1], times the post-scale.

Inside a workgroup the sixteen M-point transforms are Stockham passes of radix 16 (and one of radix 2, 4 or 8), exchanged through
the LDS image [point][16]; pass 1's transposed write-out goes through a second image [16][M + 1].

The model runs every workgroup with these index maps and tables (numpy over the threads of a workgroup), compares the result with a
plain radix-2 NTT -- itself checked against direct sums in Python integers --, checks every LDS address against the allocation and
counts bank conflicts by the rules of the gfx950 LDS: ds_read_b64 in two groups of 32 lanes over 64 banks of 4 bytes, ds_write_b64 in
four groups of 16 lanes over 32 banks.

  python tools/lde_long_model.py            # every log_n in 14 .. 20 at rate_bits 1, then one forward transform of 2^21 words
"""
import random
import sys

import numpy as np

P = 0xFFFFFFFF00000001
GEN = 7
U = np.uint64
M32 = U(0xFFFFFFFF)
EPS = U(0xFFFFFFFF)
PP = U(P)


def root_of_unity(bits):
    return pow(GEN, (P - 1) >> bits, P)


# ---------------------------------------------------------------- Goldilocks arithmetic on uint64 arrays (canonical in, canonical out)
def canon(x):
    return np.where(x >= PP, x - PP, x)


def add(a, b):
    s = a + b
    s = np.where(s < a, s + EPS, s)  # wrapped: 2^64 = 2^32 - 1
    return canon(s)


def sub(a, b):
    return np.where(a >= b, a - b, a + (PP - b))


def mul(a, b):
    a = np.asarray(a, dtype=U)
    b = np.asarray(b, dtype=U)
    a0, a1, b0, b1 = a & M32, a >> U(32), b & M32, b >> U(32)
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid_lo = (p01 & M32) + (p10 & M32) + (p00 >> U(32))
    mid_hi = (p01 >> U(32)) + (p10 >> U(32)) + (mid_lo >> U(32)) + (p11 & M32)
    l0, l1, l2, l3 = p00 & M32, mid_lo & M32, mid_hi & M32, (p11 >> U(32)) + (mid_hi >> U(32))
    r = sub(canon((l1 << U(32)) | l0), l3)  # 2^96 = -1
    return add(r, l2 * EPS)                 # 2^64 = 2^32 - 1


def powers(base, count):
    """base^0 .. base^(count - 1)"""
    out = np.ones(count, dtype=U)
    have = 1
    while have < count:
        step = U(pow(base, have, P))
        m = min(have, count - have)
        out[have:have + m] = mul(out[:m], step)
        have += m
    return out


def plain_ntt(x, root):
    """radix-2 decimation in time over the last axis; natural in, natural out"""
    n = x.shape[-1]
    bits = n.bit_length() - 1
    idx = np.arange(n)
    rev = np.zeros(n, dtype=np.int64)
    for b in range(bits):
        rev |= ((idx >> b) & 1) << (bits - 1 - b)
    a = x[..., rev].copy()
    tw = powers(root, n // 2)
    for st in range(bits):
        half = 1 << st
        a = a.reshape(x.shape[:-1] + (n >> (st + 1), 2, half))
        w = tw[:: n >> (st + 1)][:half]
        u, v = a[..., 0, :], mul(a[..., 1, :], w)
        a = np.stack([add(u, v), sub(u, v)], axis=-2)
    return a.reshape(x.shape)


def direct_sum(x, root, k):
    """X[k] in Python integers"""
    wk = pow(root, k, P)
    acc, cur = 0, 1
    for v in x.tolist():
        acc = (acc + v * cur) % P
        cur = cur * wk % P
    return acc


# ---------------------------------------------------------------- the plan of one M-point transform (LdePlan<LOGM>, csrc/lde_radix.h)
class Plan:
    def __init__(self, logm):
        self.logm, self.M, self.T = logm, 1 << logm, (1 << logm) // 16
        full, tail = logm // 4, logm % 4
        self.radix = [16] * full + ([1 << tail] if tail else [])
        self.ns = [1]
        for r in self.radix[:-1]:
            self.ns.append(self.ns[-1] * r)

    def twiddles(self, p, inverse):
        """[i][j mod Ns] = w_(Ns R)^(+-i j), the inverse's last pass times M^-1 (fill_tw)"""
        R, NS = self.radix[p], self.ns[p]
        w = root_of_unity((NS * R).bit_length() - 1)
        if inverse:
            w = pow(w, P - 2, P)
        scale = pow(self.M, P - 2, P) if inverse and p == len(self.radix) - 1 else 1
        return np.stack([mul(powers(pow(w, i, P), NS), U(scale)) for i in range(R)])


def split(log_n):
    a = log_n // 2
    return a, log_n - a


def tile_width(logm):
    """words of a tile row: one 128-byte line while M * W <= 2^14 words of LDS allow it"""
    return 16 if logm <= 10 else 1 << (14 - logm)


class Lds:
    """addresses in 8-byte words; every access is recorded for the bounds and bank checks"""

    def __init__(self, words):
        self.mem = np.zeros(words, dtype=U)
        self.words, self.out_of_bounds, self.read_conflicts, self.write_conflicts, self.accesses = words, 0, 0, 0, 0

    def _note(self, addr, write):
        self.accesses += 1
        self.out_of_bounds += int(((addr < 0) | (addr >= self.words)).sum())
        flat = addr.reshape(-1)
        group, banks = (16, 32) if write else (32, 64)
        for g0 in range(0, min(flat.size, 64), group):  # the first wave stands for all: the maps repeat every 64 threads up to a row offset
            lanes = flat[g0:g0 + group]
            first_bank = (lanes * 2) % banks
            worst = 1
            for bk in range(0, banks, 2):
                worst = max(worst, len(set(lanes[first_bank == bk].tolist())))
            if write:
                self.write_conflicts += worst - 1
            else:
                self.read_conflicts += worst - 1

    def write(self, addr, val):
        self._note(addr, True)
        self.mem[np.clip(addr, 0, self.words - 1)] = val

    def read(self, addr):
        self._note(addr, False)
        return self.mem[np.clip(addr, 0, self.words - 1)]


def small_dft(v, R, inverse):
    """R-point transforms along axis 0 (registers m + S i of a thread hold transform m, point i), natural in and out"""
    if R == 1:
        return v
    w = root_of_unity(R.bit_length() - 1)
    if inverse:
        w = pow(w, P - 2, P)
    return np.moveaxis(plain_ntt(np.moveaxis(v, 0, -1), w), -1, 0)


def workgroup_transform(v, plan, inverse, lds, q, w):
    """v[i][thread] = point q + i T of transform w; returns the same layout after the M-point transform"""
    T, NP, W = plan.T, len(plan.radix), tile_width(plan.logm)
    for p in range(NP):
        R, NS = plan.radix[p], plan.ns[p]
        S = 16 // R
        if p > 0:
            v = np.stack([lds.read((q + i * T) * W + w) for i in range(16)])
            tw = plan.twiddles(p, inverse)
            for m in range(S):
                jj = (q + m * T) % NS
                for i in range(R):
                    v[m + S * i] = mul(v[m + S * i], tw[i][jj])
        out = np.empty_like(v)
        for m in range(S):
            out[m::S] = small_dft(v[m::S], R, inverse)
        v = out
        if p < NP - 1:
            for m in range(S):
                j = q + m * T
                base = (j // NS) * NS * R + (j % NS)
                for k in range(R):
                    lds.write((base + k * NS) * W + w, v[m + S * k])
    return v


_pow_cache = {}


def pow_table(wn, n):
    """all n powers of wn (one table kept)"""
    if (wn, n) not in _pow_cache:
        _pow_cache.clear()
        _pow_cache[(wn, n)] = powers(wn, n)
    return _pow_cache[(wn, n)]


def long_transform(x, log_n, inverse, pre=None, post=None, stats=None):
    """x: one vector of n words -> its transform, as the two launches compute it"""
    a, b = split(log_n)
    A, B, n = 1 << a, 1 << b, 1 << log_n
    wn = root_of_unity(log_n)
    if inverse:
        wn = pow(wn, P - 2, P)
    mid, out = np.zeros(n, dtype=U), np.zeros(n, dtype=U)
    # ---- pass 1
    plan, W = Plan(a), tile_width(a)
    tid = np.arange(plan.T * W)
    q, w = tid // W, tid % W
    for tile in range(B // W):
        lds = Lds(W * (A + 1))
        j0 = tile * W + w
        src = (q[None, :] + np.arange(16)[:, None] * plan.T) * B + j0[None, :]
        v = x[src]
        if pre is not None:
            v = mul(v, pre[src])
        v = workgroup_transform(v, plan, inverse, lds, q, w)
        for i in range(16):
            lds.write(w * (A + 1) + q + i * plan.T, v[i])
        for i in range(16):  # the tile's W runs of A words back to back: word e = r A + k1, adjacent lanes on adjacent words
            e = tid + i * tid.size
            mid[tile * W * A + e] = lds.read((e >> a) * (A + 1) + (e & (A - 1)))
        if stats is not None and tile == 0:
            stats.append(("pass1", a, lds))
    # ---- pass 2
    plan, W = Plan(b), tile_width(b)
    tid = np.arange(plan.T * W)
    q, w = tid // W, tid % W
    for tile in range(A // W):
        lds = Lds(W * B)
        k1 = tile * W + w
        pt = q[None, :] + np.arange(16)[:, None] * plan.T
        src = pt * A + k1[None, :]
        v = mul(mid[src], pow_table(wn, n)[(pt * k1[None, :]) % n])  # the table tw[p A + k1] = wn^(p k1)
        v = workgroup_transform(v, plan, inverse, lds, q, w)
        if post is not None:
            v = mul(v, post[src])
        out[src] = v
        if stats is not None and tile == 0:
            stats.append(("pass2", b, lds))
    return out


def lde_column(values, log_n, rate_bits, stats=None):
    """values -> (coefficients, lde [2^rate][n] coset-major) as launch_lde_columns_long computes them"""
    n = 1 << log_n
    coeffs = long_transform(values, log_n, True, stats=stats)
    wN = root_of_unity(log_n + rate_bits)
    lde = []
    for s in range(1 << rate_bits):
        cs = powers(GEN * pow(wN, s, P) % P, n)
        lde.append(long_transform(coeffs, log_n, False, pre=cs, stats=stats))
    return coeffs, np.stack(lde)


def reference_lde(values, log_n, rate_bits):
    n = 1 << log_n
    wn = root_of_unity(log_n)
    coeffs = mul(plain_ntt(values, pow(wn, P - 2, P)), U(pow(n, P - 2, P)))
    wN = root_of_unity(log_n + rate_bits)
    return coeffs, np.stack([plain_ntt(mul(coeffs, powers(GEN * pow(wN, s, P) % P, n)), wn) for s in range(1 << rate_bits)])


def check(log_n, rate_bits, seed=1):
    """Returns a dict of findings; raises AssertionError where the model and the plain NTT differ."""
    n = 1 << log_n
    rng = np.random.default_rng(seed)
    values = rng.integers(0, P, size=n, dtype=U)
    stats = []
    coeffs, lde = lde_column(values, log_n, rate_bits, stats)
    rc, rl = reference_lde(values, log_n, rate_bits)
    assert np.array_equal(coeffs, rc), f"coefficients differ at log_n {log_n}"
    assert np.array_equal(lde, rl), f"LDE differs at log_n {log_n} rate_bits {rate_bits}"
    # the reference itself against direct sums in Python integers: LDE point (s, k) is the polynomial at 7 w_N^(k R + s)
    pr = random.Random(seed)
    wN = root_of_unity(log_n + rate_bits)
    for _ in range(2):
        s, k = pr.randrange(1 << rate_bits), pr.randrange(n)
        x = GEN * pow(wN, (k << rate_bits) + s, P) % P
        acc = 0
        for cf in reversed(rc.tolist()):
            acc = (acc * x + cf) % P
        assert acc == int(rl[s][k]), "plain NTT differs from the direct evaluation"
    return {"log_n": log_n, "split": split(log_n), "out_of_bounds": sum(l.out_of_bounds for _, _, l in stats),
            "read_conflicts": sum(l.read_conflicts for _, _, l in stats), "write_conflicts": sum(l.write_conflicts for _, _, l in stats),
            "lds_words": max(l.words for _, _, l in stats)}


def check_vector(log_n, inverse=False, seed=2):
    """One transform of a vector of 2^log_n words (the lengths above 2^20 have narrower tiles) against the plain NTT"""
    n = 1 << log_n
    x = np.random.default_rng(seed).integers(0, P, size=n, dtype=U)
    stats = []
    got = long_transform(x, log_n, inverse, stats=stats)
    wn = root_of_unity(log_n)
    want = mul(plain_ntt(x, pow(wn, P - 2, P)), U(pow(n, P - 2, P))) if inverse else plain_ntt(x, wn)
    assert np.array_equal(got, want), f"transform differs at log_n {log_n}"
    return {"log_n": log_n, "split": split(log_n), "tile_words": (tile_width(split(log_n)[0]), tile_width(split(log_n)[1])),
            "out_of_bounds": sum(l.out_of_bounds for _, _, l in stats), "read_conflicts": sum(l.read_conflicts for _, _, l in stats),
            "write_conflicts": sum(l.write_conflicts for _, _, l in stats), "lds_words": max(l.words for _, _, l in stats)}


def main():
    for log_n in range(14, 21):
        print(check(log_n, 1))
    print(check_vector(21))
    return 0


if __name__ == "__main__":
    sys.exit(main())

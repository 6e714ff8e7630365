"""Hand-written AIRs for the quotient's constraint classes (csrc/quotient_plan.h), each with a satisfying trace, and the quotient's
coefficient chunks computed twice in Python integers: from all 2^qdb n values at once, and class by class from the cosets each class
needs.  Test code."""
import random

import numpy as np

import air_blob as AB
from starky_bls12_381_amd.air_builder import AirBuilder

P = 0xFFFFFFFF00000001
GEN = 7  # the coset shift of the LDE and of the quotient domain


def root_of_unity(log_n):
    return pow(GEN, (P - 1) >> log_n, P)


def inv(x):
    return pow(x, P - 2, P)


def class_air(n, top=4, degree=5, seed=1):
    """(blob, row-major trace [n][19], public inputs) of an AIR of declared `degree` with plain, transition, first-row and last-row
    constraints of every class 1 .. top (top <= degree - 1 <= 4): d cell factors make class d - 1 (plain, transition) or d (first, last)."""
    assert 1 <= top <= degree - 1 <= 4 and n >= 4
    rng = random.Random(seed * 1000 + n)
    rnd = lambda: [rng.randrange(P) for _ in range(n)]
    x, y, z = rnd(), rnd(), rnd()
    g, h = ([rng.randrange(2) for _ in range(n)] for _ in range(2))
    g[0] = h[0] = g[n - 1] = h[n - 1] = g[1] = h[1] = 1  # the gated constraints bind somewhere
    xyz = [x[r] * y[r] * z[r] % P for r in range(n)]
    rec = [rng.randrange(P)]
    for r in range(n - 1):
        rec.append((3 * rec[r] + x[r]) % P)
    u = [rng.randrange(P)]
    for r in range(n - 1):
        u.append(u[r] * x[r] % P * y[r] % P)
    w2 = [x[r] * y[r] % P for r in range(n)]
    w4 = [xyz[r] if g[r] else rng.randrange(P) for r in range(n)]
    w5 = [xyz[r] if g[r] and h[r] else rng.randrange(P) for r in range(n)]
    v, p = rnd(), rnd()
    for r in range(n - 1):
        if g[r] and h[r]:
            v[r + 1] = xyz[r]
        if g[r]:
            p[r + 1] = xyz[r]
    f2, f3, f4, l2, l3, l4 = (rnd() for _ in range(6))
    f2[0], f3[0], f4[0] = w2[0], xyz[0], xyz[0]
    l2[n - 1], l3[n - 1], l4[n - 1] = w2[n - 1], xyz[n - 1], xyz[n - 1]
    cols = [x, y, z, g, h, rec, w2, xyz, w4, w5, u, v, p, f2, f3, f4, l2, l3, l4]
    pis = [rec[0], rec[n - 1]]
    b = AirBuilder(len(cols), len(pis), degree)
    L, N = b.L, b.N
    prod3 = lambda: L(0) * L(1) * L(2)
    # class 1
    b.constraint(L(3) * (1 - L(3)))
    b.constraint(L(4) * (1 - L(4)))
    b.constraint(L(6) - L(0) * L(1))
    b.transition(N(5) - L(5) * 3 - L(0))
    b.first_row(L(5) - b.PI(0))
    b.last_row(L(5) - b.PI(1))
    if top >= 2:
        b.constraint(L(7) - prod3())
        b.transition(N(10) - L(10) * L(0) * L(1))
        b.first_row(L(13) - L(0) * L(1))
        b.last_row(L(16) - L(0) * L(1))
    if top >= 3:
        b.constraint(L(3) * (L(8) - prod3()))
        b.transition(L(3) * (N(12) - prod3()))
        b.first_row(L(14) - prod3())
        b.last_row(L(17) - prod3())
    if top >= 4:
        b.constraint(L(3) * L(4) * (L(9) - prod3()))
        b.transition(L(3) * L(4) * (N(11) - prod3()))
        b.first_row(L(3) * (L(15) - prod3()))
        b.last_row(L(3) * (L(18) - prod3()))
    trace = np.array(cols, dtype=np.uint64).T.copy()
    return b.finish(), trace, np.array(pis, dtype=np.uint64)


def class_by_degrees(kind, gates, terms, n_big=1 << 13):
    """The class of one decoded constraint from the degree of its part of the quotient, multiplied out: every cell is a polynomial of
    degree n - 1, the masks have degree 0 (plain), 1 (transition: x - g^-1) and n - 1 (first / last row), Z_H has degree n."""
    d = max((sum(1 for var in m if not var & AB.PI_FLAG) for m in AB.expand(gates, terms)), default=0)
    n = n_big
    deg = d * (n - 1) + (0, 1, n - 1, n - 1)[kind] - n
    k = 1
    while deg >= k * n:
        k += 1
    return k


def _idft(vals, w_inv):
    n = len(vals)
    n_inv = inv(n)
    return [sum(vals[k] * pow(w_inv, j * k, P) for k in range(n)) % P * n_inv % P for j in range(n)]


def quotient_chunks(blob, trace, pis, classes, qdb, alpha, solve_table):
    """(chunks from all values, chunks class by class): [2^qdb][n] coefficient chunks of  sum_k mask c_k alpha^(K-1-k) / Z_H  for the
    row-major `trace`.  `classes`: the class of every constraint; `solve_table`: (ginv, cpow, vinv) of starkhip_quotient_solve_table."""
    prog = AB.parse_blob(blob)
    n, n_cols = trace.shape
    log_n = n.bit_length() - 1
    n_cosets, size = 1 << qdb, n << qdb
    w_n, w_size = root_of_unity(log_n), root_of_unity(log_n + qdb)
    coef = [_idft([int(v) for v in trace[:, c]], inv(w_n)) for c in range(n_cols)]
    xs = [GEN * pow(w_size, i, P) % P for i in range(size)]
    lde = [[sum(cf[j] * pow(xv, j, P) for j in range(n)) % P for cf in coef] for xv in xs]
    cons = [(kind, AB.expand(gates, terms)) for kind, gates, terms in AB.constraints(prog)]
    K = len(cons)
    assert K == len(classes)
    n_classes = max(int(c) for c in classes)
    g_inv = inv(w_n)
    # sums[k - 1][i]: the constraints of class k at point i, already divided by Z_H
    sums = [[0] * size for _ in range(n_classes)]
    for i, xv in enumerate(xs):
        zh = (pow(xv, n, P) - 1) % P
        masks = (1, (xv - g_inv) % P, zh * inv(n * (xv - 1) % P) % P, zh * inv(n * (w_n * xv - 1) % P) % P)
        nxt = lde[(i + n_cosets) % size]  # g x: the same coset, the next row
        zh_inv = inv(zh)
        for k, (kind, poly) in enumerate(cons):
            val = masks[kind] * AB.evaluate(poly, lde[i], nxt, pis) % P * pow(alpha, K - 1 - k, P) % P
            sums[int(classes[k]) - 1][i] = (sums[int(classes[k]) - 1][i] + val * zh_inv) % P
    total = [sum(s[i] for s in sums) % P for i in range(size)]
    full = _idft(total, inv(w_size))
    shift_inv = inv(GEN)
    full = [full[j] * pow(shift_inv, j, P) % P for j in range(size)]
    want = [full[m * n:(m + 1) * n] for m in range(n_cosets)]
    ginv, cpow, vinv = solve_table
    got = [[0] * n for _ in range(n_cosets)]
    for k in range(1, n_classes + 1):
        a = []
        for t in range(k):
            g_t = GEN * pow(w_size, t, P) % P
            assert int(ginv[t]) == inv(g_t) and int(cpow[t][1]) == pow(g_t, n, P)
            vals = [sums[k - 1][kk * n_cosets + t] for kk in range(n)]  # point i = kk 2^qdb + t is x = g_t w_n^kk
            at = _idft(vals, inv(w_n))
            a.append([at[j] * pow(int(ginv[t]), j, P) % P for j in range(n)])
        for m in range(k):
            for j in range(n):
                got[m][j] = (got[m][j] + sum(int(vinv[k][m][t]) * a[t][j] for t in range(k))) % P
    return want, got

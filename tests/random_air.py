"""Seeded random AIRs written with the Python builder (starky_bls12_381_amd/air_builder.py), each with a satisfying trace built
alongside it: boolean columns, recurrences pinned by first / last-row public inputs, product columns over local and next cells,
and gated columns (gates with and without complement) up to the declared degree.  Test code."""
import random

import numpy as np

from starky_bls12_381_amd.air_builder import AirBuilder, REF_NEXT

P = 0xFFFFFFFF00000001


def random_air(seed, n_cols, degree, n_rows):
    """(blob, row-major trace [n_rows][n_cols] uint64, public inputs uint64): the trace satisfies every constraint."""
    assert n_cols >= 1 and 2 <= degree <= 5 and n_rows >= 2
    rng = random.Random(seed)
    n = n_rows
    cols = []          # per column: list of n ints
    bools = []         # indices of 0/1 columns
    pis = []
    cons = []          # (kind, builder -> Expr) in order

    def new_col(vals):
        cols.append([v % P for v in vals])
        return len(cols) - 1

    def val(ref, r):
        return cols[ref & 0xFFFFFF][(r + 1) % n if ref & REF_NEXT else r]

    def cell(b, ref):
        return b.N(ref & 0xFFFFFF) if ref & REF_NEXT else b.L(ref)

    def pick_refs(k):
        return [rng.randrange(len(cols)) | (REF_NEXT if rng.random() < 0.3 else 0) for _ in range(k)]

    def product(refs, r):
        v = 1
        for ref in refs:
            v = v * val(ref, r) % P
        return v

    new_col([rng.randrange(P) for _ in range(n)])  # a free column to start from
    while len(cols) < n_cols:
        t = rng.randrange(6)
        if t == 0:  # free
            new_col([rng.randrange(P) for _ in range(n)])
        elif t == 1:  # boolean: b (1 - b) = 0
            b_ = new_col([rng.randrange(2) for _ in range(n)])
            bools.append(b_)
            cons.append(("constraint", lambda b, c=b_: b.L(c) * (1 - b.L(c))))
        elif t == 2:  # recurrence x' = a x + f (+-) PI, x[0] and x[n-1] public
            a, f, sign = rng.randrange(1, P), rng.randrange(len(cols)), rng.choice((1, -1))
            step = len(pis)
            pis.append(rng.randrange(P))
            x = [rng.randrange(P)]
            for r in range(n - 1):
                x.append((a * x[r] + cols[f][r] + sign * pis[step]) % P)
            c = new_col(x)
            i0, i1 = len(pis), len(pis) + 1
            pis += [x[0], x[n - 1]]
            cons.append(("first_row", lambda b, c=c, i=i0: b.L(c) - b.PI(i)))
            if sign > 0:
                cons.append(("transition", lambda b, c=c, a=a, f=f, s=step: b.N(c) - b.L(c) * a - b.L(f) - b.PI(s)))
            else:
                cons.append(("transition", lambda b, c=c, a=a, f=f, s=step: b.N(c) - b.L(c) * a - b.L(f) + b.PI(s)))
            cons.append(("last_row", lambda b, c=c, i=i1: b.L(c) - b.PI(i)))
        elif t == 3:  # product column w = k0 * prod(factors) + k1, factors local or next
            k = rng.randint(2, min(3, degree))
            refs = pick_refs(k)
            k0, k1 = rng.choice((1, P - 1, rng.randrange(2, P))), rng.choice((0, rng.randrange(P)))
            w = new_col([(k0 * product(refs, r) + k1) for r in range(n)])

            def mk(b, w=w, refs=refs, k0=k0, k1=k1):
                p = cell(b, refs[0])
                for ref in refs[1:]:
                    p = p * cell(b, ref)
                return b.L(w) - p * k0 - k1
            cons.append(("constraint", mk))
        elif bools:  # gated: prod(gates) * (w - prod(factors)), gates b or 1 - b, any kind
            kind = rng.choice(("constraint", "transition", "first_row", "last_row"))
            room = degree - (1 if kind in ("first_row", "last_row") else 0)
            g = rng.randint(1, min(2, room - 1, len(bools))) if room >= 2 else 0
            if g == 0:
                continue
            k = rng.randint(1, min(3, room - g))
            gates = [(bc, rng.random() < 0.5) for bc in rng.sample(bools, g)]
            refs = pick_refs(k)

            def gate_on(r):
                return all((cols[bc][r] == 0) if compl else (cols[bc][r] == 1) for bc, compl in gates)
            w = new_col([product(refs, r) if gate_on(r) else rng.randrange(P) for r in range(n)])

            def mk(b, w=w, refs=refs, gates=gates):
                e = None
                for bc, compl in gates:
                    ge = (1 - b.L(bc)) if compl else b.L(bc)
                    e = ge if e is None else e * ge
                p = cell(b, refs[0])
                for ref in refs[1:]:
                    p = p * cell(b, ref)
                return e * (b.L(w) - p)
            cons.append((kind, mk))
    b = AirBuilder(n_cols, len(pis), degree)
    for kind, mk in cons:
        getattr(b, kind)(mk(b))
    if b.count() == 0:  # at least one constraint: column 0 equals itself at row 0 (a PI)
        pis.append(cols[0][0])
        b = AirBuilder(n_cols, len(pis), degree)
        b.first_row(b.L(0) - b.PI(len(pis) - 1))
    trace = np.array(cols, dtype=np.uint64).T.copy()
    return b.finish(), trace, np.array(pis, dtype=np.uint64)


# (seed, columns, degree, rows): 1 to 300 columns (across the 64-column tiles), degrees 2 to 5
CASES = [(1, 1, 2, 8), (2, 7, 3, 16), (3, 40, 4, 32), (4, 64, 5, 64), (5, 65, 3, 128), (6, 130, 5, 256), (7, 200, 4, 1024),
         (8, 300, 5, 4096)]

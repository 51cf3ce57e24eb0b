"""Deterministic circuits of GENERAL gates for the prover's tests and tools/fuzz_prover.py.  TEST INFRASTRUCTURE: Python integers only,
no library call.  Every selector column is alive (the chained multiplications of the other prover tests have ql = qr = qc = 0, so a
wrong qc column or a dropped a*ql term passes them all):

  n_pub rows   (x, -, -)  ql = 1, PI = -x, x non-zero                                    ("x public", prover.rs:114-127)
  n_gates rows (a, b, c)  ql, qr, qm, qc each from {0, 1, q-1, random}, qo from {1, q-1, random non-zero},
                          c = -(ql a + qr b + qm a b + qc) / qo;  a and b are reused from the pool of earlier variables with
                          probability 0.6, so copy cycles run through all three columns
  gate row 0   reads two fresh variables of value 0 and q - 1
  gate row n_gates // 2 (when n_gates >= 2) is a constant row (-, -, c): only qc and qo alive, and c is used nowhere else -- a
                          cycle of length 1, and a cell that only the qc term constrains
  the other rows are empty.  Sigma columns: tests/circuit_frontend.make_s_polynomials (program.rs:76-147)."""
import random

from tests import bigint_model as M
from tests.circuit_frontend import make_s_polynomials

Q = M.Q
SELECTORS = ("ql", "qr", "qm", "qo", "qc")
# (n, n_pub, n_gates, seed) of the suite's general-gate proofs; tests/test_general_circuits.py pins what these seeds give.
# N = 4n = 64 is one wave; 512 is two workgroups and half the rows are empty; at n = 1024 one coset of the split spans four workgroups
SHAPES = ((16, 2, 14, 16), (128, 2, 64, 128), (1024, 2, 1022, 1024))
NO_PUBLIC = (128, 0, 64, 128)


def general_circuit(n, n_pub, n_gates, seed, small=False):
    """-> (cols, pk, public_column, publics): three witness columns of n integers, the eight circuit columns by name, the PI column
    (-x in the public rows) and the public values x themselves (what the verifier is given).  small=True draws values below 2^8."""
    assert n >= 8 and n & (n - 1) == 0 and n_pub >= 0 and n_gates >= 1 and n_pub + n_gates <= n
    rnd = random.Random(seed)
    val = lambda: rnd.randrange(1 << 8) if small else rnd.randrange(Q)
    nonzero = lambda: rnd.randrange(1, 1 << 8) if small else rnd.randrange(1, Q)
    values, pool = {}, []

    def new_var(v, pooled=True):
        name = "v%d" % len(values)
        values[name] = v % Q
        if pooled:
            pool.append(name)
        return name

    wires, sel, publics = [], {k: [] for k in SELECTORS}, []

    def row(a, b, c, ql, qr, qm, qo, qc):
        wires.append((a, b, c))
        for k, v in zip(SELECTORS, (ql, qr, qm, qo, qc)):
            sel[k].append(v % Q)

    for _ in range(n_pub):
        x = new_var(nonzero())
        publics.append(values[x])
        row(x, None, None, 1, 0, 0, 0, 0)
    constant_at = n_gates // 2 if n_gates >= 2 else -1
    for g in range(n_gates):
        qo = rnd.choice([1, Q - 1, nonzero()])
        if g == constant_at:
            qc = nonzero()
            row(None, None, new_var(-qc * pow(qo, Q - 2, Q), pooled=False), 0, 0, 0, qo, qc)
            continue
        if g == 0:
            a, b = new_var(0), new_var(Q - 1)
        else:
            a = rnd.choice(pool) if pool and rnd.random() < 0.6 else new_var(val())
            b = rnd.choice(pool) if rnd.random() < 0.6 else new_var(val())
        ql, qr, qm, qc = (rnd.choice([0, 1, Q - 1, val()]) for _ in range(4))
        va, vb = values[a], values[b]
        row(a, b, new_var(-(ql * va + qr * vb + qm * va * vb + qc) * pow(qo, Q - 2, Q)), ql, qr, qm, qo, qc)
    pk = {k: v + [0] * (n - len(v)) for k, v in sel.items()}
    rows, sig = make_s_polynomials(wires, n)
    pk.update(s1=sig[0], s2=sig[1], s3=sig[2])
    cols = [[values[r[j]] if r[j] else 0 for r in rows] for j in range(3)]
    public_column = [(-x) % Q for x in publics] + [0] * (n - n_pub)
    return cols, pk, public_column, publics


# ---- reading a circuit back from its columns alone (what the tests break and what they count) -------------------------------

def gate_residual(pk, cols, public_column, i):
    """ql a + qr b + qm a b + qo c + PI + qc of row i: zero on a satisfying witness (prover.rs:370-376)"""
    a, b, c = cols[0][i], cols[1][i], cols[2][i]
    return (pk["ql"][i] * a + pk["qr"][i] * b + pk["qm"][i] * a * b + pk["qo"][i] * c + public_column[i] + pk["qc"][i]) % Q


def constant_row(n_pub, n_gates):
    """where general_circuit puts its constant row (-, -, c): only qc and qo alive, a and b empty, c used nowhere else.  (A wired row
    can draw ql = qr = qm = 0 as well; its a and b cells still belong to variables.)"""
    assert n_gates >= 2
    return n_pub + n_gates // 2


def gate_rows(pk):
    """the rows a gate lives in (qo != 0: public rows and empty rows have qo = 0)"""
    return [i for i in range(len(pk["qo"])) if pk["qo"][i]]


def copy_cycles(pk):
    """the cycles of the permutation that s1, s2, s3 encode, as lists of (column, row): cell (col', row') holds the label
    (col + 1) w^row of the cell in front of it in its cycle (program.rs:126-137)"""
    n = len(pk["s1"])
    om, cell, x = M.omega(n), {}, 1
    for r in range(n):
        for col in range(3):
            cell[(col + 1) * x % Q] = (col, r)
        x = x * om % Q
    assert len(cell) == 3 * n
    sig = (pk["s1"], pk["s2"], pk["s3"])
    seen, cycles = set(), []
    for start in sorted(cell.values()):
        if start in seen:
            continue
        cyc, cur = [], start
        while cur not in seen:
            seen.add(cur)
            cyc.append(cur)
            cur = cell[sig[cur[0]][cur[1]]]
        assert cur == start, "s1, s2, s3 do not encode a permutation"
        cycles.append(cyc)
    return cycles


def named_cycles(pk, row):
    """copy_cycles without the one cycle of the EMPTY cells: the cycle that holds the unused A cell of the constant row `row`"""
    return [c for c in copy_cycles(pk) if (0, row) not in c]


def c_to_b_copy(pk, row):
    """(i, j): column C of row i and column B of row j lie in one copy cycle, row j's own output is used nowhere else (so b_j can be
    changed and c_j recomputed: every gate still holds and only the copy constraint is broken)"""
    cycles = named_cycles(pk, row)
    alone = {c[0] for c in cycles if len(c) == 1}
    for cyc in cycles:
        outs = [r for col, r in cyc if col == 2]
        for col, j in cyc:
            if col == 1 and outs and outs[0] != j and (2, j) in alone and (0, j) not in cyc:
                return outs[0], j
    return None

"""Circuits as bp_circuit_load_wires takes them: three variable ids per row, five selector values per row and one value per variable.
TEST INFRASTRUCTURE: Python integers only, no library call.

  general_wire_circuit   tests/general_circuits.general_circuit with the variables numbered instead of named: the same random stream, so
                         the same gates, values and copy cycles (tests/test_wire_plan.py holds the two against each other); id k is the
                         k-th variable made, 0 the empty wire, values[0] a slot nothing reads
  id_shapes              wire-id tables that stress the sort and the link pass of csrc/wire_plan.hpp, by name
  expected_target        the cell map of program.rs:76-147 from a dictionary of lists: cells of one id form a cycle in row-major order
                         and target[next] = this"""
import random

import numpy as np

from tests import bigint_model as M
from tests import general_circuits as G

Q = M.Q
SELECTORS = G.SELECTORS
SHAPES = G.SHAPES                      # (n, n_pub, n_gates, seed): n = 16, 128, 1024
NO_PUBLIC = G.NO_PUBLIC
# ids whose digits sit at every edge of the four 8-bit passes
EDGE_IDS = (1, 255, 256, 65535, 65536, 1 << 24, 1 << 31, (1 << 32) - 1)


def general_wire_circuit(n, n_pub, n_gates, seed):
    """-> dict: ids [n, 3] uint32, values (list of integers, values[id]), sel {name: n integers}, cols (a, b, c expanded), public_column
    (-x in the public rows), publics, n_public"""
    assert n >= 8 and n & (n - 1) == 0 and n_pub >= 0 and n_gates >= 1 and n_pub + n_gates <= n
    rnd = random.Random(seed)
    val = lambda: rnd.randrange(Q)
    nonzero = lambda: rnd.randrange(1, Q)
    values, pool = [0], []

    def new_var(v, pooled=True):
        values.append(v % Q)
        if pooled:
            pool.append(len(values) - 1)
        return len(values) - 1

    wires, sel, publics = [], {k: [] for k in SELECTORS}, []

    def row(a, b, c, ql, qr, qm, qo, qc):
        wires.append((a, b, c))
        for k, v in zip(SELECTORS, (ql, qr, qm, qo, qc)):
            sel[k].append(v % Q)

    for _ in range(n_pub):
        x = new_var(nonzero())
        publics.append(values[x])
        row(x, 0, 0, 1, 0, 0, 0, 0)
    constant_at = n_gates // 2 if n_gates >= 2 else -1
    for g in range(n_gates):
        qo = rnd.choice([1, Q - 1, nonzero()])
        if g == constant_at:
            qc = nonzero()
            row(0, 0, new_var(-qc * pow(qo, Q - 2, Q), pooled=False), 0, 0, 0, qo, qc)
            continue
        if g == 0:
            a, b = new_var(0), new_var(Q - 1)
        else:
            a = rnd.choice(pool) if pool and rnd.random() < 0.6 else new_var(val())
            b = rnd.choice(pool) if rnd.random() < 0.6 else new_var(val())
        ql, qr, qm, qc = (rnd.choice([0, 1, Q - 1, val()]) for _ in range(4))
        va, vb = values[a], values[b]
        row(a, b, new_var(-(ql * va + qr * vb + qm * va * vb + qc) * pow(qo, Q - 2, Q)), ql, qr, qm, qo, qc)
    wires += [(0, 0, 0)] * (n - len(wires))
    ids = np.array(wires, dtype=np.uint32)
    cols = [[values[r[j]] for r in wires] for j in range(3)]
    return dict(ids=ids, values=values, sel={k: v + [0] * (n - len(v)) for k, v in sel.items()}, cols=cols,
                public_column=[(-x) % Q for x in publics] + [0] * (n - n_pub), publics=publics, n_public=n_pub)


def id_shapes(n, seed=7):
    """{name: (ids [n, 3] uint32, passes the sort needs)} at 2^k rows"""
    cells = 3 * n
    rnd = random.Random(seed * 1000003 + n)
    flat = {}
    flat["all_zero"] = [0] * cells
    flat["all_distinct"] = list(range(1, cells + 1))
    flat["two_alternating"] = [5 if k % 2 else 9 for k in range(cells)]
    big = [7] * cells
    big[0], big[cells // 2], big[cells - 1] = 300, 2, 70000                   # three cells of their own: first, middle, last
    flat["one_group_but_three"] = big
    for passes in (1, 2, 3, 4):                                               # the edge ids a sort of `passes` passes can hold
        pool = [i for i in EDGE_IDS if i < 1 << (8 * passes)]
        mixed = [rnd.choice(pool) for _ in range(cells)]
        mixed[rnd.randrange(cells)] = max(pool)
        flat["edge_ids_%d" % passes] = mixed
    flat["random_repeats"] = [rnd.randrange(n) for _ in range(cells)]
    if n == 8:                                                                # program.rs:206-235: c <== a * b, b <== a * e
        a, b, c, e = 1, 2, 3, 4
        flat["reference_case"] = [a, b, c, a, e, b] + [0] * (cells - 6)
    out = {}
    for name, v in flat.items():
        top, passes = max(v), 0
        while top >> (8 * passes):
            passes += 1
        out[name] = (np.array(v, dtype=np.uint32).reshape(n, 3), passes)
    return out


def expected_target(ids):
    """target[3 * row + col]: the cell in front of this one in its id's row-major cycle (the last cell, for the first)"""
    flat = [int(v) for v in np.asarray(ids).reshape(-1)]
    groups = {}
    for cell, v in enumerate(flat):
        groups.setdefault(v, []).append(cell)
    target = [None] * len(flat)
    for cells in groups.values():
        for i, cell in enumerate(cells):
            target[cell] = cells[i - 1]
    return target

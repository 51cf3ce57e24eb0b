"""bp_circuit_check_sigma / bp_circuit_check_witness on the GPU: which gate rows and which copy constraints a witness violates, and
whether S1 S2 S3 encode a permutation at all.  Every expectation is a Python integer: the gate residual of tests/general_circuits.py,
the permutation read back from the labels with a Python dictionary, and closed forms on the chained multiplications (cell (2, i) <->
(0, i + 1), every other cell a fixed point).  None comes from the library.  Sizes: n = 8 is less than a wave, 256 one workgroup of the
row kernel, 512 breaks rows 255 | 256 across a workgroup edge, 1024 and 4096 span several workgroups."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import baby_plonk_rust_amd as bp
from baby_plonk_rust_amd import synthetic
from tests import bigint_model as M
from tests import general_circuits as G

pytestmark = pytest.mark.gpu
Q = M.Q
R = pow(2, 256, Q)
ABSENT = 0xFFFFFFFFFFFFFFFF
STATE = {"dead": None}
SHAPES = G.SHAPES + (G.NO_PUBLIC,)
SHAPE_IDS = ["n%d" % s[0] for s in G.SHAPES] + ["n128_no_public"]


def call(fn, *args, **kw):
    """every library call of this module: after a HIP error (BP_ERR_HIP, -9) nothing more is started on the card"""
    if STATE["dead"]:
        pytest.fail("not launched: %s" % STATE["dead"])
    try:
        return fn(*args, **kw)
    except bp.BpError as e:
        if e.code == -9:
            STATE["dead"] = str(e)
        raise


def mont(values):
    """Python integers -> [n, 4] Montgomery limbs"""
    raw = b"".join((v % Q * R % Q).to_bytes(32, "little") for v in values)
    return np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4).copy()


def le_bytes(values):
    return np.frombuffer(b"".join((v % Q).to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(-1, 32).copy()


def permutation(pk):
    """sigma as Python reads it from the labels: {(col, row): (col', row')}, S_col[row] = (col' + 1) w^row'"""
    n = len(pk["s1"])
    om, cell, x = M.omega(n), {}, 1
    for r in range(n):
        for col in range(3):
            cell[(col + 1) * x % Q] = (col, r)
        x = x * om % Q
    sig = (pk["s1"], pk["s2"], pk["s3"])
    return {(col, r): cell.get(sig[col][r]) for r in range(n) for col in range(3)}


def expected(pk, cols, public, sigma):
    """the WitnessReport Python computes: rows with a residual, cells u with value(u) != value(sigma(u)), lowest by 3 * row + col"""
    n = len(cols[0])
    rows = [i for i in range(n) if G.gate_residual(pk, cols, public, i)]
    cells = [(col, r) for r in range(n) for col in range(3) if cols[col][r] != cols[sigma[(col, r)][0]][sigma[(col, r)][1]]]
    return bp.WitnessReport(len(rows), rows[0] if rows else None, len(cells), cells[0] if cells else None, sigma[cells[0]] if cells else None)


class Case:
    """one general-gate circuit, its satisfying witness, the four broken witnesses of tests/test_gpu_prover_general.py and what Python
    expects of each: computed once per shape and never changed"""

    def __init__(self, shape):
        self.shape = shape
        self.n, self.n_pub, self.n_gates, _ = shape
        self.cols, self.pk, self.public, _ = G.general_circuit(*shape)
        self.pkv = {k: mont(v) for k, v in self.pk.items()}
        self.sigma = permutation(self.pk)
        assert sorted(self.sigma.values()) == sorted(self.sigma)
        c, pk = self, self.pk
        self.witnesses = [("good", self.cols, self.public)]
        i = G.constant_row(c.n_pub, c.n_gates)                       # the constant row (-, -, c): only the qc term contradicts c + 1
        bad = [list(x) for x in c.cols]
        bad[2][i] = (bad[2][i] + 1) % Q
        self.witnesses.append(("constant row", bad, self.public))
        alone = {cyc[0] for cyc in G.copy_cycles(pk) if len(cyc) == 1}      # an addition row whose output is used nowhere else
        i = [r for r in G.gate_rows(pk) if pk["qm"][r] == 0 and (pk["ql"][r] or pk["qr"][r]) and (2, r) in alone][0]
        bad = [list(x) for x in c.cols]
        bad[2][i] = (bad[2][i] + 1) % Q
        self.witnesses.append(("addition row", bad, self.public))
        public = list(c.public)                                      # a wrong public value (no public rows: row 1's PI is simply not zero)
        public[1] = (public[1] + 1) % Q
        self.witnesses.append(("public value", self.cols, public))
        i, j = G.c_to_b_copy(pk, G.constant_row(c.n_pub, c.n_gates))         # a C-to-B copy broken, every gate still holding
        bad = [list(x) for x in c.cols]
        bad[1][j] = (bad[1][j] + 1) % Q
        a, b = bad[0][j], bad[1][j]
        bad[2][j] = -(pk["ql"][j] * a + pk["qr"][j] * b + pk["qm"][j] * a * b + pk["qc"][j]) * pow(pk["qo"][j], Q - 2, Q) % Q
        self.witnesses.append(("copy constraint", bad, self.public))
        self.want = {what: expected(pk, cols, public, self.sigma) for what, cols, public in self.witnesses}
        w = self.want
        assert w["good"] == bp.WitnessReport(0, None, 0, None, None)
        assert all(w[k].gate_rows == 1 and w[k].copy_cells == 0 for k in ("constant row", "addition row", "public value"))
        assert w["public value"].first_gate_row == 1
        # b_j differs from its cycle, c_j (used nowhere else) follows: the edge into (1, j) and the edge out of it, nothing else
        assert w["copy constraint"].gate_rows == 0 and w["copy constraint"].copy_cells == 2

    def reports(self, circuit):
        return {what: call(circuit.check_witness, *[mont(x) for x in cols], mont(public)) for what, cols, public in self.witnesses}


@functools.lru_cache(maxsize=None)
def case(shape):
    return Case(shape)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_general_gates_counts_and_lowest_positions(shape):
    c = case(shape)
    circuit = call(bp.Circuit, c.pkv)
    try:
        assert call(circuit.check_sigma) == bp.SigmaReport(0, None, 0, None)
        got = c.reports(circuit)
        for what in c.want:
            assert got[what] == c.want[what], what
        assert got["good"].ok and not any(got[k].ok for k in got if k != "good")
    finally:
        circuit.free()


def test_the_prover_refuses_exactly_what_the_check_rejects_and_a_check_disturbs_nothing():
    from tests.test_gpu_prover_general import case as proof_case
    c, p = case(G.SHAPES[0]), proof_case(G.SHAPES[0])                # n = 16; p.want: the CPU oracle's proof of the good witness
    circuit = call(bp.Circuit, c.pkv)
    prover = bp.Prover(p.setup, circuit)
    try:
        assert call(prover.prove_with_blinding, *p.wit, p.pi, p.blinders) == p.want
        for what, cols, public in c.witnesses:
            rep = call(prover.check, *[mont(x) for x in cols], mont(public))
            assert rep == c.want[what], what
            if rep.ok:
                assert call(prover.prove_with_blinding, *[mont(x) for x in cols], mont(public), p.blinders) == p.want
            else:
                with pytest.raises(bp.BpError) as e:
                    call(prover.prove_with_blinding, *[mont(x) for x in cols], mont(public), p.blinders)
                assert e.value.code == -11, what
            assert call(prover.prove_with_blinding, *p.wit, p.pi, p.blinders) == p.want, what
    finally:
        circuit.free()


# ---- grid edges on the chained multiplications: row i = (x_i, y_i, x_i y_i), x_(i+1) = the product ----------------------------------

def bump(column, i):
    column[i] = bp.scalar_from_int((bp.scalar_to_int(column[i]) + 1) % Q)


def chained_rows(n):
    """the sets of rows to break, each by its b value: the gate of that row fails and no copy does (b_i is used once)"""
    edges = sorted({r for k in range(256, n, 256) for r in (k - 1, k)})
    sets = {"row 0": [0], "last row": [n - 1], "17 rows": sorted(random.Random(n).sample(range(n), min(17, n)))}
    if edges:
        sets["workgroup edges"] = edges
    return sets


@pytest.mark.parametrize("n", [8, 256, 512, 4096])
def test_chained_multiplications_rows_and_copy_cells_at_the_grid_edges(n):
    wit, pk = synthetic.chained_multiplications(n, 7)
    circuit = call(bp.Circuit, pk)
    try:
        assert call(circuit.check_sigma).ok
        assert call(circuit.check_witness, *wit) == bp.WitnessReport(0, None, 0, None, None)
        for what, rows in chained_rows(n).items():
            bad = [w.copy() for w in wit]
            for i in rows:
                bump(bad[1], i)
            assert call(circuit.check_witness, *bad) == bp.WitnessReport(len(rows), rows[0], 0, None, None), what
        # a_0 and c_(n-1) are fixed points of sigma: their rows fail, no copy does
        bad = [w.copy() for w in wit]
        bump(bad[0], 0)
        bump(bad[2], n - 1)
        assert call(circuit.check_witness, *bad) == bp.WitnessReport(2, 0, 0, None, None)
        # five products c_i changed, i < n - 1: row i fails, and so do both edges of the cycle (2, i) <-> (0, i + 1)
        five = set(random.Random(n + 1).sample(range(n - 1), 5))
        if n > 256:
            five = set(sorted(five)[:4]) | {255}                     # c_255 and a_256 sit in different workgroups
        five = sorted(five)
        bad = [w.copy() for w in wit]
        for i in five:
            bump(bad[2], i)
        assert call(circuit.check_witness, *bad) == bp.WitnessReport(5, five[0], 10, (2, five[0]), (0, five[0] + 1))
        # the same edge seen from its other end alone: a_1 changed (row 1 fails as well)
        bad = [w.copy() for w in wit]
        bump(bad[0], 1)
        assert call(circuit.check_witness, *bad) == bp.WitnessReport(1, 1, 2, (2, 0), (0, 1))
    finally:
        circuit.free()


# ---- forms of the witness ---------------------------------------------------------------------------------------------------------------

def raw_check(ctx, handle, ptrs, fmt, on_device):
    """bp_circuit_check_witness itself -> (return code, the five report words, pre-set to a mark)"""
    if STATE["dead"]:
        pytest.fail("not launched: %s" % STATE["dead"])
    rep = (C.c_uint64 * 5)(*[0x1122334455667788] * 5)
    rc = ctx._lib.bp_circuit_check_witness(ctx._h, handle, *ptrs, fmt, on_device, rep)
    if rc == -9:
        STATE["dead"] = "bp_circuit_check_witness returned BP_ERR_HIP"
    return rc, list(rep)


def test_host_montgomery_bytes_and_device_witnesses_give_one_report():
    import torch
    c = case(G.SHAPES[0])
    circuit = call(bp.Circuit, c.pkv)
    try:
        for what, cols, public in c.witnesses[2:]:                   # a gate row, the public value, a copy constraint
            want = c.want[what]
            assert call(circuit.check_witness, *[mont(x) for x in cols], mont(public)) == want, what
            assert call(circuit.check_witness, *[le_bytes(x) for x in cols], le_bytes(public), fmt=bp.FR_BYTES_LE) == want, what
            t = [torch.from_numpy(mont(x).view(np.int64)).cuda() for x in list(cols) + [public]]
            torch.cuda.synchronize()
            assert call(circuit.check_witness_device, *[x.data_ptr() for x in t]) == want, what
        # refusals: report untouched
        cols = [le_bytes(x) for x in c.cols] + [le_bytes(c.public)]
        cols[1][c.n - 1] = np.frombuffer(Q.to_bytes(32, "little"), dtype=np.uint8)
        mark = [0x1122334455667788] * 5
        assert raw_check(circuit.ctx, circuit.handle, [x.ctypes.data for x in cols], bp.FR_BYTES_LE, 0) == (-4, mark)
        assert b"witness" in circuit.ctx._lib.bp_last_error(circuit.ctx._h)
        t = [torch.from_numpy(mont(x).view(np.int64)).cuda() for x in list(c.cols) + [c.public]]
        torch.cuda.synchronize()
        assert raw_check(circuit.ctx, circuit.handle, [x.data_ptr() for x in t], bp.FR_BYTES_LE, 1) == (-1, mark)
        good = [mont(x) for x in c.cols] + [mont(c.public)]
        assert raw_check(circuit.ctx, circuit.handle + 1000, [x.ctypes.data for x in good], bp.FR_MONT, 0) == (-1, mark)
        assert raw_check(circuit.ctx, circuit.handle, [x.ctypes.data for x in good], bp.FR_MONT, 0) == (0, [0, ABSENT, 0, ABSENT, ABSENT])
        rep4 = (C.c_uint64 * 4)(*mark[:4])
        assert circuit.ctx._lib.bp_circuit_check_sigma(circuit.ctx._h, circuit.handle + 1000, rep4) == -1 and list(rep4) == mark[:4]
    finally:
        circuit.free()


def test_no_public_input_equals_the_zero_column():
    c = case(G.NO_PUBLIC)
    assert c.public == [0] * c.n
    circuit = call(bp.Circuit, c.pkv)
    try:
        for what, cols, public in c.witnesses:
            if what == "public value":
                continue
            w = [mont(x) for x in cols]
            assert call(circuit.check_witness, *w, None) == call(circuit.check_witness, *w, mont(public)) == c.want[what], what
            assert call(circuit.check_witness, *[le_bytes(x) for x in cols], None, fmt=bp.FR_BYTES_LE) == c.want[what], what
    finally:
        circuit.free()


# ---- sigma columns that are no permutation -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [G.SHAPES[0], G.SHAPES[2]], ids=["n16", "n1024"])
def test_sigma_defects_are_counted_and_located_and_the_witness_check_refuses(shape):
    c = case(shape)
    n, om = c.n, M.omega(c.n)
    names = ("s1", "s2", "s3")
    number = lambda cell: 3 * cell[1] + cell[0]
    witness = [mont(x) for x in c.cols] + [mont(c.public)]
    for col, row in ((0, 0), (0, n - 1), (2, 0), (2, n - 1)):        # the first and the last cell of S1 and of S3
        u = (col, row)
        # (a) a value that is no label, 4 w^r: cell u names nothing, and the cell it named is nobody's target
        pk = {k: list(v) for k, v in c.pk.items()}
        pk[names[col]][row] = 4 * pow(om, row, Q) % Q
        want_a = bp.SigmaReport(1, u, 1, c.sigma[u])
        # (b) the label another cell holds: v's target is named twice, u's own never; no value is a bad label
        v = next(x for x in sorted(c.sigma, key=number) if x != u and c.sigma[x] != c.sigma[u] and x[1] == n // 2)
        pk_b = {k: list(v_) for k, v_ in c.pk.items()}
        pk_b[names[col]][row] = c.pk[names[v[0]]][v[1]]
        want_b = bp.SigmaReport(0, None, 2, min(c.sigma[u], c.sigma[v], key=number))
        for cols, want, named in ((pk, want_a, u), (pk_b, want_b, want_b.first_bad_indegree)):
            circuit = call(bp.Circuit, {k: mont(x) for k, x in cols.items()})
            try:
                assert call(circuit.check_sigma) == want, (u, want)
                assert call(circuit.check_sigma) == want             # the cached answer
                with pytest.raises(bp.BpError) as e:
                    call(circuit.check_witness, *witness)
                assert e.value.code == -1
                assert "bp_circuit_check_sigma" in str(e.value) and "cell %d " % number(named) in str(e.value), str(e.value)
            finally:
                circuit.free()


def test_the_decode_runs_once_per_circuit_load():
    c = case(G.SHAPES[1])
    witness = [mont(x) for x in c.cols] + [mont(c.public)]
    circuit = call(bp.Circuit, c.pkv)
    assert call(circuit.check_witness, *witness).ok
    first = circuit.check_stats()
    assert call(circuit.check_witness, *witness).ok
    second = circuit.check_stats()
    assert call(circuit.check_sigma).ok
    third = circuit.check_stats()
    circuit.free()
    assert first["decode_ms"] > 0 and first["check_ms"] > 0 and first["upload_ms"] > 0
    assert second["decode_ms"] == 0 and second["check_ms"] > 0
    assert third == {"decode_ms": 0, "upload_ms": 0, "check_ms": 0}
    circuit = call(bp.Circuit, c.pkv)                                # a fresh load decodes again, whichever call comes first
    assert call(circuit.check_sigma).ok
    assert circuit.check_stats()["decode_ms"] > 0
    assert call(circuit.check_witness, *witness).ok
    assert circuit.check_stats()["decode_ms"] == 0
    circuit.free()


def test_a_two_member_group_gives_the_reports_of_one_device():
    c = case(G.SHAPES[1])
    ctx = call(bp.Context, [0, 0])
    try:
        circuit = call(bp.Circuit, c.pkv, ctx)
        assert call(circuit.check_sigma) == bp.SigmaReport(0, None, 0, None)
        got = c.reports(circuit)
        for what in c.want:
            assert got[what] == c.want[what], what
        circuit.free()
    finally:
        ctx.close()


def test_no_launch_was_refused():
    assert STATE["dead"] is None

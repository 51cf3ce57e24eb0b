"""-m gpu: circuits loaded by wire ids (bp_circuit_load_wires) and witnesses gathered from a value per variable (bp_circuit_assign_device,
bp_prove_assignment).  The sigma columns the GPU sorts and links are held byte for byte against bp_make_s_polynomials (the host code,
pinned to the reference by tests/test_circuit_frontend.py), the cell map against a Python dictionary of lists through the copy check,
the gathered columns against Python integers, and proofs against bp_prove on the expanded columns.  Shapes and sizes:
tests/wire_circuits.py; log_n 3 is less than a wave, 6 less than a tile, 10 two tiles, 12 and 16 span one and many scan chunks."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import baby_plonk_rust_amd as bp
from tests import bigint_model as M
from tests import general_circuits as G
from tests import wire_circuits as W

pytestmark = pytest.mark.gpu
Q = M.Q
R = pow(2, 256, Q)
STATE = {"dead": None}
SHAPES = W.SHAPES + (W.NO_PUBLIC,)
SHAPE_IDS = ["n%d" % s[0] for s in W.SHAPES] + ["n128_no_public"]


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
    raw = b"".join((v % Q * R % Q).to_bytes(32, "little") for v in values)
    return np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4).copy()


def le_bytes(values):
    return np.frombuffer(b"".join((v % Q).to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(-1, 32).copy()


@functools.lru_cache(maxsize=None)
def shapes_at(log_n):
    return W.id_shapes(1 << log_n)


@functools.lru_cache(maxsize=None)
def selectors_at(log_n):
    """five selector columns drawn from a pool of 61 scalars (0, 1 and q - 1 among them) -> (Montgomery columns, canonical-byte columns)"""
    rnd = random.Random(log_n)
    pool = [0, 1, Q - 1] + [rnd.randrange(Q) for _ in range(58)]
    pm, pb = mont(pool), le_bytes(pool)
    pick = np.random.RandomState(log_n).randint(0, len(pool), size=(5, 1 << log_n))
    return [np.ascontiguousarray(pm[pick[k]]) for k in range(5)], [np.ascontiguousarray(pb[pick[k]]) for k in range(5)]


def to_le(columns):
    """Montgomery columns -> canonical bytes through the host conversion of the library (bp_fr_convert, no GPU)"""
    out = []
    for c in columns:
        o = np.zeros((len(c), 32), dtype=np.uint8)
        assert bp.load().bp_fr_convert(c.ctypes.data, len(c), bp.FR_MONT, bp.FR_BYTES_LE, o.ctypes.data) == 0
        out.append(o)
    return out


def load(log_n, ids, mode, n_public=0):
    sel_m, sel_b = selectors_at(log_n)
    if mode == "bytes_host":
        return call(bp.Circuit.from_wires, sel_b, ids, n_public, fmt=bp.FR_BYTES_LE)
    if mode == "mont_device":
        import torch
        t = [torch.from_numpy(s.view(np.int64)).cuda() for s in sel_m]
        w = torch.from_numpy(np.ascontiguousarray(ids).view(np.int32)).cuda()
        torch.cuda.synchronize()
        return call(bp.Circuit.from_wires, t, w, n_public)
    return call(bp.Circuit.from_wires, sel_m, ids, n_public)


@pytest.mark.parametrize("mode", ["mont_host", "bytes_host", "mont_device"])
@pytest.mark.parametrize("log_n", [3, 6, 10, 12, 16])
def test_columns_equal_make_s_polynomials_and_the_inputs(log_n, mode):
    sel_m, sel_b = selectors_at(log_n)
    for name, (ids, _) in shapes_at(log_n).items():
        want = bp.make_s_polynomials(ids)
        circuit = load(log_n, ids, mode)
        try:
            got = call(circuit.columns)
            for k, col in enumerate(("s1", "s2", "s3")):
                assert got[col].tobytes() == want[k].tobytes(), (name, col)
            for k, col in enumerate(W.SELECTORS):
                assert got[col].tobytes() == sel_m[k].tobytes(), (name, col)
            if name in ("all_zero", "edge_ids_4"):                # the other export format, and a partial export
                got = call(circuit.columns, bp.FR_BYTES_LE)
                for k, col in enumerate(W.SELECTORS):
                    assert got[col].tobytes() == sel_b[k].tobytes(), (name, col)
                assert [got[c].tobytes() for c in ("s1", "s2", "s3")] == [x.tobytes() for x in to_le(want)], name
                only = call(circuit.columns, bp.FR_MONT, ("qc", "s2"))
                assert sorted(only) == ["qc", "s2"] and only["s2"].tobytes() == want[1].tobytes() and only["qc"].tobytes() == sel_m[4].tobytes()
        finally:
            call(circuit.free)


@pytest.mark.parametrize("log_n", [3, 6, 10, 12])
def test_cell_map_needs_no_decode_and_is_the_row_major_cycles(log_n):
    """check_sigma: all zero and a decode time of exactly 0.  The cell map itself, through the copy check: a witness that numbers its
    cells violates every cell whose predecessor is another cell, the lowest of them first, and a witness of one value per id none."""
    n = 1 << log_n
    zeros = [np.zeros((n, 4), dtype=np.uint64) for _ in range(5)]
    by_cell = [mont([3 * r + col + 1 for r in range(n)]) for col in range(3)]
    for name, (ids, _) in shapes_at(log_n).items():
        circuit = call(bp.Circuit.from_wires, zeros, ids)
        try:
            assert call(circuit.check_sigma) == bp.SigmaReport(0, None, 0, None), name
            assert call(circuit.check_stats)["decode_ms"] == 0, name
            target = W.expected_target(ids)
            moved = [u for u in range(3 * n) if target[u] != u]
            rep = call(circuit.check_witness, *by_cell)
            assert call(circuit.check_stats)["decode_ms"] == 0, name
            assert rep.copy_cells == len(moved), name
            if moved:
                u, v = moved[0], target[moved[0]]
                assert rep.first_copy_cell == (u % 3, u // 3) and rep.first_copy_target == (v % 3, v // 3), name
            by_id = [mont([int(ids[r, col]) + 1 for r in range(n)]) for col in range(3)]
            assert call(circuit.check_witness, *by_id).copy_cells == 0, name
        finally:
            call(circuit.free)


def test_a_circuit_loaded_from_columns_still_decodes():
    ids = shapes_at(6)["random_repeats"][0]
    sig = bp.make_s_polynomials(ids)
    circuit = call(bp.Circuit, selectors_at(6)[0] + list(sig))
    try:
        assert call(circuit.check_sigma).ok
        assert call(circuit.check_stats)["decode_ms"] > 0
        with pytest.raises(bp.BpError) as e:
            call(circuit.assign, mont([0, 1, 2]))
        assert e.value.code == -1 and "no wire ids" in str(e.value)
        got = call(circuit.columns)                               # export serves any handle
        assert [got[c].tobytes() for c in ("s1", "s2", "s3")] == [x.tobytes() for x in sig]
    finally:
        call(circuit.free)


class Case:
    """one general-gate circuit by wire ids, its value array and blinders, and the proof bp_prove gives for the expanded columns on a
    circuit loaded from columns: computed once per shape and never changed"""

    def __init__(self, shape):
        self.n = shape[0]
        c = W.general_wire_circuit(*shape)
        self.c, self.ids, self.n_public, self.publics = c, c["ids"], c["n_public"], c["publics"]
        self.sel = [mont(c["sel"][k]) for k in W.SELECTORS]
        self.values = mont(c["values"])
        self.wit = [mont(col) for col in c["cols"]]
        self.pi = mont(c["public_column"])
        self.blinders = [random.Random(2000 + self.n).randrange(1, Q) for _ in range(11)]
        self.tau = 0x7654321 + self.n
        self.setup = call(bp.Setup.generate_srs, self.n + 6, self.tau)
        plain = call(bp.Circuit, self.sel + list(bp.make_s_polynomials(self.ids)))
        try:
            self.want = call(bp.Prover(self.setup, plain).prove_with_blinding, *self.wit, self.pi, self.blinders)
            self.vk = call(plain.commitments, self.setup)
        finally:
            call(plain.free)
        assert len(self.want) == 624

    def load(self, ctx=None):
        return call(bp.Circuit.from_wires, self.sel, self.ids, self.n_public, ctx)


@functools.lru_cache(maxsize=None)
def case(shape):
    return Case(shape)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_assign_equals_the_expanded_columns(shape):
    import torch
    c = case(shape)
    circuit = c.load()
    try:
        for values in (c.values, le_bytes(c.c["values"]), torch.from_numpy(c.values.view(np.int64)).cuda()):
            fmt = bp.FR_BYTES_LE if getattr(values, "dtype", None) == np.uint8 else bp.FR_MONT
            got = call(circuit.assign, values, fmt)
            a, b, cc, pi = got.host()
            assert a.tobytes() == c.wit[0].tobytes() and b.tobytes() == c.wit[1].tobytes() and cc.tobytes() == c.wit[2].tobytes()
            assert pi.tobytes() == c.pi.tobytes()
            assert call(bp.Prover(c.setup, circuit).check, got) == bp.WitnessReport(0, None, 0, None, None)
        bare = call(circuit.assign, c.values, public_input=False)
        assert bare.public_input is None and bare.host()[2].tobytes() == c.wit[2].tobytes()
    finally:
        call(circuit.free)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_prove_assignment_same_bytes_commitments_and_verdict(shape):
    c = case(shape)
    circuit = c.load()
    try:
        prover = bp.Prover(c.setup, circuit)
        assert call(prover.prove_assignment, c.values, c.blinders) == c.want
        assert call(prover.prove_assignment, le_bytes(c.c["values"]), c.blinders, bp.FR_BYTES_LE) == c.want
        assert call(prover.prove_with_blinding, *c.wit, c.pi, c.blinders) == c.want          # bp_prove on a wires handle: unchanged
        assert call(circuit.commitments, c.setup) == c.vk
        verifier = call(bp.Verifier, c.setup, circuit)
        publics = mont(c.publics).reshape(1, -1, 4) if c.publics else None
        assert call(verifier.verify, [c.want], publics) is True
        if c.publics:
            wrong = mont([c.publics[0], c.publics[1] + 1]).reshape(1, -1, 4)
            assert call(verifier.verify, [c.want], wrong) is False
    finally:
        call(circuit.free)


def test_two_member_rehearsal_context_same_bytes():
    c = case(W.SHAPES[1])
    ctx = call(bp.Context, [0, 0])
    try:
        setup = call(bp.Setup.generate_srs, c.n + 6, c.tau, ctx)
        circuit = c.load(ctx)
        assert call(bp.Prover(setup, circuit).prove_assignment, c.values, c.blinders) == c.want
        assert call(circuit.commitments, setup) == c.vk
        a, b, cc, pi = call(circuit.assign, c.values).host()
        assert [a.tobytes(), b.tobytes(), cc.tobytes(), pi.tobytes()] == [x.tobytes() for x in c.wit + [c.pi]]
        call(circuit.free)
    finally:
        ctx.close()


def test_refusals():
    c = case(W.SHAPES[0])
    circuit = c.load()
    try:
        prover = bp.Prover(c.setup, circuit)
        top = len(c.c["values"]) - 1                               # the largest id: the output of the last gate row
        cells = [3 * r + col for r in range(c.n) for col in range(3) if c.ids[r, col] == top]
        for fn in (lambda v: call(circuit.assign, v), lambda v: call(prover.prove_assignment, v, c.blinders)):
            with pytest.raises(bp.BpError) as e:
                fn(c.values[:top])                                 # one short of the largest id
            assert e.value.code == -6 and "cell %d (row %d" % (cells[0], cells[0] // 3) in str(e.value)
        with pytest.raises(bp.BpError) as e:
            call(circuit.assign, le_bytes([0]) | 0xFF, bp.FR_BYTES_LE)
        assert e.value.code == -4
        # one changed value of a variable that is used: gate rows fail, copy constraints cannot
        used = int(c.ids[c.n_public, 0])
        bad = list(c.c["values"])
        bad[used] = (bad[used] + 1) % Q
        cols = [[bad[c.ids[r, j]] for r in range(c.n)] for j in range(3)]
        public = [(-bad[c.ids[r, 0]]) % Q if r < c.n_public else 0 for r in range(c.n)]
        pk = dict(c.c["sel"])
        rows = [r for r in range(c.n) if G.gate_residual(pk, cols, public, r)]
        assert rows                                                # what Python expects of the changed value: these gate rows, nothing else
        with pytest.raises(bp.BpError) as e:
            call(prover.prove_assignment, mont(bad), c.blinders)
        assert e.value.code == -11
        rep = call(prover.check, call(circuit.assign, mont(bad)))
        assert rep == bp.WitnessReport(len(rows), rows[0], 0, None, None)
        assert call(prover.prove_assignment, c.values, c.blinders) == c.want          # and the next proof is unchanged
    finally:
        call(circuit.free)


def test_bad_arguments_on_a_live_context():
    lib, ctx = bp.load(), bp.default_context()
    n = 8
    sel = [np.zeros((n, 4), dtype=np.uint64) for _ in range(5)]
    ptrs = (C.c_void_p * 5)(*[s.ctypes.data for s in sel])
    ids = np.zeros((n, 3), dtype=np.uint32)
    h = C.c_uint64(77)
    good = [ctx._h, 3, ptrs, ids.ctypes.data, 0, bp.FR_MONT, 0, C.byref(h)]
    for k, bad in ((1, 2), (1, 25), (2, None), (3, None), (4, n + 1), (5, 7), (7, None)):
        args = list(good)
        args[k] = bad
        assert lib.bp_circuit_load_wires(*args) == -1 and h.value == 77, k
    hole = (C.c_void_p * 5)(*[s.ctypes.data for s in sel[:4]] + [None])
    assert lib.bp_circuit_load_wires(ctx._h, 3, hole, ids.ctypes.data, 0, bp.FR_MONT, 0, C.byref(h)) == -1 and h.value == 77
    big = np.full((n, 32), 0xFF, dtype=np.uint8)
    over = (C.c_void_p * 5)(*[big.ctypes.data] * 5)
    assert lib.bp_circuit_load_wires(ctx._h, 3, over, ids.ctypes.data, 0, bp.FR_BYTES_LE, 0, C.byref(h)) == -4 and h.value == 77
    cols = (C.c_void_p * 8)()
    assert lib.bp_circuit_export_columns(ctx._h, 0xDEAD, bp.FR_MONT, cols) == -1
    assert lib.bp_circuit_assign_device(ctx._h, 0xDEAD, sel[0].ctypes.data, n, bp.FR_MONT, 0, 8, 8, 8, None) == -1
    out = np.full(624, 0xA5, dtype=np.uint8)
    assert lib.bp_prove_assignment(ctx._h, 1, 0xDEAD, sel[0].ctypes.data, n, bp.FR_MONT, 0, np.zeros(352, dtype=np.uint8).ctypes.data, out.ctypes.data) == -1
    assert (out == 0xA5).all()


def test_free_and_reload_at_another_size():
    """load, prove, free, load a larger circuit and prove, then the smaller one again, on one context: no workspace keeps a stale size"""
    for shape in (W.SHAPES[0], W.SHAPES[2], W.SHAPES[0]):
        c = case(shape)
        circuit = c.load()
        try:
            assert call(bp.Prover(c.setup, circuit).prove_assignment, c.values, c.blinders) == c.want
            assert call(circuit.assign, c.values).host()[0].tobytes() == c.wit[0].tobytes()
        finally:
            call(circuit.free)

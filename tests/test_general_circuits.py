"""tests/general_circuits.py pinned on the CPU, before any GPU result is compared with a proof of its circuits: the circuits are
satisfied row by row and cycle by cycle in Python integers, every selector column (qc included) is alive, the copy cycles have the
shapes the prover's permutation argument must handle, and the CPU oracle's restatement of src/prover.rs proves them -- and notices a
witness that only the qc term contradicts."""
import random

import pytest

from tests import general_circuits as G
from tests import prover_rounds as PR

Q = G.Q
ALL_SHAPES = G.SHAPES + (G.NO_PUBLIC,)


@pytest.fixture(scope="module", params=ALL_SHAPES, ids=lambda s: "n%d_pub%d_gates%d" % s[:3])
def made(request):
    n, n_pub, n_gates, seed = request.param
    return (n, n_pub, n_gates) + G.general_circuit(n, n_pub, n_gates, seed)


def test_generator_is_deterministic():
    n, n_pub, n_gates, seed = G.SHAPES[0]
    assert G.general_circuit(n, n_pub, n_gates, seed) == G.general_circuit(n, n_pub, n_gates, seed)
    assert G.general_circuit(n, n_pub, n_gates, seed) != G.general_circuit(n, n_pub, n_gates, seed + 1)


def test_rows_satisfy_their_gates_and_cycles_hold_one_value(made):
    n, n_pub, n_gates, cols, pk, public_column, publics = made
    assert all(len(c) == n for c in cols) and all(len(v) == n for v in pk.values()) and len(public_column) == n
    assert all(0 <= v < Q for c in cols for v in c) and all(0 <= v < Q for col in pk.values() for v in col)
    for i in range(n):
        assert G.gate_residual(pk, cols, public_column, i) == 0, i
    cycles = G.copy_cycles(pk)
    assert sorted(cell for c in cycles for cell in c) == [(col, r) for col in range(3) for r in range(n)]
    for cyc in cycles:
        assert len({cols[col][r] for col, r in cyc}) == 1, cyc
    # the public rows: (x, -, -), ql = 1 alone, PI = -x, x non-zero and of full width (at least one of them above 2^192)
    assert len(publics) == n_pub and public_column[n_pub:] == [0] * (n - n_pub)
    for i, x in enumerate(publics):
        assert x and cols[0][i] == x and public_column[i] == Q - x
        assert [pk[k][i] for k in G.SELECTORS] == [1, 0, 0, 0, 0]
    assert not publics or max(publics) >> 192
    # the rows behind the gates are empty
    assert G.gate_rows(pk) == list(range(n_pub, n_pub + n_gates))
    for i in range(n_pub + n_gates, n):
        assert [pk[k][i] for k in G.SELECTORS] == [0] * 5 and [c[i] for c in cols] == [0] * 3


def test_every_selector_column_is_alive(made):
    n, n_pub, n_gates, cols, pk, public_column, publics = made
    rows = G.gate_rows(pk)
    for k in ("ql", "qr", "qm", "qc"):
        alive = sum(1 for i in rows if pk[k][i])
        print("n = %d: %s non-zero in %d of %d gate rows" % (n, k, alive, n_gates))
        assert 4 * alive >= n_gates, k
        assert any(1 < pk[k][i] < Q - 1 for i in rows), k                        # full-width values, not only 0, 1 and -1
    assert len({pk["qo"][i] for i in rows}) >= 3
    # a constant row: only qc and qo alive, a and b empty, c = -qc / qo used nowhere else
    i = G.constant_row(n_pub, n_gates)
    assert pk["ql"][i] == pk["qr"][i] == pk["qm"][i] == 0 and pk["qc"][i] and pk["qo"][i]
    assert cols[0][i] == cols[1][i] == 0 and cols[2][i] * pk["qo"][i] % Q == Q - pk["qc"][i]
    assert [(2, i)] in G.copy_cycles(pk)
    # witness values 0 and q - 1 (the operands of the first gate row)
    assert cols[0][n_pub] == 0 and cols[1][n_pub] == Q - 1


def test_copy_cycles_have_every_shape(made):
    n, n_pub, n_gates, cols, pk, public_column, publics = made
    cycles = G.named_cycles(pk, G.constant_row(n_pub, n_gates))
    lens = sorted(len(c) for c in cycles)
    assert len(G.copy_cycles(pk)) == len(cycles) + 1                             # one cycle of empty cells
    assert 1 in lens and 2 in lens and lens[-1] >= 3
    assert any({col for col, _ in c} == {0, 1, 2} for c in cycles)               # one variable read as a, as b and written as c
    assert {col for c in cycles if len(c) > 1 for col, _ in c} == {0, 1, 2}
    i, j = G.c_to_b_copy(pk, G.constant_row(n_pub, n_gates))                     # what the GPU test breaks: c of row i is b of row j
    assert i != j and cols[2][i] == cols[1][j]


def test_oracle_proves_a_general_circuit_and_notices_the_constant_row():
    """n = 16 on the oracle backend alone: the proof verifies with the public values and not with others; a witness that is wrong
    only in the constant row (where ql = qr = qm = 0: nothing but qc contradicts it) trips the restatement's r(zeta) == 0"""
    from tests.prover_helpers import decode, g1_only_verify, oracle_srs, proof_challenges, prove_with_blinding, split_proof
    n, n_pub, n_gates, seed = G.SHAPES[0]
    tau = 0x1234567
    cols, pk, public_column, publics = G.general_circuit(n, n_pub, n_gates, seed)
    blinders = [random.Random(5).randrange(1, Q) for _ in range(11)]
    cpu = PR.OracleBackend(oracle_srs(n + 6, tau))
    blob = prove_with_blinding(cpu, n, cols, pk, public_column, blinders, logging=False)[2]
    assert len(blob) == 624
    vk = {k: decode(cpu.commit(cpu.Polynomial(cpu.i_ntt_381(PR.SV(pk[k])), cpu.MONO))) for k in pk}
    assert vk["qc"] is not None and vk["ql"] is not None and vk["qr"] is not None
    assert g1_only_verify(n, tau, *split_proof(blob), proof_challenges(blob), vk, publics)
    assert not g1_only_verify(n, tau, *split_proof(blob), proof_challenges(blob), vk, [publics[0], (publics[1] + 1) % Q])
    i = G.constant_row(n_pub, n_gates)
    bad = [list(c) for c in cols]
    bad[2][i] = (bad[2][i] + 1) % Q
    assert G.gate_residual(pk, bad, public_column, i) == pk["qo"][i]
    with pytest.raises(AssertionError):
        prove_with_blinding(cpu, n, bad, pk, public_column, blinders, logging=False)

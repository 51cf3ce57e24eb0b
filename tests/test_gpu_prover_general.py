"""bp_prove on circuits of GENERAL gates (tests/general_circuits.py: every selector column alive, qc included, public inputs, copy
cycles through all three columns), byte for byte against the CPU oracle's restatement of src/prover.rs.  The other prover tests prove
chained multiplications (ql = qr = qc = 0) at every size above 8, so a qc term dropped in rounds 3 AND 5, or a*ql read from the wrong
column, passes them all; on these circuits such a prover either refuses the witness or gives bytes that differ from the oracle's.
Sizes: N = 4n = 64 is one wave, 512 two workgroups (z(wX) wraps across one), and at n = 1024 one coset of a group's split spans four
workgroups.  The NTTs and MSMs are data-blind and covered at size elsewhere.  tests/test_general_circuits.py pins the circuits and the oracle's handling of them on the CPU."""
import functools
import random

import numpy as np
import pytest

import baby_plonk_rust_amd as bp
from oracle import oracle as O
from tests import general_circuits as G
from tests import prover_rounds as PR
from tests.gpu_common import experiment
from tests.prover_helpers import decode, g1_only_verify, proof_challenges, prove_with_blinding, split_proof

pytestmark = pytest.mark.gpu
Q = G.Q
SHAPE_IDS = ["n%d" % s[0] for s in G.SHAPES]


class Case:
    """one circuit, its witness and blinders, and what the oracle makes of them: computed once per shape and never changed"""

    def __init__(self, shape):
        self.n, self.n_pub, self.n_gates, seed = shape
        self.tau = 0x1234567 + self.n
        self.cols, self.pk, self.public, self.publics = G.general_circuit(*shape)
        self.blinders = [random.Random(1000 + self.n).randrange(1, Q) for _ in range(11)]
        self.wit = [PR.SV(c) for c in self.cols]
        self.pkv = {k: PR.SV(v) for k, v in self.pk.items()}
        self.pi = PR.SV(self.public)
        self.setup = bp.Setup.generate_srs(self.n + 6, self.tau)
        cpu = PR.OracleBackend(O.proj_from_bytes96(self.setup.powers_of_x()))
        cpu.threads = 16
        self.want = prove_with_blinding(cpu, self.n, self.cols, self.pk, self.public, self.blinders, logging=False)[2]
        self.vk96 = {k: cpu.commit(cpu.Polynomial(cpu.i_ntt_381(PR.SV(self.pk[k])), cpu.MONO)) for k in self.pk}
        assert len(self.want) == 624

    def prove(self, ctx=None, tables=True, pi="column"):
        """a fresh setup and circuit on `ctx` (None: the shared default context and this case's setup) -> proof bytes"""
        setup = self.setup if ctx is None and tables else bp.Setup.generate_srs(self.n + 6, self.tau, ctx, tables=tables)
        circuit = bp.Circuit(self.pkv, ctx)
        try:
            return bp.Prover(setup, circuit).prove_with_blinding(*self.wit, self.pi if pi == "column" else pi, self.blinders)
        finally:
            circuit.free()
            if setup is not self.setup and ctx is None:
                setup.ctx.srs_free(setup.handle)


@functools.lru_cache(maxsize=None)
def case(shape):
    return Case(shape)


@pytest.mark.parametrize("shape", G.SHAPES, ids=SHAPE_IDS)
def test_general_gates_proof_and_commitments_equal_the_oracle(shape):
    c = case(shape)
    assert c.prove() == c.want
    circuit = bp.Circuit(c.pkv)
    got = circuit.commitments(c.setup)
    circuit.free()
    assert set(got) == set(c.vk96) and len(got) == 8
    for k in got:
        assert got[k] == c.vk96[k], k
    for k in ("ql", "qr", "qc", "qm", "qo", "s1", "s2", "s3"):
        assert decode(got[k]) is not None, k                      # QL, QR and QC are the identity in every other circuit above n = 8


@pytest.mark.parametrize("shape", G.SHAPES, ids=SHAPE_IDS)
def test_general_gates_proof_verifies_with_its_publics_only(shape):
    c = case(shape)
    blob = c.prove()
    vk = {k: decode(v) for k, v in c.vk96.items()}
    assert g1_only_verify(c.n, c.tau, *split_proof(blob), proof_challenges(blob), vk, c.publics)
    assert not g1_only_verify(c.n, c.tau, *split_proof(blob), proof_challenges(blob), vk, [c.publics[0], (c.publics[1] + 1) % Q])


@pytest.mark.parametrize("shape", G.SHAPES, ids=SHAPE_IDS)
def test_hbm_resident_witness_and_no_tables_same_bytes(shape):
    import torch
    c = case(shape)
    t = [torch.from_numpy(w.view(np.int64)).cuda() for w in c.wit + [c.pi]]
    torch.cuda.synchronize()
    circuit = bp.Circuit(c.pkv)
    assert bp.Prover(c.setup, circuit).prove_device(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), c.blinders) == c.want
    circuit.free()
    assert c.prove(tables=False) == c.want


@pytest.mark.parametrize("members", [2, 4])
@pytest.mark.parametrize("shape", G.SHAPES[:2], ids=SHAPE_IDS[:2])
def test_group_contexts_round3_by_coset_same_bytes(shape, members):
    """two members take two cosets each, four take one each: fr_fold_scale on a non-zero PI (slot 4 of the coset inputs), quotient_coset
    with zshift 1 on general selectors, coset_recombine"""
    c = case(shape)
    ctx = bp.Context([0] * members)
    try:
        assert c.prove(ctx) == c.want
    finally:
        ctx.close()


@experiment
@pytest.mark.parametrize("shape", G.SHAPES[:2], ids=SHAPE_IDS[:2])
def test_round3_by_coset_on_one_device_same_bytes(shape, monkeypatch):
    c = case(shape)
    monkeypatch.setenv("BP_PROVE_COSET_ONE", "1")                 # read when the circuit is loaded
    assert c.prove() == c.want


def test_no_public_inputs_none_and_zero_column_same_bytes():
    """the pi_zero path (PI's transforms skipped) with general gates"""
    c = case(G.NO_PUBLIC)
    assert c.publics == [] and c.public == [0] * c.n
    assert c.prove(pi=None) == c.want
    assert c.prove() == c.want                                    # the explicit all-zero column: the general path
    vk = {k: decode(v) for k, v in c.vk96.items()}
    assert g1_only_verify(c.n, c.tau, *split_proof(c.want), proof_challenges(c.want), vk, [])


@pytest.mark.parametrize("shape", G.SHAPES, ids=SHAPE_IDS)
def test_unsatisfying_witnesses_are_refused_and_leave_the_next_proof_unchanged(shape):
    c = case(shape)
    circuit = bp.Circuit(c.pkv)
    prover = bp.Prover(c.setup, circuit)
    residuals = lambda cols, public: [i for i in range(c.n) if G.gate_residual(c.pk, cols, public, i)]
    cycles_hold = lambda cols: all(len({cols[col][r] for col, r in cyc}) == 1 for cyc in G.copy_cycles(c.pk))

    def refused(cols, public, what):
        with pytest.raises(bp.BpError) as e:
            prover.prove_with_blinding(*[PR.SV(x) for x in cols], PR.SV(public), c.blinders)
        assert e.value.code == -11, what
        assert prover.prove_with_blinding(*c.wit, c.pi, c.blinders) == c.want, what

    assert prover.prove_with_blinding(*c.wit, c.pi, c.blinders) == c.want
    # the constant row (-, -, c), ql = qr = qm = 0, c in no copy cycle: only the qc term contradicts c + 1
    i = G.constant_row(c.n_pub, c.n_gates)
    bad = [list(x) for x in c.cols]
    bad[2][i] = (bad[2][i] + 1) % Q
    assert residuals(bad, c.public) == [i] and cycles_hold(bad)
    refused(bad, c.public, "constant row")
    # an addition row (qm = 0) whose output is used nowhere else
    alone = {cyc[0] for cyc in G.copy_cycles(c.pk) if len(cyc) == 1}
    i = [r for r in G.gate_rows(c.pk) if c.pk["qm"][r] == 0 and (c.pk["ql"][r] or c.pk["qr"][r]) and (2, r) in alone][0]
    bad = [list(x) for x in c.cols]
    bad[2][i] = (bad[2][i] + 1) % Q
    assert residuals(bad, c.public) == [i] and cycles_hold(bad)
    refused(bad, c.public, "addition row")
    # a wrong public value: PI no longer cancels x in row 1
    public = list(c.public)
    public[1] = (public[1] + 1) % Q
    assert residuals(c.cols, public) == [1]
    refused(c.cols, public, "public value")
    # a copy constraint between column C of row i and column B of row j: b_j changes and c_j follows, so every gate still holds
    i, j = G.c_to_b_copy(c.pk, G.constant_row(c.n_pub, c.n_gates))
    bad = [list(x) for x in c.cols]
    bad[1][j] = (bad[1][j] + 1) % Q
    a, b = bad[0][j], bad[1][j]
    bad[2][j] = -(c.pk["ql"][j] * a + c.pk["qr"][j] * b + c.pk["qm"][j] * a * b + c.pk["qc"][j]) * pow(c.pk["qo"][j], Q - 2, Q) % Q
    assert residuals(bad, c.public) == [] and not cycles_hold(bad) and bad[2][i] != bad[1][j]
    refused(bad, c.public, "copy constraint")
    circuit.free()

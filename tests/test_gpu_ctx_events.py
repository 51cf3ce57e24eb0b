"""-m gpu: a context's HIP events have one owner (ev_get, csrc/ctx.hpp): every entry-point family that times its stages or orders
two streams takes its events from the context by name, and bp_destroy releases them in one loop.  What that can break is state
ACROSS calls -- a second call of a family on the same context, a set that grows between calls (the G1 transform's pass events),
two contexts alive at once, a context that is closed and made again -- so each case here makes one call of every family at the
smallest shapes the families' own tests use and compares with what those tests expect (their helpers are imported, not restated).
The seam events of bp_msm_g1_projective144 need 2^17 points: tests/test_gpu_multi_device.py runs them."""
import ctypes as C
import math
import random

import numpy as np
import pytest

import baby_plonk_rust_amd as bp
from baby_plonk_rust_amd import BASIS_LAGRANGE, FR_BYTES_LE
from oracle import oracle as O
from tests import kzg_model as K
from tests import pairing_cases as PC
from tests import prover_rounds as PR
from tests import test_gpu_pairing as TP
from tests import test_gpu_srs_lagrange as TL
from tests import test_gpu_verify as TV
from tests import test_gpu_verify_segments as TS
from tests import test_gpu_witness_check as TW
from tests import verify_model as V
from tests.gpu_common import EXPERIMENT
from tests.test_gpu_prover_rounds import prove_with_blinding, synthetic_circuit

pytestmark = pytest.mark.gpu
Q = TV.Q
LOG_N, N = 3, 8
TAU = 0x1234567


class Inputs:
    """the arguments of one call of every family and what Python expects of it: computed once, never changed"""

    def __init__(self):
        rnd = random.Random(0xE7E)
        # bp_verify_reduce of 2 proofs (challenges derived on the device) and bp_verify_reduce_segments of 3 proofs by 2 (given ones)
        self.recs = TV.dlog_records(rnd, 3)
        self.raw = TV.blob(self.recs)
        self.vk_dl = [rnd.randrange(1, Q) for _ in range(8)]
        self.vk = TS.vk_of(self.vk_dl)
        self.weights = [rnd.randrange(Q) for _ in range(3)]
        derived = [V.challenges_of(self.raw[624 * j: 624 * j + 624])[0] for j in range(2)]
        self.chal = [[rnd.randrange(Q) for _ in range(6)] for _ in range(3)]
        self.want = {"verify": TV.want192(N, self.recs[:2], self.vk_dl, None, self.weights[:2], derived),
                     "segments": TS.want_pairs(self.recs, self.vk_dl, None, self.weights, self.chal, 2)}
        # bp_pairing_check of one pair
        self.pairs, truth = PC.mixed_pairs(1, 201)
        host = bp.pairing_check(self.pairs, TP.X2, host=True, gt=True)
        assert host[0] == truth
        self.want["pairing"] = host
        # bp_srs_lagrange at 2^3 and 2^5, an opening on the first and the reduce of that one claim: A = W, B = C - y G + z W
        self.f, self.z = [rnd.randrange(Q) for _ in range(N)], rnd.randrange(Q)
        (y,), q_tau = K.open_lagrange([self.f], self.z, 0, TAU)
        self.want["lagrange8"], self.want["lagrange32"] = (TL.closed_form([pow(TAU, j, Q) for j in range(n)]) for n in (8, 32))
        self.want["open"] = ([y], K.point96(q_tau))
        self.want["kzg_reduce"] = (K.point96(q_tau), K.point96(K.barycentric(self.f, TAU) - y + self.z * q_tau))
        # one circuit of 2^3 rows for bp_prove and bp_circuit_check_witness; the checked witness has b_0 changed
        self.cols, self.pk, self.public = synthetic_circuit(N, 3)
        self.blinders = [random.Random(1).randrange(1, Q) for _ in range(11)]
        self.bad = [list(c) for c in self.cols]
        self.bad[1][0] = (self.bad[1][0] + 1) % Q
        self.want["check"] = TW.expected(self.pk, self.bad, self.public, TW.permutation(self.pk))
        assert self.want["check"] == bp.WitnessReport(1, 0, 0, None, None)
        self.want["proof"] = None                                  # the oracle's proof needs the SRS points: filled by the first Session


@pytest.fixture(scope="module")
def inputs():
    return Inputs()


def pass_count_and_times(ctx):
    """the library's hook bpx_srs_lagrange_pass_ms: the HIP-event time of every pass of the last G1 transform on ctx"""
    ms, k = (C.c_float * 32)(), C.c_uint32()
    fn = ctx._lib.bpx_srs_lagrange_pass_ms
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32)]
    ctx.check(fn(ctx._h, ms, 32, C.byref(k)), "bpx_srs_lagrange_pass_ms")
    return [float(ms[i]) for i in range(k.value)]


class Session:
    """what one context keeps between rounds of calls: the setups, the circuit (so that a second round meets its cached sigma) and the prover"""

    def __init__(self, ctx, inp):
        self.ctx, self.inp = ctx, inp
        self.powers = bp.Setup.generate_srs(32, TAU, ctx, tables=False)
        self.setup = bp.Setup.generate_srs(N + 6, TAU, ctx)
        self.circuit = bp.Circuit({k: PR.SV(v) for k, v in inp.pk.items()}, ctx)
        self.prover = bp.Prover(self.setup, self.circuit)
        if inp.want["proof"] is None:
            cpu = PR.OracleBackend(O.proj_from_bytes96(self.setup.powers_of_x()))
            inp.want["proof"] = prove_with_blinding(cpu, N, inp.cols, inp.pk, inp.public, inp.blinders, logging=False)[2]

    def round(self, monkeypatch=None):
        """one call of every family -> (results by name, every stage time the calls left behind)"""
        ctx, inp, got, times = self.ctx, self.inp, {}, []
        scal = TV.scal
        got["verify"] = ctx.verify_reduce(LOG_N, inp.vk, inp.raw[:624 * 2], None, scal(inp.weights[:2], (2,)), fmt=FR_BYTES_LE)
        times += ctx.verify_stats().values()
        got["segments"] = ctx.verify_reduce_segments(LOG_N, inp.vk, inp.raw, None, scal(inp.weights, (3,)), TS.chal_arr(inp.chal), FR_BYTES_LE, 2)
        times += list(ctx.verify_stats().values()) + list(ctx.verify_segments_stats().values())
        got["pairing"] = ctx.pairing_check(inp.pairs, TP.X2, gt=True)
        times += ctx.pairing_stats().values()
        lag8 = self.powers.lagrange(8, tables=False)
        passes8 = pass_count_and_times(ctx)
        lag32 = self.powers.lagrange(32, tables=False)             # more passes than the call before: the pass-event set grows
        passes32 = pass_count_and_times(ctx)
        assert (len(passes8), len(passes32)) == (3, 5)
        times += passes8 + passes32
        got["lagrange8"], got["lagrange32"] = lag8.powers_of_x(), lag32.powers_of_x()
        poly = bp.DevicePolynomial(bp.scalars_from_ints(inp.f), BASIS_LAGRANGE, ctx)
        ys, w = lag8.open(poly, bp.scalar_from_int(inp.z))
        got["open"] = (bp.scalars_to_ints(ys), w)
        got["kzg_reduce"] = lag8.opening_pairing_inputs(bp.Opening(lag8.commit_device(poly), bp.scalar_from_int(inp.z), ys, None, w))
        times += ctx.kzg_stats().values()
        ctx.srs_free(lag32.handle)
        ctx.srs_free(lag8.handle)
        got["check"] = self.circuit.check_witness(*[TW.mont(c) for c in inp.bad], TW.mont(inp.public))
        self.check_stats = self.circuit.check_stats()
        times += self.check_stats.values()
        wit = [PR.SV(c) for c in inp.cols]
        got["proof"] = self.prover.prove_with_blinding(*wit, None, inp.blinders)       # the side events (round 3's transforms beside round 2)
        if EXPERIMENT and monkeypatch is not None:                 # the seam events: round 1 staged column by column (the default from 2^18 gates)
            monkeypatch.setenv("BP_PROVE_STAGED", "1")
            assert self.prover.prove_with_blinding(*wit, None, inp.blinders) == got["proof"]
            monkeypatch.delenv("BP_PROVE_STAGED")
        st = self.prover.last_stats()
        times += st["round_ms"] + [st["total_ms"]]
        return got, times


def test_every_timed_family_twice_on_one_context(inputs, monkeypatch):
    ctx = bp.Context(0)
    try:
        s = Session(ctx, inputs)
        first, times = s.round(monkeypatch)
        assert s.check_stats["decode_ms"] > 0                      # the first check of the circuit decodes sigma
        second, times2 = s.round(monkeypatch)
        assert s.check_stats["decode_ms"] == 0                     # the second finds it cached
        for name, want in inputs.want.items():
            assert first[name] == want, name
            assert second[name] == first[name], name
        assert sorted(first) == sorted(inputs.want)
        assert all(math.isfinite(v) and v >= 0 for v in times + times2), (times, times2)
    finally:
        ctx.close()


def test_two_contexts_keep_their_own_events_and_stats(inputs):
    a, b = bp.Context(0), bp.Context(0)
    try:
        got = a.verify_reduce(LOG_N, inputs.vk, inputs.raw[:624 * 2], None, TV.scal(inputs.weights[:2], (2,)), fmt=FR_BYTES_LE)
        assert got == inputs.want["verify"] and any(v > 0 for v in a.verify_stats().values())
        assert all(v == 0 for v in b.verify_stats().values())
        assert b.pairing_check(inputs.pairs, TP.X2, gt=True) == inputs.want["pairing"] and any(v > 0 for v in b.pairing_stats().values())
        assert all(v == 0 for v in a.pairing_stats().values())
    finally:
        a.close()
        b.close()


def device_mib_in_use():
    import torch
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return (total - free) / 2**20


def test_create_use_close_three_times(inputs):
    """every cycle makes one call of each family; after the first (the process's one-time allocations are in by then) the device
    memory in use comes back to within 8 MiB, the bound of tools/leak_check.py"""
    used = []
    for _ in range(3):
        ctx = bp.Context(0)
        try:
            got, _ = Session(ctx, inputs).round()
        finally:
            ctx.close()
        assert got == inputs.want
        used.append(device_mib_in_use())
    assert all(abs(u - used[0]) < 8 for u in used[1:]), used

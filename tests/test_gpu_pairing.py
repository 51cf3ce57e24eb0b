"""-m gpu: bp_pairing_check -- one pairing check per GPU lane -- against bp_pairing_check_host byte for byte and against the known
setup secret (tests/pairing_cases.py); its rejections; and the verdict methods of Verifier on real proofs.  Shapes: one lane, one
wave and one more (63, 64, 65), more than two workgroups (130), and the empty call.  Every lane's Gt image is compared, invalid
lanes included: a verdict alone lets wrong arithmetic pass wherever the answer is "no"."""
import ctypes as C
import math
import random

import numpy as np
import pytest

import baby_plonk_rust_amd as bp
from baby_plonk_rust_amd import FR_BYTES_LE
from tests import bigint_model as M
from tests import pairing_cases as PC
from tests import tower_model as T
from tests import verify_model as V

pytestmark = pytest.mark.gpu
P, Q = PC.P, PC.Q
SIZE_MAX = C.c_size_t(-1).value
X2 = T.g2_enc192(T.g2_mul(PC.G2, PC.TAU))


@pytest.fixture(scope="module")
def ctx():
    c = bp.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 130])
def test_device_verdicts_and_images_are_the_hosts(ctx, n):
    pairs, truth = PC.mixed_pairs(n, 200 + n)
    want_v, want_gt = bp.pairing_check(pairs, X2, host=True, gt=True)
    assert want_v == truth
    got_v, got_gt = ctx.pairing_check(pairs, X2, gt=True)
    assert got_v == truth
    assert got_gt == want_gt                                        # every lane, the invalid ones included
    assert ctx.pairing_check(pairs, X2) == truth                    # without the images
    stats = ctx.pairing_stats()
    assert len(stats) == 3 and all(math.isfinite(v) and v >= 0 for v in stats.values())
    if n == 0:
        assert all(v == 0 for v in stats.values())


def test_device_gives_the_generator_literal_and_a_two_shard_context_the_same_bytes(ctx):
    verdicts, images = ctx.pairing_check([(PC.FX96[1], PC.ID96)], T.g2_enc192(PC.G2), gt=True)
    assert verdicts == [False] and images == [PC.GT_GENERATOR]
    pairs, truth = PC.mixed_pairs(65, 3)
    one = ctx.pairing_check(pairs, X2, gt=True)
    many = bp.Context([0, 0])
    try:
        assert many.pairing_check(pairs, X2, gt=True) == one and one[0] == truth
    finally:
        many.close()
    assert bp.pairing_check(pairs, X2, ctx=ctx, checks=3) == truth  # with both subgroup tests


def raw_check(ctx, x2, pairs, n, checks):
    lib = bp.load()
    x2a, buf = np.frombuffer(x2, dtype=np.uint8).copy(), np.frombuffer(pairs, dtype=np.uint8).copy()
    verdicts, gt, bad = np.full(max(n, 1), 0xA5, dtype=np.uint8), np.full(max(n, 1) * 576, 0xA5, dtype=np.uint8), C.c_size_t(12345)
    rc = lib.bp_pairing_check(ctx._h, x2a.ctypes.data, buf.ctypes.data, n, checks, verdicts.ctypes.data, gt.ctypes.data, C.byref(bad))
    return rc, bad.value, verdicts, gt


def test_device_rejections_name_the_lowest_pair_and_write_nothing(ctx):
    """bytes only: nothing here can fault a kernel"""
    n = 70
    good, truth = PC.mixed_pairs(n, 9)
    clean = ctx.pairing_check(good, X2, gt=True)
    faults = {"non-canonical x": (P.to_bytes(48, "big") + bytes(48), 0), "sort flag": (bytes([0x20 | PC.FX96[2][0]]) + PC.FX96[2][1:], 0),
              "identity with coordinates": (bytes([0x40]) + bytes(94) + b"\x01", 0), "off the curve": (PC.off_curve96(), 0),
              "outside the subgroup": (PC.outside_subgroup96(), 1)}
    for name, (rec, checks) in faults.items():
        for slots in ((2 * 66 + 1, 2 * 5), (2 * 64, 2 * 69 + 1)):        # two indices, in either order of A / B and of wave
            bad = bytearray(good)
            for s in slots:
                bad[96 * s: 96 * s + 96] = rec
            rc, first, verdicts, gt = raw_check(ctx, X2, bytes(bad), n, checks)
            assert rc == -3 and first == min(slots) // 2, name
            assert (verdicts == 0xA5).all() and (gt == 0xA5).all(), name
            with pytest.raises(bp.BpError) as e:
                ctx.pairing_check(bytes(bad), X2, checks=checks)
            assert e.value.code == -3 and e.value.index == min(slots) // 2 and ("pair %d" % (min(slots) // 2)) in str(e.value)
        assert ctx.pairing_check(good, X2, gt=True) == clean and clean[0] == truth      # no stale status
    _, off = T.g2_find_points()
    for x2, code in ((T.g2_enc192(off), -3), (PC.ID192, -1)):
        rc, first, verdicts, gt = raw_check(ctx, x2, good, n, 0)
        assert rc == code and first == SIZE_MAX and (verdicts == 0xA5).all() and (gt == 0xA5).all()


# ---- real proofs: the recipe of tests/test_gpu_verify_segments.py ----------------------------------------------------------------
def scal(values, shape):
    return np.frombuffer(V.le32(values), dtype=np.uint8).reshape(*shape, 32).copy()


def dec96(b):
    return None if b[0] & 0x40 else (int.from_bytes(b[:48], "big"), int.from_bytes(b[48:], "big"))


@pytest.fixture(scope="module")
def real(ctx):
    from tests import prover_rounds as PR
    n, tau = 64, 0x1234567
    pk, witness = V.public_circuit(n, 40)
    setup = bp.Setup.generate_srs(n + 6, tau, ctx)
    circuit = bp.Circuit({k: PR.SV(v) for k, v in pk.items()}, ctx)
    prover, rnd = bp.Prover(setup, circuit), random.Random(65)
    proofs, publics = [], []
    for _ in range(32):
        cols, public, column = witness(rnd)
        proofs.append(prover.prove_with_blinding(PR.SV(cols[0]), PR.SV(cols[1]), PR.SV(cols[2]), PR.SV(column), [rnd.randrange(1, Q) for _ in range(11)]))
        publics.append(public)
    return tau, setup, bp.Verifier(setup, circuit), proofs, publics


def test_verdicts_on_real_proofs(real):
    tau, setup, verifier, proofs, publics = real
    assert setup.x_2 == T.g2_enc192(T.g2_mul(PC.G2, tau)) and verifier.x_2 == setup.x_2
    m, rnd = len(proofs), random.Random(2)
    weights = scal([rnd.getrandbits(128) for _ in range(m)], (m,))
    pub = lambda rows: scal([x for row in rows for x in row], (len(rows), 3))

    def decide(a96, b96):                                           # the pairing equation with the known tau: tau A == B
        A, B = dec96(a96), dec96(b96)
        return A is not None and M.ec_mul(tau, A) == B
    assert verifier.verify(proofs, pub(publics), weights, fmt=FR_BYTES_LE) is True
    assert verifier.verify_each(proofs, pub(publics), fmt=FR_BYTES_LE) == [True] * m
    assert verifier.locate_invalid(proofs, pub(publics), weights, fmt=FR_BYTES_LE) == []
    bad = list(proofs)
    for j in (0, 17, 31):                                           # a flipped bit in an evaluation
        t = bytearray(bad[j])
        t[432 + 32 * (j % 6)] ^= 1
        bad[j] = bytes(t)
    wrong = [row[:] for row in publics]
    wrong[5][1] = (wrong[5][1] + 1) % Q                             # and a wrong public input
    assert verifier.verify(bad, pub(wrong), weights, fmt=FR_BYTES_LE) is False
    assert verifier.verify_each(bad, pub(wrong), fmt=FR_BYTES_LE) == [j not in (0, 5, 17, 31) for j in range(m)]
    located = verifier.locate_invalid(bad, pub(wrong), weights, fmt=FR_BYTES_LE)
    assert located == verifier.locate_invalid(bad, pub(wrong), weights, decide, FR_BYTES_LE) == [0, 5, 17, 31]
    # a setup without x_2 cannot give verdicts
    bare = bp.Verifier.__new__(bp.Verifier)
    bare.__dict__.update(verifier.__dict__)
    bare.x_2 = None
    for call in (lambda: bare.verify(proofs, pub(publics), weights, fmt=FR_BYTES_LE), lambda: bare.verify_each(proofs, pub(publics), fmt=FR_BYTES_LE),
                 lambda: bare.locate_invalid(proofs, pub(publics), weights, fmt=FR_BYTES_LE)):
        with pytest.raises(bp.BpError):
            call()

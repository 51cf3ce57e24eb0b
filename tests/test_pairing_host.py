"""CPU checks of the host pairing entry points of the C ABI (no GPU, no context): bp_g2_mul_generator, bp_pairing_gt_host and
bp_pairing_check_host against tests/tower_model.py, the reference's Gt::generator() literal, bilinearity, and pairs whose verdict
is known from the setup secret (tests/pairing_cases.py).  These are the host halves of Verifier.verify and
Verifier.locate_invalid(decide=None), which need a context to run whole (tests/test_gpu_pairing.py)."""
import ctypes as C
import random

import numpy as np
import pytest

import baby_plonk_rust_amd as bp
from tests import bigint_model as M
from tests import pairing_cases as PC
from tests import tower_model as T

P, Q = PC.P, PC.Q
SIZE_MAX = C.c_size_t(-1).value
X2 = T.g2_enc192(T.g2_mul(PC.G2, PC.TAU))


def test_g2_mul_generator_against_the_model():
    rnd = random.Random(4)
    for k in [1, 2, 3, Q - 1, PC.TAU] + [rnd.randrange(Q) for _ in range(3)]:
        enc = bp.g2_mul_generator(k)
        assert enc == T.g2_enc192(T.g2_mul(PC.G2, k)), k
        assert T.g2_on_curve(T.g2_dec192(enc))
    assert bp.g2_mul_generator(1) == T.g2_enc192(PC.G2)
    assert bp.g2_mul_generator(0) == PC.ID192
    for k in (Q, Q + 1, (1 << 256) - 1):
        with pytest.raises(bp.BpError) as e:
            bp.g2_mul_generator(k)
        assert e.value.code == -4
    lib = bp.load()
    out = np.zeros(192, dtype=np.uint8)
    assert lib.bp_g2_mul_generator(None, out.ctypes.data) == -1 and lib.bp_g2_mul_generator(out.ctypes.data, None) == -1


def test_g2_output_round_trips_and_bad_x2_is_refused():
    """the decoder of bp_pairing_check_host takes what bp_g2_mul_generator writes; a point off the curve, and a curve point
    outside the subgroup under checks & 2, are BP_ERR_BAD_POINT -- both found with the model"""
    pairs, truth = PC.mixed_pairs(2, 1)
    assert bp.pairing_check(pairs, bp.g2_mul_generator(PC.TAU), host=True) == truth
    outside, off = T.g2_find_points()
    for x2, checks, code in ((T.g2_enc192(off), 0, -3), (T.g2_enc192(outside), 2, -3), (PC.ID192, 0, -1), (bytes([0x80]) + X2[1:], 0, -3),
                             (P.to_bytes(48, "big") + X2[48:], 0, -3)):
        with pytest.raises(bp.BpError) as e:
            bp.pairing_check(pairs, x2, host=True, checks=checks)
        assert e.value.code == code and e.value.index is None
    assert len(bp.pairing_check(pairs, T.g2_enc192(outside), host=True)) == 2           # on the curve: accepted without checks & 2
    assert bp.pairing_check(pairs, X2, host=True, checks=3) == truth


def test_pairing_of_the_generators_is_the_references_literal():
    assert bp.pairing_gt(M.enc96(M.ec_mul(1)), T.g2_enc192(PC.G2)) == PC.GT_GENERATOR


def test_pairing_is_bilinear_and_identities_give_one():
    g1, g2 = PC.FX96[1], T.g2_enc192(PC.G2)
    for a, b in ((2, 3), (5, 7), (31, 29), (999, Q - 1)):
        ab = a * b % Q
        want = bp.pairing_gt(M.enc96(M.ec_mul(ab)), g2)
        assert bp.pairing_gt(PC.FX96[a], T.g2_enc192(T.g2_mul(PC.G2, b))) == want
        assert bp.pairing_gt(g1, T.g2_enc192(T.g2_mul(PC.G2, ab))) == want
        assert want not in (PC.GT_ONE, PC.GT_GENERATOR)
    # e(G1, G2)^6 from the model's Fp12 product of the literal: the image is the field element, not an opaque blob
    gt = PC.f12_from(PC.GT_GENERATOR)
    assert bp.pairing_gt(PC.FX96[2], T.g2_enc192(T.g2_mul(PC.G2, 3))) == PC.f12_bytes(T.f12_pow(gt, 6))
    assert bp.pairing_gt(PC.ID96, g2) == PC.GT_ONE and bp.pairing_gt(g1, PC.ID192) == PC.GT_ONE and bp.pairing_gt(PC.ID96, PC.ID192) == PC.GT_ONE
    _, off = T.g2_find_points()
    for p, q in ((PC.off_curve96(), g2), (g1, T.g2_enc192(off)), (bytes([0xC0]) + bytes(95), g2)):
        with pytest.raises(bp.BpError) as e:
            bp.pairing_gt(p, q)
        assert e.value.code == -3


@pytest.mark.parametrize("n", [0, 1, 2, 5, 17])
def test_check_host_verdicts_follow_the_known_secret(n):
    pairs, truth = PC.mixed_pairs(n, 100 + n)
    assert bp.pairing_check(pairs, X2, host=True) == truth
    verdicts, images = bp.pairing_check(pairs, X2, host=True, gt=True)
    assert verdicts == truth and len(images) == n
    for ok, image in zip(truth, images):
        assert (image == PC.GT_ONE) == ok


def test_check_host_with_a_large_secret_and_the_three_identity_cases():
    tau = 0x1234567
    x2 = bp.g2_mul_generator(tau)
    A = PC.FX96[9]
    pairs = [(A, M.enc96(M.ec_mul(9 * tau % Q))), (A, M.enc96(M.ec_mul((9 * tau + 1) % Q))), (PC.ID96, PC.ID96), (PC.ID96, A), (A, PC.ID96)]
    assert bp.pairing_check(pairs, x2, host=True) == [True, False, True, False, False]
    # (G1, identity) under x_2 = G2 leaves the single term pairing(G1, G2): the generator literal
    verdicts, images = bp.pairing_check([(PC.FX96[1], PC.ID96)], T.g2_enc192(PC.G2), host=True, gt=True)
    assert verdicts == [False] and images == [PC.GT_GENERATOR]
    # an invalid pair's image is pairing(G1, G2)^(tau a - b), from the model
    (_, (image,)) = bp.pairing_check([(PC.FX96[3], PC.FX96[PC.TAU * 3 - 2])], X2, host=True, gt=True)
    assert image == PC.f12_bytes(T.f12_pow(PC.f12_from(PC.GT_GENERATOR), 2))


def raw_check(x2, pairs, n, checks, want_gt=True):
    lib = bp.load()
    x2a = np.frombuffer(x2, dtype=np.uint8).copy()
    buf = np.frombuffer(pairs, dtype=np.uint8).copy()
    verdicts, gt, bad = np.full(max(n, 1), 0xA5, dtype=np.uint8), np.full(max(n, 1) * 576, 0xA5, dtype=np.uint8), C.c_size_t(12345)
    rc = lib.bp_pairing_check_host(x2a.ctypes.data, buf.ctypes.data, n, checks, verdicts.ctypes.data, gt.ctypes.data if want_gt else None, C.byref(bad))
    return rc, bad.value, verdicts, gt


def test_check_host_rejections_name_the_lowest_pair_and_write_nothing():
    n = 9
    good, truth = PC.mixed_pairs(n, 5)
    non_canonical = P.to_bytes(48, "big") + bytes(48)
    faults = {"non-canonical x": (non_canonical, 0), "non-canonical y": (bytes(48) + (P + 5).to_bytes(48, "big"), 0),
              "compression flag": (bytes([0x80 | PC.FX96[2][0]]) + PC.FX96[2][1:], 0), "sort flag": (bytes([0x20 | PC.FX96[2][0]]) + PC.FX96[2][1:], 0),
              "identity with coordinates": (bytes([0x40]) + bytes(94) + b"\x01", 0), "zero coordinates without the flag": (bytes(96), 0),
              "off the curve": (PC.off_curve96(), 0), "outside the subgroup": (PC.outside_subgroup96(), 1)}
    for name, (rec, checks) in faults.items():
        for slots in ((2 * 3,), (2 * 6 + 1, 2 * 4), (2 * 8 + 1, 2 * 8, 2 * 7 + 1)):                 # A of pair 3; B of 6 and A of 4; three at 8, 8, 7
            bad = bytearray(good)
            for s in slots:
                bad[96 * s: 96 * s + 96] = rec
            rc, first, verdicts, gt = raw_check(X2, bytes(bad), n, checks)
            assert rc == -3 and first == min(slots) // 2, name
            assert (verdicts == 0xA5).all() and (gt == 0xA5).all(), name
    # the subgroup test is asked for, not implied
    bad = bytearray(good)
    bad[0:96] = PC.outside_subgroup96()
    rc, first, verdicts, _ = raw_check(X2, bytes(bad), n, 0)
    assert rc == 0 and first == SIZE_MAX and [bool(v) for v in verdicts[1:]] == truth[1:]
    # x_2: rejected before any pair is looked at, nothing written, no pair named
    _, off = T.g2_find_points()
    for x2, code in ((T.g2_enc192(off), -3), (PC.ID192, -1)):
        rc, first, verdicts, gt = raw_check(x2, bytes(bad), n, 1)
        assert rc == code and first == SIZE_MAX and (verdicts == 0xA5).all() and (gt == 0xA5).all()
    # a clean call: first_bad = SIZE_MAX, the verdicts, and gt only where asked
    rc, first, verdicts, gt = raw_check(X2, good, n, 1, want_gt=False)
    assert rc == 0 and first == SIZE_MAX and [bool(v) for v in verdicts] == truth and (gt == 0xA5).all()
    # n = 0 writes nothing; null pointers are arguments errors
    rc, first, verdicts, gt = raw_check(X2, good, 0, 0)
    assert rc == 0 and (verdicts == 0xA5).all() and (gt == 0xA5).all()
    lib = bp.load()
    x2a, buf, v, fb = np.frombuffer(X2, dtype=np.uint8).copy(), np.frombuffer(good, dtype=np.uint8).copy(), np.zeros(n, dtype=np.uint8), C.c_size_t()
    assert lib.bp_pairing_check_host(None, buf.ctypes.data, n, 0, v.ctypes.data, None, C.byref(fb)) == -1
    assert lib.bp_pairing_check_host(x2a.ctypes.data, None, n, 0, v.ctypes.data, None, C.byref(fb)) == -1
    assert lib.bp_pairing_check_host(x2a.ctypes.data, buf.ctypes.data, n, 0, None, None, C.byref(fb)) == -1
    assert lib.bp_pairing_check_host(x2a.ctypes.data, buf.ctypes.data, n, 0, v.ctypes.data, None, None) == -1
    assert lib.bp_pairing_check(None, x2a.ctypes.data, buf.ctypes.data, n, 0, v.ctypes.data, None, C.byref(fb)) == -1
    assert lib.bp_pairing_last_stats(None, None) == -1
    assert lib.bp_pairing_gt_host(None, None, None) == -1

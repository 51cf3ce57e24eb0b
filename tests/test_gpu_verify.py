"""-m gpu: bp_verify_reduce (Verifier::verify, src/verifier.rs:80-192, for a batch and up to the two pairings) against Python
integers.  A and B are linear in the points, so records whose points have KNOWN discrete logs (the crate's fixture holds i G for
i < 1000) make the expected outputs one scalar multiplication each, for any batch size (tests/verify_model.py); such records are
not valid proofs and need not be -- the pairing decides validity, not this call.  Real proofs (bp_prove) are checked with the
known tau: the pairing equation e(A, [tau]_2) == e(B, [1]_2) is tau A == B."""
import ctypes as C
import json
import os
import random
import time

import numpy as np
import pytest

import baby_plonk_rust_amd as bp
from baby_plonk_rust_amd import FR_BYTES_LE, FR_MONT
from tests import bigint_model as M
from tests import verify_model as V

pytestmark = pytest.mark.gpu
Q, P = M.Q, M.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_MAX = 2**64 - 1
FX = V.fixture_points()


@pytest.fixture(scope="module")
def ctx():
    c = bp.Context(0)
    yield c
    c.close()


def scal(values, shape):
    """canonical little-endian bytes as the uint8 array Context.verify_reduce takes with fmt=FR_BYTES_LE"""
    return np.frombuffer(V.le32(values), dtype=np.uint8).reshape(*shape, 32).copy()


def dlog_records(rnd, m, identity_every=0):
    """m records of fixture points (known discrete logs) and random canonical evaluations"""
    recs = []
    for j in range(m):
        dl = [rnd.randrange(1, 1000) for _ in range(9)]
        if identity_every and j % identity_every == 1:
            dl[rnd.randrange(9)] = 0                             # record 0 of the fixture: the identity, 0xc0 then zeros
        recs.append((dl, [rnd.randrange(Q) for _ in range(6)]))
    return recs


def blob(recs):
    return b"".join(b"".join(FX[k] for k in dl) + V.le32(ev) for dl, ev in recs)


def vk_of(dlogs):
    return b"".join(M.enc96(M.ec_mul(k)) for k in dlogs)


def want192(n, recs, vk_dl, publics, weights, chal):
    a, b = V.reduce_dlogs(n, recs, vk_dl, publics, weights, chal)
    return M.enc96(M.ec_mul(a)), M.enc96(M.ec_mul(b))


@pytest.fixture(scope="module")
def derived():
    """512 dlog records and their challenges from the Python twin of the transcript (the slow part: once per module)"""
    rnd = random.Random(0xB47C4)
    recs = dlog_records(rnd, 512, identity_every=37)
    raw = blob(recs)
    chal, draws = [], []
    for j in range(512):
        ch, d = V.challenges_of(raw[624 * j: 624 * j + 624])
        chal.append(ch)
        draws += d
    assert max(draws) >= 8, "the batch must reach deep into the rejection sampling of transcript.rs:70-82"
    return recs, raw, chal


@pytest.mark.parametrize("n,n_public", [(8, 0), (8, 1), (8, 3), (64, 0), (64, 3), (64, 64)])
def test_exact_bytes_with_challenges_derived_on_the_device(ctx, derived, n, n_public):
    recs, raw, chal = derived
    rnd = random.Random(n * 1000 + n_public)
    m = len(recs)
    vk_dl = [rnd.randrange(1, Q) for _ in range(8)]
    publics = [[rnd.randrange(Q) for _ in range(n_public)] for _ in range(m)]
    weights = [rnd.randrange(Q) for _ in range(m)]
    got = ctx.verify_reduce(n.bit_length() - 1, vk_of(vk_dl), raw, scal([x for row in publics for x in row], (m, n_public)) if n_public else None,
                            scal(weights, (m,)), fmt=FR_BYTES_LE)
    assert got == want192(n, recs, vk_dl, publics, weights, chal)
    # the host entry point derives the same challenges (one implementation, two compilations)
    assert [bp.scalars_to_ints(row) for row in bp.plonk_challenges(raw[:624 * 4])] == chal[:4]
    if (n, n_public) == (8, 3):                                 # the same through Montgomery limbs
        got_m = ctx.verify_reduce(3, vk_of(vk_dl), raw, np.stack([bp.scalars_from_ints(row) for row in publics]), bp.scalars_from_ints(weights))
        assert got_m == got
    # one proof, no weights: the two arguments of verifier.rs:187-191 themselves
    for j in (0, 1, m - 1):
        one = ctx.verify_reduce(n.bit_length() - 1, vk_of(vk_dl), raw[624 * j: 624 * j + 624],
                                scal(publics[j], (1, n_public)) if n_public else None, None, fmt=FR_BYTES_LE)
        assert one == want192(n, [recs[j]], vk_dl, [publics[j]], None, [chal[j]])


def test_exact_bytes_with_given_challenges_on_the_roots_and_edge_weights(ctx):
    n, n_public, m = 8, 3, 4096
    rnd = random.Random(0x5EED5)
    om = M.omega(n)
    recs = dlog_records(rnd, m, identity_every=101)
    chal = [[rnd.randrange(Q) for _ in range(6)] for _ in range(m)]
    weights = [rnd.randrange(Q) for _ in range(m)]
    publics = [[rnd.randrange(Q) for _ in range(n_public)] for _ in range(m)]
    for j, zeta in ((5, 1), (6, pow(om, 2, Q)), (7, pow(om, 5, Q)), (m - 1, pow(om, 7, Q)), (2000, 1), (2001, pow(om, 1, Q))):
        chal[j][3] = zeta                                        # zeta^n = 1: inside the public rows (w^0, w^1, w^2) and outside
    chal[9] = [0] * 6                                            # all-zero challenges are scalars like any other here
    weights[10], weights[11], weights[12], weights[5] = 0, 1, Q - 1, Q - 1
    recs[300], chal[300], publics[300] = recs[299], chal[299], publics[299]       # one record twice, different weights
    assert weights[299] != weights[300]
    vk_dl = [rnd.randrange(Q) for _ in range(8)]
    vk_dl[4] = 0                                                 # a vk commitment may be the identity (QC = 0)
    got = ctx.verify_reduce(3, vk_of(vk_dl), blob(recs), scal([x for row in publics for x in row], (m, n_public)), scal(weights, (m,)),
                            scal([x for row in chal for x in row], (m, 6)), fmt=FR_BYTES_LE)
    assert got == want192(n, recs, vk_dl, publics, weights, chal)
    # all weights zero: both outputs are the identity, encoded like bp_msm_g1 encodes it
    ident = bytes([0x40]) + bytes(95)
    assert ctx.verify_reduce(3, vk_of(vk_dl), blob(recs[:64]), None, scal([0] * 64, (64,)), scal([x for row in chal[:64] for x in row], (64, 6)),
                             fmt=FR_BYTES_LE) == (ident, ident)
    assert ctx.verify_reduce(3, vk_of(vk_dl), b"", None, None) == (ident, ident)                       # m = 0
    # n = 64 with the public inputs reaching the root zeta sits on
    n, m2 = 64, 96
    om = M.omega(n)
    publics = [[rnd.randrange(Q) for _ in range(40)] for _ in range(m2)]
    chal2 = [row[:] for row in chal[:m2]]
    for j, e in ((0, 0), (1, 39), (2, 40), (3, 63)):
        chal2[j][3] = pow(om, e, Q)
    got = ctx.verify_reduce(6, vk_of(vk_dl), blob(recs[:m2]), scal([x for row in publics for x in row], (m2, 40)), scal(weights[:m2], (m2,)),
                            scal([x for row in chal2 for x in row], (m2, 6)), fmt=FR_BYTES_LE)
    assert got == want192(n, recs[:m2], vk_dl, publics, weights[:m2], chal2)


# ---- real proofs -------------------------------------------------------------------------------------------------------------
def dec96(b):
    return None if b[0] & 0x40 else (int.from_bytes(b[:48], "big"), int.from_bytes(b[48:], "big"))


@pytest.fixture(scope="module")
def real(ctx):
    from tests import prover_rounds as PR
    n, tau = 64, 0x1234567
    pk, witness = V.public_circuit(n, 40)
    setup = bp.Setup.generate_srs(n + 6, tau, ctx)
    circuit = bp.Circuit({k: PR.SV(v) for k, v in pk.items()}, ctx)
    prover, rnd = bp.Prover(setup, circuit), random.Random(64)
    proofs, publics = [], []
    for _ in range(64):
        cols, public, column = witness(rnd)
        blinders = [rnd.randrange(1, Q) for _ in range(11)]
        proofs.append(prover.prove_with_blinding(PR.SV(cols[0]), PR.SV(cols[1]), PR.SV(cols[2]), PR.SV(column), blinders))
        publics.append(public)
    assert len(set(proofs)) == 64
    return tau, bp.Verifier(setup, circuit), proofs, publics


def accepts(tau, sides):
    A, B = dec96(sides[0]), dec96(sides[1])
    return A is not None and M.ec_mul(tau, A) == B


def test_real_proofs_accept_and_every_tampering_rejects(real):
    tau, verifier, proofs, publics = real
    rnd = random.Random(1)
    m = len(proofs)
    weights = scal([rnd.getrandbits(128) for _ in range(m)], (m,))
    pub = lambda rows: scal([x for row in rows for x in row], (len(rows), 3))
    assert accepts(tau, verifier.pairing_inputs(proofs, pub(publics), weights, fmt=FR_BYTES_LE))
    assert accepts(tau, verifier.pairing_inputs(proofs, np.stack([bp.scalars_from_ints(r) for r in publics]),
                                                bp.scalars_from_ints([rnd.getrandbits(128) for _ in range(m)])))
    for j in (0, m // 2, m - 1):                                 # a flipped bit in an evaluation
        bad = list(proofs)
        t = bytearray(bad[j])
        t[432 + 32 * (j % 6)] ^= 1
        bad[j] = bytes(t)
        assert not accepts(tau, verifier.pairing_inputs(bad, pub(publics), weights, fmt=FR_BYTES_LE)), j
    wrong = [row[:] for row in publics]
    wrong[17][1] = (wrong[17][1] + 1) % Q                        # a wrong public input
    assert not accepts(tau, verifier.pairing_inputs(proofs, pub(wrong), weights, fmt=FR_BYTES_LE))
    swapped = list(proofs)
    swapped[3], swapped[40] = swapped[40], swapped[3]            # two proofs swapped against their public-input rows
    assert not accepts(tau, verifier.pairing_inputs(swapped, pub(publics), weights, fmt=FR_BYTES_LE))
    for j in range(0, m, 8):                                     # singly, weight 1
        assert accepts(tau, verifier.pairing_inputs(proofs[j], pub([publics[j]]), None, fmt=FR_BYTES_LE)), j
    assert not accepts(tau, verifier.pairing_inputs(proofs[0], pub([publics[1]]), None, fmt=FR_BYTES_LE))


def test_toy_proof_gives_the_two_sides_of_the_reference_verifier(ctx):
    from tests import prover_rounds as PR
    from tests.test_gpu_prover_rounds import g1_only_verify
    toy = json.load(open(os.path.join(ROOT, "tests", "golden", "path_vectors.json")))["toy_proof"]
    n, tau = 8, 101
    cols = {k: [int.from_bytes(bytes.fromhex(h), "little") for h in v] for k, v in toy["columns"].items()}
    setup = bp.Setup.generate_srs(n + 6, tau, ctx)
    verifier = bp.Verifier(setup, bp.Circuit({k: PR.SV(v) for k, v in cols.items()}, ctx))
    proof = bytes.fromhex(toy["proof624"])
    A, B = verifier.pairing_inputs(proof, scal([80], (1, 1)), None, fmt=FR_BYTES_LE)
    assert accepts(tau, (A, B))
    pts = {f: M.dec48(proof[48 * k: 48 * k + 48]) for k, f in enumerate(V.POINT_FIELDS)}
    ev = [int.from_bytes(proof[432 + 32 * k: 464 + 32 * k], "little") for k in range(6)]
    ch, _ = V.challenges_of(proof)
    vk = {k: dec96(v) for k, v in verifier.commitments.items()}
    wa, wb = V.pairing_sides(n, pts, ev, ch, vk, [80])
    assert (A, B) == (M.enc96(wa), M.enc96(wb))
    assert g1_only_verify(n, tau, pts, dict(zip(V.EVAL_FIELDS, ev)), dict(zip(("beta", "gamma", "alpha", "zeta", "nu", "mu"), ch)), vk, [80])
    assert not accepts(tau, verifier.pairing_inputs(proof, scal([81], (1, 1)), None, fmt=FR_BYTES_LE))
    # Context.verify_reduce takes the same key as its 768 bytes or as the dict of Circuit.commitments
    assert verifier.ctx.verify_reduce(3, verifier.commitments, proof, scal([80], (1, 1)), fmt=FR_BYTES_LE) == (A, B)


# ---- rejections --------------------------------------------------------------------------------------------------------------
def off_curve48():
    x = 5
    while pow((x**3 + 4) % P, (P - 1) // 2, P) == 1:
        x += 1
    return bytes([0x80 | (x >> 376)]) + (x & ((1 << 376) - 1)).to_bytes(47, "big")


def outside_subgroup48(rnd):
    """on the curve, outside the prime-order subgroup (the cofactor is ~2^126: a random curve point almost never is inside)"""
    while True:
        x = rnd.randrange(P)
        rhs = (x**3 + 4) % P
        y = pow(rhs, (P + 1) // 4, P)
        if y * y % P == rhs:
            acc, pt, k = None, (x, y), Q
            while k:                                             # [q] P without reducing the scalar
                if k & 1:
                    acc = M.ec_add(acc, pt)
                pt = M.ec_add(pt, pt)
                k >>= 1
            if acc is not None:
                return M.enc48((x, y))


def test_rejections_name_the_lowest_proof_and_leave_the_output_alone(ctx):
    rnd = random.Random(77)
    m = 24
    recs = dlog_records(rnd, m)
    good = blob(recs)
    vk, weights = vk_of([rnd.randrange(1, Q) for _ in range(8)]), scal([rnd.randrange(Q) for _ in range(m)], (m,))
    cleared = bytes([FX[5][0] & 0x7F]) + FX[5][1:]

    def with_faults(faults):
        t = bytearray(good)
        for proof, kind, field, value in faults:
            off = 624 * proof + (48 * field if kind == "point" else 432 + 32 * field)
            t[off: off + len(value)] = value
        return bytes(t)
    q_le = Q.to_bytes(32, "little")
    cases = [
        ([(3, "point", 5, off_curve48()), (9, "point", 0, outside_subgroup48(rnd))], -3, 3, "not on the curve"),
        ([(2, "point", 8, outside_subgroup48(rnd)), (7, "point", 0, cleared)], -3, 2, "subgroup"),   # lowest PROOF, not lowest column
        ([(4, "point", 1, cleared), (11, "eval", 2, q_le)], -3, 4, "encoding"),
        ([(1, "eval", 5, q_le), (6, "point", 3, off_curve48())], -4, 1, "z_omega_bar"),
        ([(8, "eval", 0, q_le), (8, "point", 7, cleared)], -3, 8, "w_zeta_1"),                          # a tie reports the point
        ([(m - 1, "eval", 3, (2**256 - 1).to_bytes(32, "little"))], -4, m - 1, "s1_bar"),
    ]
    lib = ctx._lib
    good2 = ctx.verify_reduce(3, vk, good[:624 * 2], None, weights[:2], fmt=FR_BYTES_LE)
    for faults, code, index, text in cases:
        with pytest.raises(bp.BpError) as e:
            ctx.verify_reduce(3, vk, with_faults(faults), None, weights, fmt=FR_BYTES_LE)
        assert e.value.code == code and e.value.index == index and text in str(e.value), (faults, str(e.value))
        assert ("proof %d" % index) in str(e.value)
        # the boundary itself: first_bad and an untouched out192
        buf = np.frombuffer(with_faults(faults), dtype=np.uint8).copy()
        vkb, out, bad = np.frombuffer(vk, dtype=np.uint8).copy(), np.full(192, 0xA5, dtype=np.uint8), C.c_size_t(0)
        rc = lib.bp_verify_reduce(ctx._h, 3, vkb.ctypes.data, buf.ctypes.data, m, None, 0, weights.ctypes.data, None, FR_BYTES_LE,
                                  out.ctypes.data, C.byref(bad))
        assert rc == code and bad.value == index and (out == 0xA5).all()
        # no stale status: the next valid call on the same context succeeds
        assert ctx.verify_reduce(3, vk, good[:624 * 2], None, weights[:2], fmt=FR_BYTES_LE) == good2
    # non-canonical weights / public inputs / challenges, and the argument rules
    w_bad = weights.copy()
    w_bad[13] = np.frombuffer(q_le, dtype=np.uint8)
    with pytest.raises(bp.BpError) as e:
        ctx.verify_reduce(3, vk, good, None, w_bad, fmt=FR_BYTES_LE)
    assert e.value.code == -4 and e.value.index == 13
    with pytest.raises(bp.BpError) as e:
        ctx.verify_reduce(3, vk, good, None, None)               # no weights for more than one proof
    assert e.value.code == -1
    with pytest.raises(bp.BpError) as e:
        ctx.verify_reduce(3, vk, good, scal([1] * (m * 9), (m, 9)), weights, fmt=FR_BYTES_LE)          # n_public > n
    assert e.value.code == -6
    with pytest.raises(bp.BpError) as e:
        ctx.verify_reduce(2, vk, good, None, weights, fmt=FR_BYTES_LE)
    assert e.value.code == -1
    with pytest.raises(bp.BpError) as e:
        ctx.verify_reduce(3, bytes([0x80]) + vk[1:], good, None, weights, fmt=FR_BYTES_LE)              # a vk point with a flag it may not carry
    assert e.value.code == -3
    assert ctx.verify_reduce(3, vk, good[:624 * 2], None, weights[:2], fmt=FR_BYTES_LE) == good2


def test_vk_record_of_zero_coordinates_is_the_identity_only_with_the_infinity_flag(ctx):
    """a verifier-key commitment of 96 zero bytes is canonical and carries no flag, so it is the pair (0, 0), which is not on the curve:
    BP_ERR_BAD_POINT, as G1Affine::from_uncompressed refuses it; the same slot as 0x40 and zeros is the identity and is taken"""
    rnd = random.Random(78)
    good = blob(dlog_records(rnd, 2))
    vk, weights = vk_of([rnd.randrange(1, Q) for _ in range(8)]), scal([rnd.randrange(Q) for _ in range(2)], (2,))
    for k in (0, 3, 7):
        with pytest.raises(bp.BpError) as e:
            ctx.verify_reduce(3, vk[:96 * k] + bytes(96) + vk[96 * (k + 1):], good, None, weights, fmt=FR_BYTES_LE)
        assert e.value.code == -3 and ("commitment %d rejected" % k) in str(e.value)
        a, b = ctx.verify_reduce(3, vk[:96 * k] + bytes([0x40]) + bytes(95) + vk[96 * (k + 1):], good, None, weights, fmt=FR_BYTES_LE)
        assert len(a) == 96 and len(b) == 96
    a, b = ctx.verify_reduce(3, vk, good, None, weights, fmt=FR_BYTES_LE)          # no stale error: the valid key still goes through
    assert len(a) == 96 and len(b) == 96


def test_stage_times_are_sane_and_group_contexts_use_their_primary(ctx):
    rnd = random.Random(3)
    m = 2048
    recs = dlog_records(rnd, m)
    raw, vk_dl = blob(recs), [rnd.randrange(1, Q) for _ in range(8)]
    weights = [rnd.randrange(Q) for _ in range(m)]
    chal = [[rnd.randrange(Q) for _ in range(6)] for _ in range(m)]
    w, c = scal(weights, (m,)), scal([x for row in chal for x in row], (m, 6))
    want = want192(8, recs, vk_dl, None, weights, chal)
    ctx.verify_reduce(3, vk_of(vk_dl), raw, None, w, c, fmt=FR_BYTES_LE)                              # first call: workspaces grow
    t0 = time.perf_counter()
    got = ctx.verify_reduce(3, vk_of(vk_dl), raw, None, w, None, fmt=FR_BYTES_LE)
    wall_ms = (time.perf_counter() - t0) * 1e3
    st = ctx.verify_stats()
    assert len(st) == 5 and all(np.isfinite(v) and v >= 0 for v in st.values()), st
    assert st["transcript_ms"] > 0 and st["decode_check_ms"] > 0 and st["msm_ms"] > 0 and sum(st.values()) < wall_ms, (st, wall_ms)
    assert got != want                                            # derived challenges differ from the random ones given below
    assert ctx.verify_reduce(3, vk_of(vk_dl), raw, None, w, c, fmt=FR_BYTES_LE) == want
    assert ctx.verify_stats()["transcript_ms"] < st["transcript_ms"]                                  # given challenges: no transcript kernel
    many = bp.Context([0, 0])                                     # a group context runs the batch on its primary member
    try:
        assert many.verify_reduce(3, vk_of(vk_dl), raw, None, w, c, fmt=FR_BYTES_LE) == want
    finally:
        many.close()

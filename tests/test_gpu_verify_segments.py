"""-m gpu: bp_verify_reduce_segments -- one pair (A_s, B_s) per segment of a batch -- against Python integers.  As in
tests/test_gpu_verify.py, records whose points have KNOWN discrete logs (the crate's fixture holds i G for i < 1000) make every
expected pair two scalar multiplications of G (tests/verify_model.py reduce_dlogs on the segment's slice).  The shapes are the
smallest at which the kernels can go wrong: one lane, one wave and one more (m = 63, 64, 65), more than one workgroup of the
per-proof kernels (130), segments that end inside a wave, short last segments, and tree levels that straddle segment ends
(segment = 7).  Real proofs (bp_prove) and the known tau decide validity for the bisection of Verifier.locate_invalid."""
import ctypes as C
import functools
import math
import random

import numpy as np
import pytest

import baby_plonk_rust_amd as bp
from baby_plonk_rust_amd import FR_BYTES_LE
from tests import bigint_model as M
from tests import verify_model as V

pytestmark = pytest.mark.gpu
Q, P = M.Q, M.P
X2 = 0xD201000000010000 ** 2
FX = V.fixture_points()
IDENT = bytes([0x40]) + bytes(95)
N, LOG_N = 8, 3


@pytest.fixture(scope="module")
def ctx():
    c = bp.Context(0)
    yield c
    c.close()


def scal(values, shape):
    """canonical little-endian bytes as the uint8 array Context.verify_reduce takes with fmt=FR_BYTES_LE"""
    return np.frombuffer(V.le32(values), dtype=np.uint8).reshape(*shape, 32).copy()


def dlog_records(rnd, m, identity_every=0):
    """m records of fixture points (known discrete logs) and random canonical evaluations; record 0 of the fixture is the identity"""
    recs = []
    for j in range(m):
        dl = [rnd.randrange(1, 1000) for _ in range(9)]
        if identity_every and j % identity_every == 1:
            dl[rnd.randrange(9)] = 0
        recs.append((dl, [rnd.randrange(Q) for _ in range(6)]))
    return recs


def blob(recs):
    return b"".join(b"".join(FX[k] for k in dl) + V.le32(ev) for dl, ev in recs)


@functools.lru_cache(maxsize=None)
def g_windows():
    """[d 16^i G for d < 16] for i < 64, affine, from tests/bigint_model.py's addition: the fixed-base table of g_times"""
    rows, base = [], (M.GX, M.GY)
    for _ in range(64):
        row = [None, base]
        for _ in range(14):
            row.append(M.ec_add(row[-1], base))
        rows.append(row)
        base = M.ec_add(row[15], base)
    return rows


@functools.lru_cache(maxsize=None)
def g_times(k):
    """enc96(k G) in Python integers: 64 table entries summed in Jacobian coordinates (one inversion at the end instead of one per
    addition, as M.ec_mul pays: the expected pairs of a parametrisation are hundreds of such products).  The entries are
    d 16^i G with distinct i, so a partial sum never meets its next term or its negative: only the empty sum is special."""
    k %= Q
    acc = None
    for i in range(64):
        d = (k >> (4 * i)) & 15
        if not d:
            continue
        x2, y2 = g_windows()[i][d]
        if acc is None:
            acc = (x2, y2, 1)
            continue
        x1, y1, z1 = acc
        z1z1 = z1 * z1 % P
        u2, s2 = x2 * z1z1 % P, y2 * z1 * z1z1 % P
        h, r = (u2 - x1) % P, (s2 - y1) % P
        assert h, "a partial sum met its next term"
        hh = h * h % P
        hhh, v = h * hh % P, x1 * hh % P
        x3 = (r * r - hhh - 2 * v) % P
        acc = (x3, (r * (v - x3) - y1 * hhh) % P, z1 * h % P)
    if acc is None:
        return M.enc96(None)
    zi = pow(acc[2], P - 2, P)
    return M.enc96((acc[0] * zi * zi % P, acc[1] * zi * zi * zi % P))


def test_the_fixed_base_helper_is_the_models_multiplication():
    rnd = random.Random(9)
    for k in [0, 1, 2, 15, 16, 17, Q - 1, X2] + [rnd.randrange(Q) for _ in range(3)]:
        assert g_times(k) == M.enc96(M.ec_mul(k)), k


def vk_of(dlogs):
    return b"".join(g_times(k) for k in dlogs)


def want_pairs(recs, vk_dl, publics, weights, chal, segment):
    """reduce_dlogs on every segment's slice of the records, public-input rows, weights and challenges"""
    m, out = len(recs), []
    for lo in range(0, m, segment):
        hi = min(m, lo + segment)
        a, b = V.reduce_dlogs(N, recs[lo:hi], vk_dl, publics[lo:hi] if publics else None, weights[lo:hi] if weights is not None else None, chal[lo:hi])
        out.append((g_times(a), g_times(b)))
    return out


def pub_arr(publics, n_public):
    return scal([x for row in publics for x in row], (len(publics), n_public)) if n_public else None


def chal_arr(chal):
    return scal([x for row in chal for x in row], (len(chal), 6))


@pytest.fixture(scope="module")
def batch():
    """130 dlog records with identity points among them, given challenges, weights, and two sets of public inputs; every smaller
    batch of the exact-bytes test is a prefix"""
    rnd = random.Random(0x5E6)
    recs = dlog_records(rnd, 130, identity_every=9)
    chal = [[rnd.randrange(Q) for _ in range(6)] for _ in range(130)]
    weights = [rnd.randrange(Q) for _ in range(130)]
    publics = {0: None, 3: [[rnd.randrange(Q) for _ in range(3)] for _ in range(130)]}
    vk_dl = [rnd.randrange(1, Q) for _ in range(8)]
    return recs, blob(recs), chal, weights, publics, vk_dl


def segments_of(m):
    return sorted({1, 2, 7, 64, m, m + 5})


@pytest.mark.parametrize("n_public", [0, 3])
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 130])
def test_exact_bytes_against_the_model_with_given_challenges(ctx, batch, m, n_public):
    recs, raw, chal, weights, publics, vk_dl = batch
    pub = publics[n_public][:m] if n_public else None
    for segment in segments_of(m):
        got = ctx.verify_reduce_segments(LOG_N, vk_of(vk_dl), raw[:624 * m], pub_arr(pub, n_public) if n_public else None, scal(weights[:m], (m,)),
                                         chal_arr(chal[:m]), FR_BYTES_LE, segment)
        want = want_pairs(recs[:m], vk_dl, pub, weights[:m], chal[:m], segment)
        assert len(got) == len(want) == -(-m // segment)
        assert got == want, (m, segment, [s for s in range(len(want)) if got[s] != want[s]])
    # segment = 1 without weights: the two arguments of verifier.rs:187-191 of every proof
    got = ctx.verify_reduce_segments(LOG_N, vk_of(vk_dl), raw[:624 * m], pub_arr(pub, n_public) if n_public else None, None, chal_arr(chal[:m]), FR_BYTES_LE, 1)
    assert got == want_pairs(recs[:m], vk_dl, pub, None, chal[:m], 1)


def test_exact_bytes_with_challenges_derived_on_the_device(ctx):
    m, n_public = 9, 3                                          # the transcript kernel is stage 1, shared with bp_verify_reduce and tested there
    rnd = random.Random(0xD3)
    recs = dlog_records(rnd, m, identity_every=4)
    raw = blob(recs)
    chal = [V.challenges_of(raw[624 * j: 624 * j + 624])[0] for j in range(m)]
    weights = [rnd.randrange(Q) for _ in range(m)]
    publics = [[rnd.randrange(Q) for _ in range(n_public)] for _ in range(m)]
    vk_dl = [rnd.randrange(1, Q) for _ in range(8)]
    for segment in segments_of(m):
        got = ctx.verify_reduce_segments(LOG_N, vk_of(vk_dl), raw, pub_arr(publics, n_public), scal(weights, (m,)), None, FR_BYTES_LE, segment)
        assert got == want_pairs(recs, vk_dl, publics, weights, chal, segment), segment
    got_m = ctx.verify_reduce_segments(LOG_N, vk_of(vk_dl), raw, np.stack([bp.scalars_from_ints(row) for row in publics]), bp.scalars_from_ints(weights),
                                       segment=7)                # the same through Montgomery limbs
    assert got_m == want_pairs(recs, vk_dl, publics, weights, chal, 7)


def test_edge_scalars_weights_and_an_identity_in_the_key(ctx):
    """the scalar of a_1 is rho nu, of w_zeta_1 rho zeta in B and rho in A, of A's second term rho mu: given challenges put every
    edge of the split k = k1 x^2 + k0 there -- once with rho = 1, once behind a random weight"""
    rnd = random.Random(0xED6E)
    edges = [0, 1, X2 - 1, X2, X2 + 1, Q - 1]
    m = 3 * len(edges) + 8
    recs = dlog_records(rnd, m, identity_every=5)
    chal = [[rnd.randrange(Q) for _ in range(6)] for _ in range(m)]
    weights = [rnd.randrange(1, Q) for _ in range(m)]
    for i, v in enumerate(edges):
        j = i                                                    # rho = 1: nu = zeta = mu = v
        weights[j] = 1
        chal[j][3] = chal[j][4] = chal[j][5] = v
        j = len(edges) + i                                       # rho random: rho nu = rho zeta = rho mu = v
        u = v * pow(weights[j], Q - 2, Q) % Q
        chal[j][3] = chal[j][4] = chal[j][5] = u
        assert weights[j] * u % Q == v
        j = 2 * len(edges) + i                                   # the weight itself on the edge: the scalar of W_zeta in A
        weights[j] = v
    base = 3 * len(edges)
    weights[base: base + 4] = [0, 0, 0, 0]                       # a whole segment (of 4) with weight 0, 1 and q - 1 around it
    weights[base + 4], weights[base + 5] = 1, Q - 1
    assert base % 2 == 0
    vk_dl = [rnd.randrange(1, Q) for _ in range(8)]
    vk_dl[4] = 0                                                 # a vk commitment may be the identity (QC = 0)
    publics = [[rnd.randrange(Q) for _ in range(3)] for _ in range(m)]
    for segment in (1, 2, 4, m):
        got = ctx.verify_reduce_segments(LOG_N, vk_of(vk_dl), blob(recs), pub_arr(publics, 3), scal(weights, (m,)), chal_arr(chal), FR_BYTES_LE, segment)
        assert got == want_pairs(recs, vk_dl, publics, weights, chal, segment), segment
        if segment == 1:
            assert got[base] == got[base + 3] == (IDENT, IDENT)
        if segment == 2:
            assert got[base // 2] == got[base // 2 + 1] == (IDENT, IDENT)
    # the four weightless proofs as one whole segment
    got = ctx.verify_reduce_segments(LOG_N, vk_of(vk_dl), blob(recs[base:]), pub_arr(publics[base:], 3), scal(weights[base:], (m - base,)),
                                     chal_arr(chal[base:]), FR_BYTES_LE, 4)
    assert got[0] == (IDENT, IDENT) and got[1] != (IDENT, IDENT)
    assert got == want_pairs(recs[base:], vk_dl, publics[base:], weights[base:], chal[base:], 4)
    assert ctx.verify_reduce_segments(LOG_N, vk_of(vk_dl), b"", None, None, None, FR_BYTES_LE, 3) == []      # m = 0


def curve_point_outside_the_subgroup(rnd):
    """96 bytes of a point on the curve and outside the prime-order subgroup (the cofactor is ~2^126: a random curve point is)"""
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
                return M.enc96((x, y))


@pytest.mark.parametrize("key", ["in_subgroup", "outside_subgroup"])
def test_consistency_with_bp_verify_reduce(ctx, batch, key):
    """every segment pair is bp_verify_reduce of that slice byte for byte; the host sum of the pairs is bp_verify_reduce of the batch
    (for a key inside the subgroup);
    and a segments call in between leaves bp_verify_reduce's own bytes alone.  The verifier key is only checked for the curve, so
    a commitment outside the subgroup is legal input: there the endomorphism is not [x^2] and the shared bases must still agree."""
    recs, raw, chal, weights, publics, vk_dl = batch
    m, rnd = 130, random.Random(5)
    vk = vk_of(vk_dl)
    if key == "outside_subgroup":
        vk = vk[:96 * 2] + curve_point_outside_the_subgroup(rnd) + vk[96 * 3:]
    pub, w, ch = pub_arr(publics[3], 3), scal(weights, (m,)), chal_arr(chal)
    whole = ctx.verify_reduce(LOG_N, vk, raw, pub, w, ch, FR_BYTES_LE)
    if key == "in_subgroup":
        assert [whole] == want_pairs(recs, vk_dl, publics[3], weights, chal, m)
    for segment in (1, 7, 64):
        got = ctx.verify_reduce_segments(LOG_N, vk, raw, pub, w, ch, FR_BYTES_LE, segment)
        assert ctx.verify_reduce(LOG_N, vk, raw, pub, w, ch, FR_BYTES_LE) == whole
        for s, pair in enumerate(got):
            lo, hi = s * segment, min(m, (s + 1) * segment)
            assert pair == ctx.verify_reduce(LOG_N, vk, raw[624 * lo: 624 * hi], pub[lo:hi], w[lo:hi], ch[lo:hi], FR_BYTES_LE), (segment, s)
        if key == "in_subgroup":                                 # (outside it, k -> k P is not additive mod q: the pairs need not add up)
            total = tuple(bp.sum_partials(b"".join(bp.bytes96_to_partial(pair[i]) for pair in got)) for i in (0, 1))
            assert total == whole, segment
    st, split = ctx.verify_stats(), ctx.verify_segments_stats()
    assert len(st) == 5 and len(split) == 3 and all(np.isfinite(v) and v >= 0 for v in list(st.values()) + list(split.values()))
    many = bp.Context([0, 0])                                    # a group context runs the call on its primary member
    try:
        assert many.verify_reduce_segments(LOG_N, vk, raw, pub, w, ch, FR_BYTES_LE, 64)[2] == got[2]
    finally:
        many.close()


def off_curve48():
    x = 5
    while pow((x**3 + 4) % P, (P - 1) // 2, P) == 1:
        x += 1
    return bytes([0x80 | (x >> 376)]) + (x & ((1 << 376) - 1)).to_bytes(47, "big")


def test_rejections_name_the_lowest_proof_and_leave_the_output_alone(ctx):
    """faults are bytes of the records only; nothing here reaches the multiplication kernels"""
    rnd = random.Random(78)
    m = 24
    good = blob(dlog_records(rnd, m))
    vk, weights = vk_of([rnd.randrange(1, Q) for _ in range(8)]), scal([rnd.randrange(Q) for _ in range(m)], (m,))
    cleared = bytes([FX[5][0] & 0x7F]) + FX[5][1:]
    q_le = Q.to_bytes(32, "little")

    def with_faults(faults):
        t = bytearray(good)
        for proof, kind, field, value in faults:
            off = 624 * proof + (48 * field if kind == "point" else 432 + 32 * field)
            t[off: off + len(value)] = value
        return bytes(t)
    cases = [
        ([(4, "point", 1, cleared), (11, "eval", 2, q_le)], -3, 4, "encoding"),
        ([(1, "eval", 5, q_le), (6, "point", 3, off_curve48())], -4, 1, "z_omega_bar"),
        ([(9, "point", 8, off_curve48()), (7, "point", 0, cleared)], -3, 7, "a_1"),            # lowest PROOF, not lowest column
        ([(8, "eval", 0, q_le), (8, "point", 7, cleared)], -3, 8, "w_zeta_1"),                  # a tie reports the point
    ]
    lib = ctx._lib
    vkb = np.frombuffer(vk, dtype=np.uint8).copy()
    good3 = ctx.verify_reduce_segments(LOG_N, vk, good, None, weights, None, FR_BYTES_LE, 3)
    for segment in (1, 3, m):
        for faults, code, index, text in cases:
            with pytest.raises(bp.BpError) as e:
                ctx.verify_reduce_segments(LOG_N, vk, with_faults(faults), None, weights, None, FR_BYTES_LE, segment)
            assert e.value.code == code and e.value.index == index and text in str(e.value) and ("proof %d" % index) in str(e.value), str(e.value)
            buf = np.frombuffer(with_faults(faults), dtype=np.uint8).copy()
            out, bad = np.full(192 * m, 0xA5, dtype=np.uint8), C.c_size_t(0)
            rc = lib.bp_verify_reduce_segments(ctx._h, LOG_N, vkb.ctypes.data, buf.ctypes.data, m, None, 0, weights.ctypes.data, None, FR_BYTES_LE,
                                               segment, out.ctypes.data, C.byref(bad))
            assert rc == code and bad.value == index and (out == 0xA5).all()
        assert ctx.verify_reduce_segments(LOG_N, vk, good, None, weights, None, FR_BYTES_LE, 3) == good3      # no stale status
    w_bad = weights.copy()
    w_bad[13] = np.frombuffer(q_le, dtype=np.uint8)
    with pytest.raises(bp.BpError) as e:
        ctx.verify_reduce_segments(LOG_N, vk, good, None, w_bad, None, FR_BYTES_LE, 5)
    assert e.value.code == -4 and e.value.index == 13
    # the argument rules of its own: segment 0; no weights for a segment of several proofs
    out = np.full(192 * m, 0xA5, dtype=np.uint8)
    buf = np.frombuffer(good, dtype=np.uint8).copy()
    assert lib.bp_verify_reduce_segments(ctx._h, LOG_N, vkb.ctypes.data, buf.ctypes.data, m, None, 0, weights.ctypes.data, None, FR_BYTES_LE, 0,
                                         out.ctypes.data, None) == -1
    assert lib.bp_verify_reduce_segments(ctx._h, LOG_N, vkb.ctypes.data, buf.ctypes.data, 3, None, 0, None, None, FR_BYTES_LE, 2, out.ctypes.data, None) == -1
    assert (out == 0xA5).all()
    with pytest.raises(bp.BpError) as e:
        ctx.verify_reduce_segments(LOG_N, vk, good, None, weights, None, FR_BYTES_LE, 0)
    assert e.value.code == -1
    with pytest.raises(bp.BpError) as e:
        ctx.verify_reduce_segments(LOG_N, vk, good[:624 * 3], None, None, None, FR_BYTES_LE, 2)
    assert e.value.code == -1
    assert len(ctx.verify_reduce_segments(LOG_N, vk, good[:624 * 3], None, None, None, FR_BYTES_LE, 1)) == 3      # weight 1 each
    assert len(ctx.verify_reduce_segments(LOG_N, vk, good[:624], None, None, None, FR_BYTES_LE, 2)) == 1          # m = 1
    with pytest.raises(bp.BpError) as e:
        ctx.verify_reduce_segments(LOG_N, vk, good, scal([1] * (m * 9), (m, 9)), weights, None, FR_BYTES_LE, 2)       # n_public > n
    assert e.value.code == -6
    with pytest.raises(bp.BpError) as e:
        ctx.verify_reduce_segments(2, vk, good, None, weights, None, FR_BYTES_LE, 2)
    assert e.value.code == -1
    with pytest.raises(bp.BpError) as e:
        ctx.verify_reduce_segments(LOG_N, bytes([0x80]) + vk[1:], good, None, weights, None, FR_BYTES_LE, 2)
    assert e.value.code == -3
    assert ctx.verify_reduce_segments(LOG_N, vk, good, None, weights, None, FR_BYTES_LE, 3) == good3


# ---- locating, with real proofs ----------------------------------------------------------------------------------------------
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
    return tau, bp.Verifier(setup, circuit), proofs, publics


def test_locate_invalid_names_exactly_the_bad_proofs(real):
    tau, verifier, proofs, publics = real
    m, rnd = len(proofs), random.Random(2)
    weights = scal([rnd.getrandbits(128) for _ in range(m)], (m,))
    calls = []

    def decide(a96, b96):                                        # the pairing equation with the known tau: tau A == B
        calls.append(1)
        A, B = dec96(a96), dec96(b96)
        return A is not None and M.ec_mul(tau, A) == B
    pub = lambda rows: scal([x for row in rows for x in row], (len(rows), 3))
    bound = lambda k: 1 + 2 * k * math.ceil(math.log2(m))
    assert verifier.locate_invalid(proofs, pub(publics), weights, decide, FR_BYTES_LE) == [] and len(calls) == 1
    # the segment pairs of real proofs: every one accepted alone, and segment = m is pairing_inputs itself
    assert all(decide(*pair) for pair in verifier.pairing_inputs_segments(proofs, pub(publics), weights, None, FR_BYTES_LE, 5))
    assert verifier.pairing_inputs_segments(proofs, pub(publics), weights, None, FR_BYTES_LE, m) == [verifier.pairing_inputs(proofs, pub(publics), weights,
                                                                                                                               fmt=FR_BYTES_LE)]
    bad = list(proofs)
    for j in (0, 17, 31):                                        # a flipped bit in an evaluation
        t = bytearray(bad[j])
        t[432 + 32 * (j % 6)] ^= 1
        bad[j] = bytes(t)
    calls.clear()
    assert verifier.locate_invalid(bad, pub(publics), weights, decide, FR_BYTES_LE) == [0, 17, 31]
    assert 1 < len(calls) <= bound(3), len(calls)
    wrong = [row[:] for row in publics]
    wrong[5][1] = (wrong[5][1] + 1) % Q                          # a wrong public input
    calls.clear()
    assert verifier.locate_invalid(proofs, pub(wrong), weights, decide, FR_BYTES_LE) == [5]
    assert 1 < len(calls) <= bound(1), len(calls)

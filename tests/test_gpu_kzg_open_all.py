"""-m gpu: all n proofs of one polynomial on its domain in one call (Setup.open_all, bp_kzg_open_all, bp_kzg_open_all_device,
bp_srs_open_all_prepare), byte for byte against closed forms in Python integers over the oracle's G1 (tests/kzg_model.py): proof i is
[horner(quotient_coeffs(f, w^i), tau)] G -- no division by tau - w^i, so tau on the domain is covered -- and value i is f(w^i) by
Horner.  No expectation comes from the library; test_against_single_openings compares two of its routes ON TOP of the closed form.
Sizes: log_n = 1..4 (a few lanes, N = 4 the smallest real convolution), 7 (N = 256: the first pass with >= 64 groups and a
non-trivial twiddle), 9 (N = 1024: more than one workgroup per pass)."""
import random

import numpy as np
import pytest

import baby_plonk_rust_amd as bp
from baby_plonk_rust_amd import BASIS_LAGRANGE, BASIS_MONOMIAL, FR_BYTES_LE, FR_MONT
from tests import bigint_model as M
from tests import kzg_model as K

pytestmark = pytest.mark.gpu
Q = M.Q
ID96 = bytes([0x40]) + bytes(95)
TAU = 0x5EED0123456789ABCDEF0F1E2D3C4B5A69788796A5B4C3D2E1F00112233445566 % Q
LOGS = (1, 2, 3, 4, 7, 9)


@pytest.fixture(scope="module")
def ctx():
    c = bp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def setups(ctx):
    """powers-of-tau setups by (length, tau), made once"""
    made = {}

    def get(n, tau=TAU):
        if (n, tau) not in made:
            made[(n, tau)] = bp.Setup.generate_srs(n, tau, ctx, tables=False)
        return made[(n, tau)]
    yield get
    for s in made.values():
        ctx.srs_free(s.handle)


def values_of(f, n):
    return [K.horner(f, z) for z in K.domain(n)]


def proof_scalars(f, n, tau):
    """q_i(tau) for q_i = (f - f(w^i)) / (x - w^i), division-free; zero-padding f to n coefficients would add zero coefficients only"""
    return [K.horner(K.quotient_coeffs(f, z), tau) for z in K.domain(n)]


def records(scalars):
    return [K.point96(k) for k in scalars]


def check(got, want_ys, want_proofs):
    ys, proofs = got
    assert ys.shape == (len(want_ys), 4) and proofs.shape == (len(want_ys), 96)
    assert bp.scalars_to_ints(ys) == want_ys
    for i, w in enumerate(want_proofs):
        assert bytes(proofs[i]) == w, i


def host(ctx, ints, basis=BASIS_MONOMIAL):
    return bp.Polynomial(bp.scalars_from_ints(ints), basis, ctx)


def dev(ctx, ints, basis=BASIS_MONOMIAL):
    return bp.DevicePolynomial(bp.scalars_from_ints(ints), basis, ctx)


def raw_open_all(ctx, handle, ints, basis, log_n):
    """bp_kzg_open_all itself with canonical little-endian bytes in and out: (rc, values as ints, proofs [n, 96])"""
    n = 1 << log_n
    src = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints) + bytes(32), dtype=np.uint8).copy()
    vals, proofs = np.zeros(32 * n, dtype=np.uint8), np.zeros((n, 96), dtype=np.uint8)
    rc = ctx._lib.bp_kzg_open_all(ctx._h, handle, src.ctypes.data, len(ints), basis, FR_BYTES_LE, log_n, vals.ctypes.data, proofs.ctypes.data)
    return rc, [int.from_bytes(vals[32 * i: 32 * i + 32].tobytes(), "little") for i in range(n)], proofs


# ---- 1. the closed form under a generated SRS of known tau ---------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", LOGS)
def test_closed_form(ctx, setups, log_n):
    n, rng = 1 << log_n, random.Random(log_n)
    setup = setups(n - 1)                                         # only the first n - 1 points are used
    rand = [rng.randrange(Q) for _ in range(n)]
    polys = {"random": rand, "zero": [0] * n, "constant": [rng.randrange(1, Q)], "top": [0] * (n - 1) + [1],
             "len 1": [rng.randrange(1, Q)], "len 2": [rng.randrange(Q), rng.randrange(1, Q)], "len n-1": [rng.randrange(1, Q) for _ in range(n - 1)]}
    for name, f in polys.items():
        want_ys, want = values_of(f, n), records(proof_scalars(f, n, TAU))
        if name == "random":
            rand_ys, rand_want = want_ys, want
        if name in ("zero", "constant", "len 1"):
            assert want == [ID96] * n                              # the quotient of a constant is zero
        if name == "top":                                          # X^(n-1) alone: h_m = P_{n-2-m}, pi_i = sum_m w^(i m) P_{n-2-m}
            assert want[0] == K.point96(sum(pow(TAU, k, Q) for k in range(n - 1)))
        check(setup.open_all(host(ctx, f), n), want_ys, want)                                       # host entry, Montgomery limbs
        check(setup.open_all(dev(ctx, f), n), want_ys, want)                                        # device entry
        rc, vals, proofs = raw_open_all(ctx, setup.handle, f, BASIS_MONOMIAL, log_n)            # host entry, canonical bytes
        assert rc == 0 and vals == want_ys and [bytes(p) for p in proofs] == want, name
    # the Lagrange form of the random polynomial (its values by Horner, not by the library): the same proofs, and the values are the input
    want_ys, want = rand_ys, rand_want
    check(setup.open_all(host(ctx, want_ys, BASIS_LAGRANGE)), want_ys, want)
    check(setup.open_all(dev(ctx, want_ys, BASIS_LAGRANGE)), want_ys, want)
    rc, vals, proofs = raw_open_all(ctx, setup.handle, want_ys, BASIS_LAGRANGE, log_n)
    assert rc == 0 and vals == want_ys and [bytes(p) for p in proofs] == want
    # values = NULL is allowed
    out = np.zeros((n, 96), dtype=np.uint8)
    p = host(ctx, rand)
    assert ctx._lib.bp_kzg_open_all(ctx._h, setup.handle, p._ptr(), n, BASIS_MONOMIAL, FR_MONT, log_n, None, out.ctypes.data) == 0
    assert [bytes(x) for x in out] == want


# ---- 2. degenerate point sets ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau_kind", ("one", "on_domain"))
def test_degenerate_points(ctx, setups, tau_kind):
    """tau = 1: all points equal, so additions become doublings and cancellations; tau = w_8: tau on the domain"""
    n, rng = 8, random.Random(8)
    tau = 1 if tau_kind == "one" else M.omega(n)
    setup = setups(n - 1, tau)
    for f in ([rng.randrange(Q) for _ in range(n)], [0] * (n - 1) + [1], [rng.randrange(Q) for _ in range(n - 1)]):
        check(setup.open_all(dev(ctx, f), n), values_of(f, n), records(proof_scalars(f, n, tau)))


# ---- 3. a point set that is no powers of tau -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (8, 128))
@pytest.mark.parametrize("a", (0x1234567, 0))
def test_progression_points(ctx, n, a):
    """P_k = (a + k d) G: the map is linear in the points, so pi_i = [sum_m w^(i m) sum_k f_{m+1+k} (a + k d)] G -- the index map
    pinned with no tau identity.  a = 0 makes P_0 the identity: bp_srs_generate_progression accepts it (the SRS store holds it as
    (0, 0)), so that case runs too."""
    d, rng = 0x89ABCDEF01, random.Random(n + a)
    h = ctx.srs_generate_progression(n - 1, a, d)
    setup = bp.Setup(h, ctx, tables=False)
    try:
        f, dom = [rng.randrange(Q) for _ in range(n)], K.domain(n)
        hm = [sum(f[m + 1 + k] * (a + k * d) for k in range(n - 1 - m)) % Q for m in range(n)]
        want = records([K.horner(hm, z) for z in dom])             # sum_m z^m h_m
        check(setup.open_all(dev(ctx, f), n), values_of(f, n), want)
        check(setup.open_all(host(ctx, f), n), values_of(f, n), want)
    finally:
        ctx.srs_free(h)


# ---- 4. against the route that exists today -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (8, 16))
def test_against_single_openings(ctx, setups, n):
    rng = random.Random(n)
    setup, f = setups(n), [rng.randrange(Q) for _ in range(n)]
    p = dev(ctx, f)
    ys, proofs = setup.open_all(p, n)
    check((ys, proofs), values_of(f, n), records(proof_scalars(f, n, TAU)))
    for i, z in enumerate(K.domain(n)):
        y1, w1 = setup.open(p, bp.scalar_from_int(z))
        assert bytes(proofs[i]) == w1 and (ys[i] == y1[0]).all(), i


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------------------
def test_claims_pass_the_batch_check(ctx, setups):
    n, rng = 128, random.Random(5)
    setup, f = setups(n), [rng.randrange(Q) for _ in range(n)]
    p = dev(ctx, f)
    com = K.point96(K.horner(f, TAU))
    assert setup.commit_many_device([p])[0] == com
    ys, proofs = setup.open_all(p, n)
    dom, picks = K.domain(n), (0, 1, 63, 64, 127)

    def claims(ys, proofs):
        return [bp.Opening(com, bp.scalar_from_int(dom[i]), ys[i:i + 1], None, bytes(proofs[i])) for i in picks]
    for on_host in (True, False):
        assert setup.verify_openings(claims(ys, proofs), host=on_host) is True
    swapped = proofs.copy()
    swapped[[63, 64]] = swapped[[64, 63]]                          # one proof swapped for its neighbour
    assert setup.verify_openings(claims(ys, swapped)) is False
    off = ys.copy()
    off[1] = bp.scalar_from_int((K.horner(f, dom[1]) + 1) % Q)    # one value off by one
    assert setup.verify_openings(claims(off, proofs)) is False


# ---- 6. the prepared table ---------------------------------------------------------------------------------------------------------------------
def test_prepared_table(ctx):
    rng = random.Random(6)
    setup = bp.Setup.generate_srs(16, TAU, ctx, tables=False)
    lag_before = ctx.srs_lagrange(setup.handle, 4)
    f8, f16 = [rng.randrange(Q) for _ in range(8)], [rng.randrange(Q) for _ in range(16)]
    p8, p16 = dev(ctx, f8), dev(ctx, f16)
    first = setup.open_all(p8, 8)
    assert ctx.kzg_open_all_stats()["table_ms"] > 0
    check(first, values_of(f8, 8), records(proof_scalars(f8, 8, TAU)))
    again = setup.open_all(p8, 8)
    stats = ctx.kzg_open_all_stats()
    assert stats["table_ms"] == 0 and min(stats["field_ms"], stats["toeplitz_ms"], stats["final_ms"]) > 0
    assert (again[0] == first[0]).all() and (again[1] == first[1]).all()
    check(setup.open_all(p16, 16), values_of(f16, 16), records(proof_scalars(f16, 16, TAU)))      # log_n = 4 replaces the table
    assert ctx.kzg_open_all_stats()["table_ms"] > 0
    back = setup.open_all(p8, 8)                                                                     # and 3 again
    assert ctx.kzg_open_all_stats()["table_ms"] > 0 and (back[0] == first[0]).all() and (back[1] == first[1]).all()
    other = bp.Setup.generate_srs(16, TAU, ctx, tables=False)                                        # explicit prepare == none
    other.prepare_open_all(8)
    prepared = other.open_all(p8, 8)
    assert ctx.kzg_open_all_stats()["table_ms"] == 0 and (prepared[1] == first[1]).all() and (prepared[0] == first[0]).all()
    other.prepare_open_all(1)                                                                        # log_n = 0: nothing to prepare
    lag_after = ctx.srs_lagrange(setup.handle, 4)
    assert ctx.srs_export(lag_before) == ctx.srs_export(lag_after)
    for h in (lag_before, lag_after, other.handle, setup.handle):
        ctx.srs_free(h)                                                                              # bp_srs_free with a table attached succeeds
    with pytest.raises(bp.BpError):
        ctx.srs_len(setup.handle)


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_output_untouched(ctx, setups):
    setup = setups(16)
    lag = ctx.srs_lagrange(setup.handle, 3)
    f = list(range(1, 9))
    try:
        cases = {"Lagrange SRS handle": (lag, f, BASIS_MONOMIAL, 3, -5),
                 "n - 1 > srs_len": (setup.handle, f, BASIS_MONOMIAL, 5, -6),
                 "n_values > n": (setup.handle, f + [1], BASIS_MONOMIAL, 3, -6),
                 "Lagrange input of the wrong length": (setup.handle, f[:7], BASIS_LAGRANGE, 3, -6),
                 "log_n = 24": (setup.handle, f, BASIS_MONOMIAL, 24, -10),
                 "a byte scalar >= q": (setup.handle, f[:7] + [Q], BASIS_MONOMIAL, 3, -4),
                 "unknown handle": (0xDEAD, f, BASIS_MONOMIAL, 3, -1)}
        for name, (handle, ints, basis, log_n, code) in cases.items():
            n_out = 1 << min(log_n, 5)                             # the buffers of a call that must write nothing: small is enough
            src = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), dtype=np.uint8).copy()
            vals, proofs = np.full(32 * n_out, 0xA5, dtype=np.uint8), np.full(96 * n_out, 0xA5, dtype=np.uint8)
            rc = ctx._lib.bp_kzg_open_all(ctx._h, handle, src.ctypes.data, len(ints), basis, FR_BYTES_LE, log_n, vals.ctypes.data, proofs.ctypes.data)
            assert rc == code, (name, rc)
            assert (vals == 0xA5).all() and (proofs == 0xA5).all(), name
            if name != "a byte scalar >= q":                       # the device entry takes Montgomery limbs: no such thing as a value >= q
                d = dev(ctx, [v % Q for v in ints])
                rc = ctx._lib.bp_kzg_open_all_device(ctx._h, handle, d._ptr(), len(ints), basis, log_n, vals.ctypes.data, proofs.ctypes.data)
                assert rc == code and (vals == 0xA5).all() and (proofs == 0xA5).all(), name
        out = np.full(96, 0xA5, dtype=np.uint8)
        src = np.zeros(32, dtype=np.uint8)
        assert ctx._lib.bp_kzg_open_all(ctx._h, setup.handle, src.ctypes.data, 1, BASIS_MONOMIAL, 7, 0, None, out.ctypes.data) == -1      # bad format
        assert ctx._lib.bp_kzg_open_all(ctx._h, setup.handle, src.ctypes.data, 1, 9, FR_MONT, 0, None, out.ctypes.data) == -1              # bad basis
        assert ctx._lib.bp_kzg_open_all(ctx._h, setup.handle, None, 1, BASIS_MONOMIAL, FR_MONT, 0, None, out.ctypes.data) == -1            # null polynomial
        assert ctx._lib.bp_kzg_open_all(ctx._h, setup.handle, src.ctypes.data, 1, BASIS_MONOMIAL, FR_MONT, 0, None, None) == -1            # null output
        assert ctx._lib.bp_kzg_open_all_last_stats(ctx._h, None) == -1 and ctx._lib.bp_srs_open_all_prepare(None, setup.handle, 3) == -1
        assert (out == 0xA5).all()
    finally:
        ctx.srs_free(lag)


def test_log_n_zero(ctx, setups):
    """one proof, the identity, and the value f_0; an empty SRS prefix is enough (n - 1 = 0 points)"""
    setup = setups(16)
    for f in ([12345], []):
        for p in (host(ctx, f), dev(ctx, f)):
            ys, proofs = setup.open_all(p, 1)
            assert bp.scalars_to_ints(ys) == [f[0] if f else 0] and bytes(proofs[0]) == ID96
    rc, vals, proofs = raw_open_all(ctx, setup.handle, [777], BASIS_LAGRANGE, 0)
    assert rc == 0 and vals == [777] and bytes(proofs[0]) == ID96
    assert ctx.kzg_open_all_stats() == {"table_ms": 0, "field_ms": 0, "toeplitz_ms": 0, "final_ms": 0}


# ---- 8. a group context ------------------------------------------------------------------------------------------------------------------------
def test_group_context(ctx, setups):
    """a two-member rehearsal context {0, 0}: the SRS is sharded, the points are collected on the primary device; the bytes of the
    plain context"""
    n, rng = 16, random.Random(16)
    f = [rng.randrange(Q) for _ in range(n)]
    want_ys, want = values_of(f, n), records(proof_scalars(f, n, TAU))
    check(setups(n).open_all(host(ctx, f), n), want_ys, want)
    many = bp.Context([0, 0])
    try:
        assert many.n_shards() == 2
        setup = bp.Setup.generate_srs(n, TAU, many, tables=False)
        check(setup.open_all(host(many, f), n), want_ys, want)
        check(setup.open_all(dev(many, f), n), want_ys, want)
        check(setup.open_all(host(many, want_ys, BASIS_LAGRANGE)), want_ys, want)
        many.srs_free(setup.handle)
    finally:
        many.close()

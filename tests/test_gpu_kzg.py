"""-m gpu: KZG openings in either basis (Setup.open, bp_kzg_open, bp_kzg_open_device) and their batch check (bp_kzg_verify_reduce,
Setup.verify_openings), byte for byte against the closed form of tests/kzg_model.py under a generated SRS of known tau: the values
by Horner / the barycentric formula in Python integers, the proof as [q(tau)] G from the oracle's G1.  No expectation comes from the
library (the cross-basis test compares two of its routes with each other, on top of the closed form)."""
import ctypes as C
import random

import numpy as np
import pytest

import baby_plonk_rust_amd as bp
from baby_plonk_rust_amd import BASIS_LAGRANGE, BASIS_MONOMIAL, FR_BYTES_LE, FR_MONT
from tests import bigint_model as M
from tests import kzg_model as K
from tests import pairing_cases as PC

pytestmark = pytest.mark.gpu
Q = M.Q
ID96 = bytes([0x40]) + bytes(95)
TAU = 0x5EED0123456789ABCDEF0F1E2D3C4B5A69788796A5B4C3D2E1F00112233445566 % Q
BIG = 131073                                 # points of the long Monomial setup: the quotient of the longest polynomial below


@pytest.fixture(scope="module")
def ctx():
    c = bp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def setups(ctx):
    """powers-of-tau setups by length and their Lagrange forms, made once"""
    made = {}

    def get(n, lagrange=False):
        if (n, False) not in made:
            made[(n, False)] = bp.Setup.generate_srs(n, TAU, ctx, tables=False)
        if lagrange and (n, True) not in made:
            made[(n, True)] = made[(n, False)].lagrange(n, tables=False)
        return made[(n, lagrange)]
    yield get
    for s in made.values():
        ctx.srs_free(s.handle)


def dev(ctx, ints, basis):
    return bp.DevicePolynomial(bp.scalars_from_ints(ints), basis, ctx)


def host(ctx, ints, basis):
    return bp.Polynomial(bp.scalars_from_ints(ints), basis, ctx)


def check_open(setup, polys, z, nu, want):
    """Setup.open against (ys, q(tau)) of the model"""
    ys, w = setup.open(polys, bp.scalar_from_int(z), None if nu is None else bp.scalar_from_int(nu))
    want_ys, want_w = want
    assert bp.scalars_to_ints(ys) == want_ys
    assert w == K.point96(want_w)
    return ys, w


def code_of(fn):
    with pytest.raises(bp.BpError) as e:
        fn()
    return e.value.code


# ---- Lagrange form -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 8, 64, 256, 1024, 8192])
def test_lagrange_opening(ctx, setups, n):
    """n = 1, 2, 8: a few lanes of one wave; 64: one wave; 256: one workgroup; 1024: several workgroups, one scan tile; 8192: four
    scan tiles and sums across 32 workgroups.  Every z of {random, 0, w^0, w, w^(n/2), w^(n-1), w_2n} (the last off the domain with z^n = -1) with every f of
    {random, zero, constant, one-hot at m, one-hot next to m}, m the index of z on the domain (n / 2 where z is off it)."""
    rng = random.Random(n)
    lag, dom = setups(n, True), K.domain(n)
    zs = {"random": rng.randrange(Q), "zero": 0, "w^0": 1, "w": dom[1 % n], "w^(n/2)": dom[n // 2], "w^(n-1)": dom[n - 1], "w_2n": M.omega(2 * n)}
    fixed = {"random": [rng.randrange(Q) for _ in range(n)], "zero": [0] * n, "constant": [rng.randrange(1, Q)] * n}
    polys = {k: dev(ctx, v, BASIS_LAGRANGE) for k, v in fixed.items()}
    for zname, z in zs.items():
        m = dom.index(z) if z in dom else n // 2
        hot = {"hot at m": [int(i == m) * 5 for i in range(n)], "hot next to m": [int(i == (m + 1) % n) * 7 for i in range(n)]}
        for fname, f in list(fixed.items()) + list(hot.items()):
            p = polys[fname] if fname in polys else dev(ctx, f, BASIS_LAGRANGE)
            ys, w = check_open(lag, p, z, None, K.open_lagrange([f], z, 0, TAU))
            if fname in ("zero", "constant"):
                assert w == ID96, (zname, fname)
            if z in dom:
                assert bp.scalars_to_ints(ys) == [f[m]], (zname, fname)


# ---- Monomial form -----------------------------------------------------------------------------------------------------------------------
DIV_PATH = {2: 1, 33: 1, 34: 2, 2049: 2, 2050: 3, 4097: 3, 131074: 4}      # length -> poly_div_run path of its quotient (no quotient at 1)


@pytest.mark.parametrize("length", [1, 2, 33, 34, 2049, 2050, 4097, 131074])
def test_monomial_opening(ctx, setups, length):
    """the quotient has length - 1 coefficients: one chunk (1, 32), the plain carry (33 .. 2048), the workgroup carry (2049, 4096) and
    the segmented carry (131073) of poly_div_run, either side of each boundary"""
    rng = random.Random(length)
    setup = setups(BIG)
    f = [rng.randrange(Q) for _ in range(length - 1)] + [rng.randrange(1, Q)]
    p = dev(ctx, f, BASIS_MONOMIAL)
    for z in (rng.randrange(Q), 0, 1):
        _, w = check_open(setup, p, z, None, K.open_monomial([f], z, 0, TAU))
        if length == 1:
            assert w == ID96
        else:
            assert ctx.poly_stats()["div_path"] == DIV_PATH[length], (length, ctx.poly_stats())


def test_monomial_quotient_keeps_its_zero_coefficients(ctx, setups):
    """f = x^5 - z^5 has the quotient x^4 + z x^3 + .. + z^4; at z = 0 that is x^4 with four zero coefficients below it, which
    bp_poly_div would squeeze out"""
    f = [0, 0, 0, 0, 0, 1]
    check_open(setups(8), dev(ctx, f, BASIS_MONOMIAL), 0, None, ([0], pow(TAU, 4, Q)))


# ---- the same polynomial in both bases -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 1024])
def test_cross_basis(ctx, setups, n):
    rng = random.Random(n + 1)
    coeffs = [rng.randrange(Q) for _ in range(n)]
    mono = dev(ctx, coeffs, BASIS_MONOMIAL)
    evals = mono.ntt()
    for z in (rng.randrange(Q), K.domain(n)[n // 4 + 1]):
        want = K.open_monomial([coeffs], z, 0, TAU)
        a = check_open(setups(n), mono, z, None, want)
        b = check_open(setups(n, True), evals, z, None, want)
        assert (a[0] == b[0]).all() and a[1] == b[1]


# ---- many polynomials at one point ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 7, 16])
@pytest.mark.parametrize("basis", [BASIS_LAGRANGE, BASIS_MONOMIAL])
def test_many_polynomials(ctx, setups, count, basis):
    rng = random.Random(count * 2 + basis)
    n = 64
    if basis == BASIS_LAGRANGE:
        vecs = [[rng.randrange(Q) for _ in range(n)] for _ in range(count)]
        setup, model = setups(n, True), K.open_lagrange
    else:
        lengths = ([0, 5, 33, 1, 64, 2, 65, 17] * 2)[:count] if count > 1 else [40]      # mixed, with a zero polynomial and a constant
        vecs = [[rng.randrange(Q) for _ in range(k)] for k in lengths]
        setup, model = setups(n), K.open_monomial
    polys = [dev(ctx, v, basis) for v in vecs]
    for z in (rng.randrange(Q), K.domain(n)[3]):
        for nu in (rng.randrange(Q), 0, 1):
            check_open(setup, polys, z, nu, model(vecs, z, nu, TAU))
    if count == 1:
        check_open(setup, polys[0], z, None, model(vecs, z, 0, TAU))


# ---- host and device entry points, both scalar formats ----------------------------------------------------------------------------
def raw_open(ctx, setup, vecs, basis, z, nu, fmt, device):
    """bp_kzg_open / bp_kzg_open_device through ctypes: (rc, ys as integers, W96).  The device call takes Montgomery polynomials."""
    def scal(vals, f):
        if f == FR_MONT:
            return bp.scalars_from_ints(vals)
        return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(-1, 32).copy()
    k = len(vecs)
    if device:
        keep = [dev(ctx, v, basis) for v in vecs]
        ptrs = (C.c_void_p * k)(*[p._ptr() or None for p in keep])
    else:
        keep = [scal(v, fmt) for v in vecs]
        ptrs = (C.c_void_p * k)(*[a.ctypes.data if len(a) else None for a in keep])
    lens = (C.c_size_t * k)(*[len(v) for v in vecs])
    zz, nn = scal([z], fmt), None if nu is None else scal([nu], fmt)
    ys, w = scal([0] * k, fmt), np.zeros(96, dtype=np.uint8)
    fn = ctx._lib.bp_kzg_open_device if device else ctx._lib.bp_kzg_open
    rc = fn(ctx._h, setup.handle, ptrs, lens, k, basis, zz.ctypes.data, None if nn is None else nn.ctypes.data, fmt, ys.ctypes.data, w.ctypes.data)
    got = bp.scalars_to_ints(ys) if fmt == FR_MONT else [int.from_bytes(ys[j].tobytes(), "little") for j in range(k)]
    return rc, got, bytes(w)


@pytest.mark.parametrize("basis", [BASIS_LAGRANGE, BASIS_MONOMIAL])
def test_host_and_device_calls_in_both_formats(ctx, setups, basis):
    rng = random.Random(90 + basis)
    n = 64
    vecs = [[rng.randrange(Q) for _ in range(n if basis == BASIS_LAGRANGE else k)] for k in (64, 0, 31)]
    setup = setups(n, basis == BASIS_LAGRANGE)
    z, nu = rng.randrange(Q), rng.randrange(Q)
    want_ys, want_w = (K.open_lagrange if basis == BASIS_LAGRANGE else K.open_monomial)(vecs, z, nu, TAU)
    for device in (False, True):
        for fmt in (FR_MONT, FR_BYTES_LE):
            assert raw_open(ctx, setup, vecs, basis, z, nu, fmt, device) == (0, want_ys, K.point96(want_w)), (device, fmt)
    # the host form through the Python interface
    check_open(setup, [host(ctx, v, basis) for v in vecs], z, nu, (want_ys, want_w))
    stats = ctx.kzg_stats()
    assert stats["values_quotient_ms"] > 0 and stats["commit_ms"] > 0


# ---- verdicts ---------------------------------------------------------------------------------------------------------------------------
def honest_claims(ctx, setup, m, count, seed):
    """m claims of `count` short Monomial polynomials each, every field from the library's own commit and open"""
    rng = random.Random(seed)
    out, logs = [], []
    for _ in range(m):
        vecs = [[rng.randrange(Q) for _ in range(rng.randrange(2, 9))] for _ in range(count)]
        polys = [dev(ctx, v, BASIS_MONOMIAL) for v in vecs]
        z, nu = rng.randrange(Q), rng.randrange(Q)
        ys, w = setup.open(polys, bp.scalar_from_int(z), bp.scalar_from_int(nu))
        out.append(bp.Opening(setup.commit_many_device(polys), bp.scalar_from_int(z), ys, bp.scalar_from_int(nu), w))
        logs.append(K.horner(vecs[0], TAU))
    return out, logs


@pytest.mark.parametrize("m", [1, 2, 65])
def test_verdicts(ctx, setups, m):
    setup = setups(16)
    claims, logs = honest_claims(ctx, setup, m, 2, m)
    rng = random.Random(1000 + m)
    weights = bp.scalars_from_ints([rng.getrandbits(128) | 1 << 127 for _ in range(m)])
    assert setup.verify_openings(claims, weights, host=True) is True and setup.verify_openings(claims, weights, host=False) is True
    assert setup.verify_openings(claims) is True                                          # weights drawn inside
    t = m // 2
    o = claims[t]
    bump = lambda limbs: bp.scalar_from_int(bp.scalar_to_int(limbs) + 1)
    other_c = [K.point96(logs[t] + 1)] + list(o.commitments[1:])
    tampered = {"C": o._replace(commitments=other_c), "y": o._replace(ys=np.stack([bump(o.ys[0]), o.ys[1]])), "z": o._replace(z=bump(o.z)),
                "nu": o._replace(nu=bump(o.nu)), "W": o._replace(proof=K.point96(3))}
    for what, bad in tampered.items():
        batch = claims[:t] + [bad] + claims[t + 1:]
        on_host = setup.verify_openings(batch, weights, host=True)
        assert on_host is False, what
        assert setup.verify_openings(batch, weights, host=False) is on_host, what
    assert ctx.kzg_stats()["reduce_ms"] > 0


def test_reduce_of_nothing_and_of_one_claim_without_weights(ctx, setups):
    setup = setups(16)
    assert setup.opening_pairing_inputs([]) == (ID96, ID96)
    claims, _ = honest_claims(ctx, setup, 1, 1, 5)
    single = claims[0]._replace(nu=None, commitments=claims[0].commitments[0])
    assert setup.verify_openings(single) is True                                         # nu = None, weights = None: one claim of one polynomial
    # A = W and B = C - y G + z W, as the closed form has them
    a96, b96 = setup.opening_pairing_inputs(single)
    assert a96 == single.proof


# ---- errors -----------------------------------------------------------------------------------------------------------------------------
def test_open_errors(ctx, setups):
    mono, lag = setups(8), setups(8, True)
    f8 = [1, 2, 3, 4, 5, 6, 7, 8]
    z = bp.scalar_from_int(5)
    assert code_of(lambda: mono.open(dev(ctx, f8, BASIS_LAGRANGE), z)) == -5                 # the basis of the SRS, both ways
    assert code_of(lambda: lag.open(dev(ctx, f8, BASIS_MONOMIAL), z)) == -5
    assert code_of(lambda: lag.open(dev(ctx, f8[:4], BASIS_LAGRANGE), z)) == -6             # Lagrange: exactly srs_len values
    assert code_of(lambda: lag.open(dev(ctx, f8 + f8, BASIS_LAGRANGE), z)) == -6
    assert code_of(lambda: lag.open(dev(ctx, [], BASIS_LAGRANGE), z)) == -6
    assert code_of(lambda: mono.open(dev(ctx, f8 + [9, 10], BASIS_MONOMIAL), z)) == -6      # nine quotient coefficients, eight points
    check_open(mono, dev(ctx, f8 + [9], BASIS_MONOMIAL), 5, None, K.open_monomial([f8 + [9]], 5, 0, TAU))      # eight: fits
    assert code_of(lambda: mono.open([dev(ctx, f8, BASIS_MONOMIAL)] * 2, z)) == -1           # two polynomials need nu
    assert code_of(lambda: mono.open([dev(ctx, f8, BASIS_MONOMIAL)] * 17, z, z)) == -1      # 1 <= count <= 16
    assert code_of(lambda: mono.open([], z)) == -1
    assert raw_open(ctx, mono, [], BASIS_MONOMIAL, 5, None, FR_MONT, True)[0] == -1         # count = 0 at the C ABI
    assert code_of(lambda: bp.Setup(12345, ctx, tables=False).open(dev(ctx, f8, BASIS_MONOMIAL), z)) == -1      # unknown handle
    for device in (False, True):
        assert raw_open(ctx, mono, [f8], BASIS_MONOMIAL, Q, None, FR_BYTES_LE, device)[0] == -4       # z = q
        assert raw_open(ctx, mono, [f8, f8], BASIS_MONOMIAL, 5, Q + 1, FR_BYTES_LE, device)[0] == -4   # nu > q
    assert raw_open(ctx, mono, [f8[:7] + [Q]], BASIS_MONOMIAL, 5, None, FR_BYTES_LE, False)[0] == -4   # a host coefficient = q
    assert raw_open(ctx, lag, [[Q + 5] + f8[:7]], BASIS_LAGRANGE, 5, None, FR_BYTES_LE, False)[0] == -4
    # the zero polynomial (n_j = 0) alone: value 0, no quotient, the identity
    assert raw_open(ctx, mono, [[]], BASIS_MONOMIAL, 5, None, FR_MONT, True) == (0, [0], ID96)
    # Context.poly_evaluate of a Lagrange polynomial is still refused: the opening is the call that evaluates in that basis
    assert code_of(lambda: dev(ctx, f8, BASIS_LAGRANGE).coeffs_evaluate(z)) == -5


def test_reduce_errors(ctx, setups):
    setup = setups(16)
    claims, _ = honest_claims(ctx, setup, 5, 2, 77)
    weights = bp.scalars_from_ints([3, 5, 7, 11, 13])
    off_curve = bytearray(claims[3].proof)
    off_curve[95] ^= 1
    with pytest.raises(bp.BpError) as e:
        setup.opening_pairing_inputs(claims[:3] + [claims[3]._replace(proof=bytes(off_curve))] + claims[4:], weights)
    assert e.value.code == -3 and e.value.index == 3
    bad_c = [claims[1].commitments[0], bytes(off_curve)]
    with pytest.raises(bp.BpError) as e:                                                 # an off-curve commitment in claim 1 and the proof of claim 3: the lowest
        setup.opening_pairing_inputs([claims[0], claims[1]._replace(commitments=bad_c), claims[2], claims[3]._replace(proof=bytes(off_curve)), claims[4]], weights)
    assert e.value.code == -3 and e.value.index == 1
    outside = PC.outside_subgroup96()
    batch = claims[:2] + [claims[2]._replace(proof=outside)] + claims[3:]
    a96, b96 = setup.opening_pairing_inputs(batch, weights, checks=0)                    # on the curve: accepted when nobody asks for more
    assert len(a96) == 96 and len(b96) == 96
    with pytest.raises(bp.BpError) as e:
        setup.opening_pairing_inputs(batch, weights, checks=1)
    assert e.value.code == -3 and e.value.index == 2
    batch = claims[:4] + [claims[4]._replace(commitments=[claims[4].commitments[0], outside])]
    with pytest.raises(bp.BpError) as e:
        setup.opening_pairing_inputs(batch, weights, checks=1)
    assert e.value.code == -3 and e.value.index == 4
    assert setup.opening_pairing_inputs(claims, weights, checks=1) == setup.opening_pairing_inputs(claims, weights, checks=0)
    assert code_of(lambda: setup.opening_pairing_inputs(claims)) == -1                   # several claims need weights
    assert code_of(lambda: setup.opening_pairing_inputs([c._replace(nu=None) for c in claims], weights)) == -1      # two polynomials need nu
    no_x2 = bp.Setup.from_points(setup.powers_of_x(), ctx, tables=False)
    assert code_of(lambda: no_x2.verify_openings(claims, weights)) == -1
    ctx.srs_free(no_x2.handle)
    # a canonical-bytes scalar >= q names its claim
    le = lambda vals: np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8).copy()
    com = b"".join(b"".join(c.commitments) for c in claims)
    zs = [bp.scalar_to_int(c.z) for c in claims]
    ys = [bp.scalar_to_int(y) for c in claims for y in c.ys]
    nus = [bp.scalar_to_int(c.nu) for c in claims]
    proofs = b"".join(c.proof for c in claims)
    good = ctx.kzg_verify_reduce(com, le(zs), le(ys), le(nus), proofs, le([3, 5, 7, 11, 13]), fmt=FR_BYTES_LE)
    assert good == setup.opening_pairing_inputs(claims, weights)                        # both scalar formats, the same bytes
    with pytest.raises(bp.BpError) as e:
        ctx.kzg_verify_reduce(com, le(zs), le(ys[:4] + [Q] + ys[5:]), le(nus), proofs, le([3, 5, 7, 11, 13]), fmt=FR_BYTES_LE)
    assert e.value.code == -4 and e.value.index == 2


# ---- a context over two shards -----------------------------------------------------------------------------------------------------
def test_group_context_gives_the_same_bytes():
    many = bp.Context([0, 0])
    try:
        n, rng = 1024, random.Random(4)
        setup = bp.Setup.generate_srs(n, TAU, many, tables=False)
        lag = setup.lagrange(n, tables=False)
        f = [rng.randrange(Q) for _ in range(n)]
        for z in (rng.randrange(Q), K.domain(n)[77]):
            check_open(lag, dev(many, f, BASIS_LAGRANGE), z, None, K.open_lagrange([f], z, 0, TAU))
            check_open(setup, dev(many, f, BASIS_MONOMIAL), z, None, K.open_monomial([f], z, 0, TAU))
    finally:
        many.close()

"""-m gpu: the n / l cell proofs of one polynomial in one call (Setup.open_cosets, bp_kzg_open_cosets, bp_kzg_open_cosets_device,
bp_srs_open_cosets_prepare), byte for byte against closed forms in Python integers over the oracle's G1 (tests/kzg_cells_model.py):
proof k is [q_k(tau)] G with q_k = f div (x^l - w^(k l)) by the schoolbook recurrence, value k l + j is f(w^(k + r j)) by Horner.  No
expectation comes from the library; the comparisons with open_all and Setup.commit come ON TOP of the closed form.  Sizes
(log_n, log_l): (2,1) and (3,2) a few lanes; (4,2); (7,3) R = 32, eight sub-transforms of more than one pass side by side; (9,6) the
PeerDAS cell, l = 64, r = 8, five halving passes; (9,2) r = 128, a pass of the batched transforms spans more than one workgroup."""
import random

import numpy as np
import pytest

import baby_plonk_rust_amd as bp
from baby_plonk_rust_amd import BASIS_LAGRANGE, BASIS_MONOMIAL, FR_BYTES_LE, FR_MONT
from tests import bigint_model as M
from tests import kzg_cells_model as CM
from tests import kzg_model as K

pytestmark = pytest.mark.gpu
Q = M.Q
ID96 = bytes([0x40]) + bytes(95)
TAU = 0x5EED0123456789ABCDEF0F1E2D3C4B5A69788796A5B4C3D2E1F00112233445566 % Q
PAIRS = ((2, 1), (3, 2), (4, 2), (7, 3), (9, 6), (9, 2))


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


def model(f, n, l, tau=TAU):
    """(values in cell order [r][l], proof records [r]) of the model"""
    values, scalars = CM.all_cells(f, n, l, tau)
    return values, [K.point96(s) for s in scalars]


def check(got, want_values, want_proofs):
    cells, proofs = got
    r, l = len(want_values), len(want_values[0])
    assert cells.shape == (r, l, 4) and proofs.shape == (r, 96)
    assert bp.scalars_to_ints(cells) == [v for row in want_values for v in row]
    for k, w in enumerate(want_proofs):
        assert bytes(proofs[k]) == w, k


def host(ctx, ints, basis=BASIS_MONOMIAL):
    return bp.Polynomial(bp.scalars_from_ints(ints), basis, ctx)


def dev(ctx, ints, basis=BASIS_MONOMIAL):
    return bp.DevicePolynomial(bp.scalars_from_ints(ints), basis, ctx)


def raw(ctx, handle, ints, basis, log_n, log_l, fill=0):
    """bp_kzg_open_cosets itself with canonical little-endian bytes in and out: (rc, values as ints in cell order, proofs, raw values)"""
    n, r = 1 << min(log_n, 9), max(1 << min(log_n, 9) >> min(log_l, 9), 1)
    src = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints) + bytes(32), dtype=np.uint8).copy()
    vals, proofs = np.full(32 * n, fill, dtype=np.uint8), np.full((r, 96), fill, dtype=np.uint8)
    rc = ctx._lib.bp_kzg_open_cosets(ctx._h, handle, src.ctypes.data, len(ints), basis, FR_BYTES_LE, log_n, log_l, vals.ctypes.data, proofs.ctypes.data)
    return rc, [int.from_bytes(vals[32 * i: 32 * i + 32].tobytes(), "little") for i in range(n)], proofs, vals


# ---- 1. the closed form under a generated SRS of known tau ---------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_l", PAIRS)
def test_closed_form(ctx, setups, log_n, log_l):
    n, l, rng = 1 << log_n, 1 << log_l, random.Random(32 * log_n + log_l)
    r = n // l
    setup = setups(n - l)                                          # only the first n - l points are used
    rand = [rng.randrange(Q) for _ in range(n)]
    polys = {"random": rand, "zero": [0] * n, "top": [0] * (n - 1) + [1], "short": [rng.randrange(1, Q) for _ in range(l - 1)],
             "len l+1": [rng.randrange(1, Q) for _ in range(l + 1)], "len n-1": [rng.randrange(1, Q) for _ in range(n - 1)]}
    for name, f in polys.items():
        want_values, want = model(f, n, l)
        flat = [v for row in want_values for v in row]
        if name == "random":
            rand_values, rand_want = want_values, want
        if name in ("zero", "short"):
            assert want == [ID96] * r                              # fewer than l + 1 coefficients: every quotient is zero
        if name == "len l+1":                                      # q_k = f_l for every k
            assert want == [K.point96(f[l])] * r
        check(setup.open_cosets(host(ctx, f), l, n), want_values, want)                              # host entry, Montgomery limbs
        check(setup.open_cosets(dev(ctx, f), l, n), want_values, want)                               # device entry
        rc, vals, proofs, _ = raw(ctx, setup.handle, f, BASIS_MONOMIAL, log_n, log_l)               # host entry, canonical bytes
        assert rc == 0 and vals == flat and [bytes(p) for p in proofs] == want, name
    # the Lagrange form of the random polynomial (its values by Horner, not by the library): the same proofs, and the values are a
    # permutation of the input: natural order in, cell order out
    natural = [K.horner(rand, z) for z in K.domain(n)]
    assert [natural[k + r * j] for k in range(r) for j in range(l)] == [v for row in rand_values for v in row]
    check(setup.open_cosets(host(ctx, natural, BASIS_LAGRANGE), l), rand_values, rand_want)
    check(setup.open_cosets(dev(ctx, natural, BASIS_LAGRANGE), l), rand_values, rand_want)
    rc, vals, proofs, _ = raw(ctx, setup.handle, natural, BASIS_LAGRANGE, log_n, log_l)
    assert rc == 0 and vals == [v for row in rand_values for v in row] and [bytes(p) for p in proofs] == rand_want
    # values = NULL is allowed
    out = np.zeros((r, 96), dtype=np.uint8)
    p = host(ctx, rand)
    assert ctx._lib.bp_kzg_open_cosets(ctx._h, setup.handle, p._ptr(), n, BASIS_MONOMIAL, FR_MONT, log_n, log_l, None, out.ctypes.data) == 0
    assert [bytes(x) for x in out] == rand_want
    d = dev(ctx, rand)
    out[:] = 0
    assert ctx._lib.bp_kzg_open_cosets_device(ctx._h, setup.handle, d._ptr(), n, BASIS_MONOMIAL, log_n, log_l, None, out.ctypes.data) == 0
    assert [bytes(x) for x in out] == rand_want


# ---- 2. l = 1 is open_all ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", (3, 7))
def test_cell_size_one_equals_open_all(ctx, setups, log_n):
    n, rng = 1 << log_n, random.Random(log_n)
    setup, f = setups(n - 1), [rng.randrange(Q) for _ in range(n)]
    want_ys = [K.horner(f, z) for z in K.domain(n)]
    want = [K.point96(K.horner(K.quotient_coeffs(f, z), TAU)) for z in K.domain(n)]
    assert model(f, n, 1) == ([[y] for y in want_ys], want)         # the two closed forms agree
    for p in (host(ctx, f), dev(ctx, f)):
        cells, proofs = setup.open_cosets(p, 1, n)
        ys, all_proofs = setup.open_all(p, n)
        assert cells.shape == (n, 1, 4) and (cells.reshape(n, 4) == ys).all() and (proofs == all_proofs).all()
        check((cells, proofs), [[y] for y in want_ys], want)


# ---- 3. l = n: one cell, the whole domain ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", (0, 3))
def test_one_cell(ctx, setups, log_n):
    """one identity proof, all n evaluations, no G1 kernel (the G1 stage times are zero); an SRS of zero usable points is enough"""
    n, rng = 1 << log_n, random.Random(77 + log_n)
    setup = setups(1)
    for f in ([rng.randrange(Q) for _ in range(n)], [rng.randrange(1, Q)], []):
        natural = [K.horner(f, z) for z in K.domain(n)]
        for p in (host(ctx, f), dev(ctx, f)):
            cells, proofs = setup.open_cosets(p, n, n)
            assert cells.shape == (1, n, 4) and bp.scalars_to_ints(cells) == natural and [bytes(x) for x in proofs] == [ID96]
            stats = ctx.kzg_open_all_stats()
            assert stats["table_ms"] == 0 and stats["toeplitz_ms"] == 0 and stats["final_ms"] == 0
        rc, vals, proofs, _ = raw(ctx, setup.handle, f, BASIS_MONOMIAL, log_n, log_n)
        assert rc == 0 and vals == natural and bytes(proofs[0]) == ID96
    natural = [rng.randrange(Q) for _ in range(n)]                  # a Lagrange input: the values are the input
    cells, proofs = setup.open_cosets(dev(ctx, natural, BASIS_LAGRANGE), n)
    assert bp.scalars_to_ints(cells) == natural and bytes(proofs[0]) == ID96


# ---- 4. degenerate and foreign point sets ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau_kind", ("one", "on_domain"))
def test_degenerate_points(ctx, setups, tau_kind):
    """tau = 1: all points equal, so additions become doublings and cancellations; tau = w_8: tau on the domain (a_k = tau^l for one k)"""
    n, l, rng = 8, 2, random.Random(8)
    tau = 1 if tau_kind == "one" else M.omega(n)
    setup = setups(n - l, tau)
    for f in ([rng.randrange(Q) for _ in range(n)], [0] * (n - 1) + [1], [rng.randrange(Q) for _ in range(n - 1)]):
        check(setup.open_cosets(dev(ctx, f), l, n), *model(f, n, l, tau))


@pytest.mark.parametrize("log_n,log_l", ((3, 1), (7, 3)))
@pytest.mark.parametrize("a", (0x1234567, 0))
def test_progression_points(ctx, log_n, log_l, a):
    """P_k = (a + k d) G: the map is linear in the points, so pi_k = [sum_m (w^l)^(k m) h_m] G with h from the double sum over the
    scalars a + k d -- the index map pinned with no tau identity.  a = 0 makes P_0 the identity."""
    n, l = 1 << log_n, 1 << log_l
    d, rng = 0x89ABCDEF01, random.Random(n + a)
    h = ctx.srs_generate_progression(n - l, a, d)
    setup = bp.Setup(h, ctx, tables=False)
    try:
        f = [rng.randrange(Q) for _ in range(n)]
        hm = CM.h_double_sum(f, n, l, [(a + k * d) % Q for k in range(n)])
        want = [K.point96(s) for s in CM.proofs_from_h(hm, n, l)]
        values = [CM.cell_values(f, n, l, k) for k in range(n // l)]
        check(setup.open_cosets(dev(ctx, f), l, n), values, want)
        check(setup.open_cosets(host(ctx, f), l, n), values, want)
    finally:
        ctx.srs_free(h)


# ---- 5. against the routes that exist ------------------------------------------------------------------------------------------------------------
def test_against_commit_and_single_openings(ctx, setups):
    n, l, rng = 16, 4, random.Random(42)
    r = n // l
    setup, f = setups(n), [rng.randrange(Q) for _ in range(n)]
    p = dev(ctx, f)
    cells, proofs = setup.open_cosets(p, l, n)
    check((cells, proofs), *model(f, n, l))
    for k in range(r):                                             # the n / l MSM route: commit to the quotient of the host division
        q = CM.quotient(f, n, l, k)
        assert len(q) == n - l and setup.commit(host(ctx, q)) == bytes(proofs[k]), k
    ys, singles = setup.open_all(p, n)                             # the l single-point proofs of a cell claim the same values
    com, dom = K.point96(K.horner(f, TAU)), K.domain(n)
    for k in range(r):
        idx = [k + r * j for j in range(l)]
        assert (ys[idx] == cells[k]).all()
        claims = [bp.Opening(com, bp.scalar_from_int(dom[i]), cells[k, j:j + 1], None, bytes(singles[i])) for j, i in enumerate(idx)]
        assert setup.verify_openings(claims) is True


# ---- 6. the table slot and its key -----------------------------------------------------------------------------------------------------------------
def test_table_key(ctx):
    rng = random.Random(6)
    setup = bp.Setup.generate_srs(16, TAU, ctx, tables=False)
    f = [rng.randrange(Q) for _ in range(16)]
    p = dev(ctx, f)
    want4, want2 = model(f, 16, 4), model(f, 16, 2)
    want_ys = [K.horner(f, z) for z in K.domain(16)]
    want_all = [K.point96(K.horner(K.quotient_coeffs(f, z), TAU)) for z in K.domain(16)]
    table_ms = lambda: ctx.kzg_open_all_stats()["table_ms"]
    first = setup.open_cosets(p, 4, 16)
    assert table_ms() > 0
    check(first, *want4)
    again = setup.open_cosets(p, 4, 16)
    stats = ctx.kzg_open_all_stats()
    assert stats["table_ms"] == 0 and min(stats["field_ms"], stats["toeplitz_ms"], stats["final_ms"]) > 0
    assert (again[0] == first[0]).all() and (again[1] == first[1]).all()
    ys, proofs = setup.open_all(p, 16)                             # the key (4, 0) replaces (4, 2)
    assert table_ms() > 0 and bp.scalars_to_ints(ys) == want_ys and [bytes(x) for x in proofs] == want_all
    ys2, proofs2 = setup.open_all(p, 16)
    assert table_ms() == 0 and (ys2 == ys).all() and (proofs2 == proofs).all()
    back = setup.open_cosets(p, 4, 16)                             # and (4, 2) again
    assert table_ms() > 0 and (back[0] == first[0]).all() and (back[1] == first[1]).all()
    check(setup.open_cosets(p, 2, 16), *want2)                     # another cell size at the same n is another key
    assert table_ms() > 0
    check(setup.open_cosets(p, 2, 16), *want2)
    assert table_ms() == 0
    other = bp.Setup.generate_srs(16, TAU, ctx, tables=False)      # explicit prepare == none
    other.prepare_open_cosets(16, 4)
    prepared = other.open_cosets(p, 4, 16)
    assert table_ms() == 0 and (prepared[0] == first[0]).all() and (prepared[1] == first[1]).all()
    other.prepare_open_cosets(16, 16)                              # l = n: nothing to prepare, the table stays
    other.open_cosets(p, 4, 16)
    assert table_ms() == 0
    other.prepare_open_cosets(16, 1)                               # l = 1 is prepare_open_all
    other.open_all(p, 16)
    assert table_ms() == 0
    for h in (other.handle, setup.handle):
        ctx.srs_free(h)                                            # bp_srs_free with a table attached succeeds
    with pytest.raises(bp.BpError):
        ctx.srs_len(setup.handle)


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_output_untouched(ctx, setups):
    setup = setups(16)
    lag = ctx.srs_lagrange(setup.handle, 3)
    f = list(range(1, 9))
    try:
        cases = {"log_l > log_n": (setup.handle, f, BASIS_MONOMIAL, 3, 4, -1),
                 "Lagrange SRS handle": (lag, f, BASIS_MONOMIAL, 3, 1, -5),
                 "n - l > srs_len": (setup.handle, f, BASIS_MONOMIAL, 5, 3, -6),
                 "n_values > n": (setup.handle, f + [1], BASIS_MONOMIAL, 3, 1, -6),
                 "Lagrange input of the wrong length": (setup.handle, f[:7], BASIS_LAGRANGE, 3, 1, -6),
                 "log_n = 24": (setup.handle, f, BASIS_MONOMIAL, 24, 6, -10),
                 "a byte scalar >= q": (setup.handle, f[:7] + [Q], BASIS_MONOMIAL, 3, 1, -4),
                 "a byte scalar >= q, one cell": (setup.handle, f[:7] + [Q], BASIS_MONOMIAL, 3, 3, -4),
                 "unknown handle": (0xDEAD, f, BASIS_MONOMIAL, 3, 1, -1)}
        for name, (handle, ints, basis, log_n, log_l, code) in cases.items():
            rc, _, proofs, vals = raw(ctx, handle, ints, basis, log_n, log_l, fill=0xA5)
            assert rc == code, (name, rc)
            assert (vals == 0xA5).all() and (proofs == 0xA5).all(), name
            if not name.startswith("a byte scalar"):               # the device entry takes Montgomery limbs: no such thing as a value >= q
                d = dev(ctx, [v % Q for v in ints])
                rc = ctx._lib.bp_kzg_open_cosets_device(ctx._h, handle, d._ptr(), len(ints), basis, log_n, log_l, vals.ctypes.data, proofs.ctypes.data)
                assert rc == code and (vals == 0xA5).all() and (proofs == 0xA5).all(), name
        out = np.full(96, 0xA5, dtype=np.uint8)
        src = np.zeros(64, dtype=np.uint8)
        lib, h = ctx._lib, setup.handle
        assert lib.bp_kzg_open_cosets(ctx._h, h, src.ctypes.data, 1, BASIS_MONOMIAL, 7, 1, 1, None, out.ctypes.data) == -1      # bad format
        assert lib.bp_kzg_open_cosets(ctx._h, h, src.ctypes.data, 1, 9, FR_MONT, 1, 1, None, out.ctypes.data) == -1              # bad basis
        assert lib.bp_kzg_open_cosets(ctx._h, h, None, 1, BASIS_MONOMIAL, FR_MONT, 1, 1, None, out.ctypes.data) == -1            # null polynomial
        assert lib.bp_kzg_open_cosets(ctx._h, h, src.ctypes.data, 1, BASIS_MONOMIAL, FR_MONT, 1, 1, None, None) == -1            # null output
        assert lib.bp_srs_open_cosets_prepare(ctx._h, h, 3, 4) == -1 and lib.bp_srs_open_cosets_prepare(ctx._h, h, 5, 3) == -6
        assert lib.bp_srs_open_cosets_prepare(ctx._h, lag, 3, 1) == -5 and lib.bp_srs_open_cosets_prepare(ctx._h, h, 24, 6) == -10
        assert (out == 0xA5).all()
    finally:
        ctx.srs_free(lag)


# ---- 8. a group context ------------------------------------------------------------------------------------------------------------------------
def test_group_context(ctx, setups):
    """a two-member rehearsal context {0, 0}: the SRS is sharded, the points are collected on the primary device; the bytes of the
    plain context"""
    n, l, rng = 16, 4, random.Random(16)
    f = [rng.randrange(Q) for _ in range(n)]
    want = model(f, n, l)
    plain = setups(n).open_cosets(host(ctx, f), l, n)
    check(plain, *want)
    many = bp.Context([0, 0])
    try:
        assert many.n_shards() == 2
        setup = bp.Setup.generate_srs(n, TAU, many, tables=False)
        for p in (host(many, f), dev(many, f)):
            got = setup.open_cosets(p, l, n)
            assert (got[0] == plain[0]).all() and (got[1] == plain[1]).all()
        natural = [K.horner(f, z) for z in K.domain(n)]
        check(setup.open_cosets(host(many, natural, BASIS_LAGRANGE), l), *want)
        many.srs_free(setup.handle)
    finally:
        many.close()

"""-m gpu: the structure of an SRS -- bp_srs_powers_reduce against its closed form byte for byte, bp_srs_check_powers on clean,
broken, spliced and mislabelled powers of tau (with the bound on its reduces and pairings), and bp_srs_adopt_lagrange on exported
Lagrange points.  Expected values: Python integers, turned into points by O.g1_mul as the neighbouring tests do; broken inputs
are made from exports of generated SRSs (bp_srs_generate / bp_srs_lagrange have their own tests)."""
import random

import numpy as np
import pytest

import baby_plonk_rust_amd as bp
from baby_plonk_rust_amd import BASIS_LAGRANGE, BASIS_MONOMIAL
from oracle import oracle as O
from tests import bigint_model as M

pytestmark = pytest.mark.gpu
Q = M.Q
TAU, TAU2 = 0x1F2E3D4C5B6A7988776655, 0x5EED5EED5EED
RHO = (1 << 127) | 0x1234567890ABCDEF1234567890ABCDE
PROG_A, PROG_D = 0x1234567, 0xABCDEF01
ID96 = M.enc96(None)


def g1_bytes(k):
    """k G as a 96-byte record"""
    return ID96 if k % Q == 0 else bytes(O.g1_bytes96(O.g1_mul(O.g1_generator(), O.fr_from_int(k % Q))))


OTHER96 = g1_bytes(0xC0FFEE)                                    # a subgroup point that belongs to no SRS here
INVALID_ARG, BAD_POINT, BAD_SCALAR, BASIS, LENGTH, TOO_LARGE = -1, -3, -4, -5, -6, -10


@pytest.fixture(scope="module")
def ctx():
    c = bp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def group():
    c = bp.Context([0, 0])
    yield c
    c.close()


def code_of(fn):
    with pytest.raises(bp.BpError) as e:
        fn()
    return e.value.code


def ceil_log2(n):
    return (n - 1).bit_length() if n > 1 else 0


def powers_bytes(ctx, n, tau):
    h = ctx.srs_generate(n, tau)
    try:
        return ctx.srs_export(h)
    finally:
        ctx.srs_free(h)


def replaced(points96, at, record=OTHER96):
    return points96[:96 * at] + record + points96[96 * (at + 1):]


def setup_of(ctx, points96, tau=TAU, tables=False):
    return bp.Setup.from_points(points96, ctx, tables=tables, x_2=bp.g2_mul_generator(tau))


def within_bound(ctx, length):
    st = ctx.srs_check_stats()
    return 1 <= st["reduces"] <= 2 + ceil_log2(length) and st["reduces"] == st["pairings"]


# ---- bp_srs_powers_reduce ------------------------------------------------------------------------------------------------------------
def reduce_closed_form(first, n_pairs, rho=RHO):
    """A = (sum rho^i k_{first+i}) G and B = (sum rho^i k_{first+i+1}) G for the progression k_j = a + j d"""
    ka = kb = 0
    r = 1
    for i in range(n_pairs):
        ka = (ka + r * (PROG_A + (first + i) * PROG_D)) % Q
        kb = (kb + r * (PROG_A + (first + i + 1) * PROG_D)) % Q
        r = r * rho % Q
    return g1_bytes(ka), g1_bytes(kb)


@pytest.mark.parametrize("length, first, n_pairs", [(2, 0, 1), (3, 1, 1), (65, 0, 64), (65, 7, 50)])
def test_reduce_is_its_closed_form(ctx, length, first, n_pairs):
    h = ctx.srs_generate_progression(length, PROG_A, PROG_D)
    assert ctx.srs_powers_reduce(h, RHO, first, n_pairs) == reduce_closed_form(first, n_pairs)
    assert ctx.srs_powers_reduce(h, 2, first, n_pairs) == reduce_closed_form(first, n_pairs, 2)
    assert ctx.srs_powers_reduce(h, Q - 1, first, n_pairs) == reduce_closed_form(first, n_pairs, Q - 1)
    ctx.srs_free(h)


@pytest.mark.parametrize("which", ["single", "group"])
def test_reduce_at_2p14_without_and_with_tables(ctx, group, which):
    """2^14 + 1 points: the MSM at first = 1 (and at 4) starts inside the SRS, on the raw points and then on the table path"""
    c = ctx if which == "single" else group
    n = (1 << 14) + 1
    h = c.srs_generate_progression(n, PROG_A, PROG_D)
    want = {(0, 1 << 14): reduce_closed_form(0, 1 << 14), (3, 1 << 13): reduce_closed_form(3, 1 << 13)}
    for tables in (False, True):
        if tables:
            assert c.srs_precompute(h)["windows"] > 0
        for (first, n_pairs), pair in want.items():
            assert c.srs_powers_reduce(h, RHO, first, n_pairs) == pair, (tables, first, n_pairs)
            assert c.msm_stats()["tables"] == tables
    c.srs_free(h)


def test_reduce_edges_and_refusals(ctx):
    h = ctx.srs_generate_progression(9, PROG_A, PROG_D)
    assert ctx.srs_powers_reduce(h, RHO, 0, 0) == (ID96, ID96) and ctx.srs_powers_reduce(h, RHO, 8, 0) == (ID96, ID96)
    assert ctx.srs_powers_reduce(h, RHO) == reduce_closed_form(0, 8)
    for first, n_pairs in ((0, 9), (1, 8), (8, 1), (9, 0), (2**63, 2**63)):
        assert code_of(lambda: ctx.srs_powers_reduce(h, RHO, first, n_pairs)) == INVALID_ARG
    for rho in (0, 1):
        assert code_of(lambda: ctx.srs_powers_reduce(h, rho, 0, 8)) == INVALID_ARG
    for rho in (Q, Q + 5, 2**256 - 1):
        assert code_of(lambda: ctx.srs_powers_reduce(h, rho, 0, 8)) == BAD_SCALAR
    assert code_of(lambda: ctx.srs_powers_reduce(h + 1000, RHO, 0, 1)) == INVALID_ARG
    lag = ctx.srs_lagrange(h, 3)
    assert code_of(lambda: ctx.srs_powers_reduce(lag, RHO, 0, 7)) == BASIS
    assert code_of(lambda: ctx.srs_check_powers(lag, bp.g2_mul_generator(TAU), RHO)) == BASIS
    ctx.srs_free(lag)
    ctx.srs_free(h)


# ---- bp_srs_check_powers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [1, 2, 3, 65, 1024, (1 << 14) + 1])
def test_clean_powers_pass_with_one_reduce_and_one_pairing(ctx, length):
    setup = bp.Setup.generate_srs(length, TAU, ctx, tables=length > 1024)
    assert setup.check_powers(RHO) is None and setup.check_powers() is None
    st = ctx.srs_check_stats()
    assert (st["reduces"], st["pairings"]) == ((1, 1) if length > 1 else (0, 0)) and st["ms"] > 0
    bad = np.zeros(1, dtype=np.uint64)                           # the C entry itself: BP_OK leaves SIZE_MAX
    import ctypes as C
    r = np.frombuffer(RHO.to_bytes(32, "little"), dtype=np.uint8).copy()
    x2 = np.frombuffer(setup.x_2, dtype=np.uint8).copy()
    assert ctx._lib.bp_srs_check_powers(ctx._h, setup.handle, x2.ctypes.data, r.ctypes.data, 0, 2, bad.ctypes.data_as(C.POINTER(C.c_size_t))) == 0
    assert int(bad[0]) == 2**64 - 1
    ctx.srs_free(setup.handle)


def test_wrong_x_2_fails_at_the_first_pair(ctx):
    pts = powers_bytes(ctx, 65, TAU)
    setup = setup_of(ctx, pts, TAU + 1)
    assert setup.check_powers(RHO) == 1 and within_bound(ctx, 65)
    assert setup_of(ctx, pts, TAU).check_powers(RHO) is None
    no_x2 = bp.Setup.from_points(pts, ctx, tables=False)
    assert code_of(no_x2.check_powers) == INVALID_ARG


def test_x_2_rules(ctx):
    pts = powers_bytes(ctx, 4, TAU)
    h = ctx.srs_load(pts)
    assert code_of(lambda: ctx.srs_check_powers(h, bytes([0x40]) + bytes(191), RHO)) == INVALID_ARG      # the identity
    off = bytearray(bp.g2_mul_generator(TAU))
    off[191] ^= 1
    assert code_of(lambda: ctx.srs_check_powers(h, bytes(off), RHO)) == BAD_POINT                         # not on the curve
    assert code_of(lambda: ctx.srs_check_powers(h, bp.g2_mul_generator(TAU), 1)) == INVALID_ARG
    assert code_of(lambda: ctx.srs_check_powers(h, bp.g2_mul_generator(TAU), Q)) == BAD_SCALAR
    ctx.srs_free(h)


def test_generator_flag(ctx):
    """P_i = 2 tau^i G is consistent with x_2 = tau G2 but does not start at the generator"""
    n = 6
    pts = b"".join(g1_bytes(2 * pow(TAU, i, Q)) for i in range(n))
    setup = setup_of(ctx, pts)
    assert setup.check_powers(RHO, generator=True) == 0
    assert setup.check_powers(RHO, generator=False) is None
    assert setup_of(ctx, powers_bytes(ctx, n, TAU)).check_powers(RHO, generator=True) is None


@pytest.mark.parametrize("length", [3, 65, 1024])
def test_one_replaced_point_is_located(ctx, length):
    pts = powers_bytes(ctx, length, TAU)
    for j in sorted({1, length // 2, length - 1}):
        setup = setup_of(ctx, replaced(pts, j), tables=length == 1024)
        assert setup.check_powers(RHO) == j, j
        assert within_bound(ctx, length)
        ctx.srs_free(setup.handle)
    setup = setup_of(ctx, replaced(pts, 0))                      # P_0 replaced: the generator test sees it, without it pair 0 fails
    assert setup.check_powers(RHO) == 0 and setup.check_powers(RHO, generator=False) == 1


def test_a_splice_fails_only_at_the_seam(ctx):
    length, j = 65, 33
    a, b = powers_bytes(ctx, length, TAU), powers_bytes(ctx, length, TAU2)
    spliced = a[:96 * j] + b[96 * j:]
    assert setup_of(ctx, spliced, TAU).check_powers(RHO) == j and within_bound(ctx, length)
    # relative to the second tau the seam is the same pair; the pairs in front of it fail too
    assert setup_of(ctx, spliced, TAU2).check_powers(RHO) == 1
    # only the pair j - 1 fails: the ranges on either side of it reduce to pairs that hold
    h = ctx.srs_load(spliced)
    assert bp.pairing_check([ctx.srs_powers_reduce(h, RHO, 0, j - 1)], bp.g2_mul_generator(TAU), host=True) == [True]
    assert bp.pairing_check([ctx.srs_powers_reduce(h, RHO, j, length - 1 - j)], bp.g2_mul_generator(TAU2), host=True) == [True]
    assert bp.pairing_check([ctx.srs_powers_reduce(h, RHO, j - 1, 1)], bp.g2_mul_generator(TAU), host=True) == [False]
    ctx.srs_free(h)
    truncated = a[:96 * 40]                                      # a truncated file is a shorter clean SRS
    assert setup_of(ctx, truncated).check_powers(RHO) is None


def test_two_breaks_report_the_lower(ctx):
    length = 1024
    pts = powers_bytes(ctx, length, TAU)
    for lo, hi in ((5, 900), (511, 512), (1, 1023)):
        assert setup_of(ctx, replaced(replaced(pts, hi), lo)).check_powers(RHO) == lo
        assert within_bound(ctx, length)


def test_group_context_checks_across_the_shard_boundary(group):
    length = 1024
    pts = powers_bytes(group, length, TAU)
    assert group.n_shards() == 2
    clean = setup_of(group, pts)
    assert clean.check_powers(RHO) is None
    st = group.srs_check_stats()
    assert (st["reduces"], st["pairings"]) == (1, 1)
    for j in (length // 2, length // 2 - 1):
        assert setup_of(group, replaced(pts, j)).check_powers(RHO) == j
        assert within_bound(group, length)


# ---- bp_srs_adopt_lagrange -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lagrange_sets(ctx):
    """per n: (powers Setup, its computed Lagrange Setup, the exported Lagrange records)"""
    out = {}
    for n in (1, 2, 64, 1024):
        powers = bp.Setup.generate_srs(n + 6, TAU, ctx, tables=False)
        lag = powers.lagrange(n, tables=False)
        out[n] = (powers, lag, lag.powers_of_x())
    return out


@pytest.mark.parametrize("n", [1, 2, 64, 1024])
def test_adopted_points_are_a_lagrange_srs(ctx, lagrange_sets, n):
    powers, lag, L = lagrange_sets[n]
    adopted = bp.Setup.from_lagrange_points(L, powers, RHO, tables=False)
    st = ctx.srs_check_stats()
    assert (st["reduces"], st["pairings"]) == (1, 0)
    assert ctx.srs_basis(adopted.handle) == (BASIS_LAGRANGE, n.bit_length() - 1) and ctx.srs_len(adopted.handle) == n
    assert adopted.powers_of_x() == L and adopted.x_2 == powers.x_2 and adopted.handle != lag.handle
    assert ctx.srs_basis(powers.handle) == (BASIS_MONOMIAL, 0) and powers.powers_of_x()[:96] == g1_bytes(1)      # sources untouched
    rnd = random.Random(n)
    poly = bp.Polynomial(bp.scalars_from_ints([rnd.randrange(Q) for _ in range(n)]), BASIS_LAGRANGE, ctx)
    commitment = adopted.commit(poly)
    assert commitment == lag.commit(poly)
    z = bp.scalar_from_int(rnd.randrange(Q))
    ys, proof = adopted.open(poly, z)
    assert adopted.verify_openings(bp.Opening(commitment, z, ys, None, proof))
    assert bp.Setup.from_lagrange_points(L, powers, tables=False).powers_of_x() == L             # rho drawn inside
    if n >= 64:                                                   # the compressed records of the same points
        again = bp.Setup.from_lagrange_points(lag.powers_of_x_compressed(), powers, RHO, tables=n == 1024, compressed=True)
        assert again.powers_of_x() == L and again.basis == BASIS_LAGRANGE and again.commit(poly) == commitment


def adopt_index(fn):
    with pytest.raises(bp.BpError) as e:
        fn()
    assert e.value.code == BAD_POINT
    return e.value.index


@pytest.mark.parametrize("n", [2, 64, 1024])
def test_wrong_lagrange_points_are_located_and_make_no_handle(ctx, lagrange_sets, n):
    powers, _, L = lagrange_sets[n]
    handles_before = len(ctx_handles(ctx, powers))
    for j in sorted({0, n // 2, n - 1}):
        assert adopt_index(lambda: bp.Setup.from_lagrange_points(replaced(L, j), powers, RHO, tables=False)) == j
        st = ctx.srs_check_stats()
        assert st["reduces"] <= 2 + ceil_log2(n) and st["pairings"] == 0
    a, b = (0, 1) if n == 2 else (n // 4, n // 2 + 3)
    swapped = replaced(replaced(L, a, L[96 * b: 96 * b + 96]), b, L[96 * a: 96 * a + 96])
    assert adopt_index(lambda: bp.Setup.from_lagrange_points(swapped, powers, RHO, tables=False)) == a
    assert len(ctx_handles(ctx, powers)) == handles_before        # nothing adopted, the intermediate handles freed


def ctx_handles(ctx, powers):
    """the SRS handles alive on the context, probed: handles are small consecutive integers"""
    alive = []
    for h in range(1, powers.handle + 4096):
        try:
            ctx.srs_len(h)
            alive.append(h)
        except bp.BpError:
            pass
    return alive


def test_adopt_refusals(ctx, lagrange_sets):
    powers, lag, L = lagrange_sets[64]
    pts = ctx.srs_load(L)
    before = ctx_handles(ctx, powers)
    assert code_of(lambda: ctx.srs_adopt_lagrange(pts, powers.handle, 5, RHO)) == LENGTH              # 64 points, log_n = 5
    assert code_of(lambda: ctx.srs_adopt_lagrange(pts, powers.handle, 7, RHO)) == LENGTH
    short = ctx.srs_generate(63, TAU)
    assert code_of(lambda: ctx.srs_adopt_lagrange(pts, short, 6, RHO)) == INVALID_ARG                 # powers too short
    assert code_of(lambda: ctx.srs_adopt_lagrange(lag.handle, powers.handle, 6, RHO)) == BASIS        # a Lagrange source on either side
    assert code_of(lambda: ctx.srs_adopt_lagrange(pts, lag.handle, 6, RHO)) == BASIS
    assert code_of(lambda: ctx.srs_adopt_lagrange(pts, powers.handle, 25, RHO)) == TOO_LARGE
    assert code_of(lambda: ctx.srs_adopt_lagrange(pts, powers.handle, 6, 1)) == INVALID_ARG
    assert code_of(lambda: ctx.srs_adopt_lagrange(pts, powers.handle, 6, Q)) == BAD_SCALAR
    ctx.srs_free(short)
    assert ctx_handles(ctx, powers) == before
    assert code_of(lambda: bp.Setup.from_lagrange_points(L[:96 * 48], powers)) == -2                  # 48 points
    ctx.srs_free(pts)


def test_group_context_adopts(group):
    n = 64
    powers = bp.Setup.generate_srs(n, TAU, group, tables=False)
    lag = powers.lagrange(n, tables=False)
    L = lag.powers_of_x()
    adopted = bp.Setup.from_lagrange_points(L, powers, RHO, tables=False)
    assert adopted.powers_of_x() == L and group.srs_basis(adopted.handle) == (BASIS_LAGRANGE, 6)
    assert adopt_index(lambda: bp.Setup.from_lagrange_points(replaced(L, n // 2), powers, RHO, tables=False)) == n // 2

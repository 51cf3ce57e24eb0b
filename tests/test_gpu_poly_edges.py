"""-m gpu: the Polynomial layer (csrc/poly.hip, poly_kernels.hpp, capi_poly.hip) at
the edges of its dispatch: every division path at its thresholds (Context.poly_stats() says which one ran), evaluation across the
K = 16 -> 32 switch and past 256 partials, products at the single-pass / multi-pass transform edge, the device entry points across
workgroup edges, with unequal lengths and in place, the grand product past 256 scan tiles, and canonical-byte vectors holding a
value >= q.

Results are bit-exact Montgomery limbs: no tolerances.  Every expected value comes from Python integers, from the CPU oracle or
from construction (a dividend is BUILT from a known quotient); none from another GPU call.

Times on an MI355X, one run of this file together with tests/test_gpu_poly.py (pytest --durations=0; 98 tests in 7.9 s; the slowest
existing case, test_gpu_poly.py::test_mul_literals_and_random, took 0.03 s; what is not listed took less than 0.03 s):

    0.49 s  test_evaluate_sizes[4194304-host], [4194305-host]            the oracle's evaluation of 2^22 coefficients + a 134 MB upload
    0.45 s  test_division_...named_path[2228229x17-host-exact]           build + the oracle's long division (the second witness)
    0.42 s  test_division_...named_path[2097157x16-host-exact]           the same
    0.39 s  test_division_...named_path[2097153x1-host-exact]            the same
    0.36 s  test_division_...named_path[8390657x4097-host-exact]         build of 8.4 M coefficients (268 MB per array), no oracle
    0.32 s  setup of the grand-product columns (once for both tests)     2^20 roots and their multiples on the CPU
    0.26 s  test_evaluate_special_points_past_the_k_switch               three sums over 4 M Python integers
    0.20 s  test_device_scalar_op_both_bases_and_in_place[70001]         six expectations of 70 001 Python integers
    0.16 s  test_device_scale_powers[70001], test_mul_...[32768-32769]
    0.13 s  test_division_...named_path[8390657x4097-host-remainder]     268 MB up, 268 MB down
    0.10 s  test_division_...named_path[8390657x4097-device-*]
    0.07 - 0.09 s  the two grand products at 2^20, test_device_add_sub...[70001-*]

The shapes of 2 M coefficients and more ran as one test of 0.5 - 0.8 s each at first and were split by entry point and dividend
(and the evaluations by entry point); a shape's first case still pays for the CPU side -- the build, and the oracle's division or
evaluation, which IS the reference -- and that part cannot be split further without shrinking a shape below its threshold.  No GPU
side of a case takes more than 0.13 s.
"""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import baby_plonk_rust_amd as bp
from oracle import oracle as O
from tests.gpu_common import Q

gpu = pytest.mark.gpu
MONO, LAG = bp.BASIS_MONOMIAL, bp.BASIS_LAGRANGE
R = pow(2, 256, Q)
RINV = pow(R, Q - 2, Q)
PERIOD = 4099            # prime, so a tiled vector lines up with no chunk, tile or block size


@pytest.fixture(scope="module")
def ctx():
    return bp.default_context()


# ---------------------------------------------------------------------------------------------- host-side helpers (Python ints)
def mont(vals):
    """canonical integers -> [n, 4] Montgomery limbs"""
    if not len(vals):
        return np.zeros((0, 4), dtype=np.uint64)
    return np.frombuffer(b"".join((v % Q * R % Q).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def ints(a):
    b = np.ascontiguousarray(a, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[i: i + 32], "little") * RINV % Q for i in range(0, len(b), 32)]


def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % Q
    return acc


def dev(ctx, a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4).view(np.int64).copy()).to(torch.device("cuda", ctx.device))
    torch.cuda.synchronize()
    return t


def back(t):
    return t.cpu().numpy().view(np.uint64)


def build_dividend(nq, m, b0, bm, seed, zero_at=()):
    """(a, q): q_i = t[i mod PERIOD] over PERIOD random non-zero scalars (0 at the indices of zero_at), a = q * (b0 + bm x^m), with
    no n log n product on the host: a_k = b0 q_k + bm q_{k-m} is PERIOD-periodic away from the m entries at each end"""
    rnd = random.Random(seed)
    t = [rnd.randrange(1, Q) for _ in range(PERIOD)]
    zero = set(zero_at)
    q_at = lambda i: 0 if i in zero else t[i % PERIOD]
    q = mont(t)[np.arange(nq) % PERIOD]
    a = np.zeros((nq + m, 4), dtype=np.uint64)
    if nq > m:
        u = mont([(b0 * t[k] + bm * t[(k - m) % PERIOD]) % Q for k in range(PERIOD)])
        a[m:nq] = u[np.arange(m, nq) % PERIOD]
    fix = set(range(min(m, nq))) | set(range(max(m, nq), nq + m))
    for z in zero:
        fix |= {z, z + m}
    fix = sorted(fix)
    a[fix] = mont([((b0 * q_at(k) if k < nq else 0) + (bm * q_at(k - m) if k >= m else 0)) % Q for k in fix])
    if zero:
        q[sorted(zero)] = 0
    return a, q


def binomial(m, b0, bm):
    b = np.zeros((m + 1, 4), dtype=np.uint64)
    b[0], b[m] = mont([b0])[0], mont([bm])[0]
    return b


def host_div(ctx, a, b):
    out, n = np.empty((max(len(a), 1), 4), dtype=np.uint64), C.c_size_t()
    ctx.check(ctx._lib.bp_poly_div(ctx._h, a.ctypes.data, len(a), b.ctypes.data, len(b), MONO, bp.FR_MONT, out.ctypes.data, C.byref(n)), "bp_poly_div")
    return out[: n.value]


def dev_div(ctx, a, b):
    return (bp.DevicePolynomial(a, MONO, ctx) / bp.DevicePolynomial(b, MONO, ctx)).values


def same(got, want):
    return got.shape == want.shape and bool((got == want).all())


# ---------------------------------------------------------------------------------------------- the builder itself (no GPU)
@pytest.mark.parametrize("nq,m", [(97, 3), (10243, 5), (131073, 1), (2, 8)])
def test_dividend_builder_against_the_oracle_division(nq, m):
    rnd = random.Random(1000 * nq + m)
    b0, bm = rnd.randrange(1, Q), rnd.randrange(2, Q)
    a, q = build_dividend(nq, m, b0, bm, seed=nq + m)
    assert len(a) == nq + m and len(q) == nq and not (q == 0).all(axis=1).any()
    assert same(O.poly_binop("poly_div", a, binomial(m, b0, bm)), q)            # the quotient has no zero coefficient: *n_out == nq
    if nq == 97:                                                                  # and against the schoolbook product in Python ints
        qi, want = ints(q), [0] * (nq + m)
        for i, v in enumerate(qi):
            want[i] = (want[i] + b0 * v) % Q
            want[i + m] = (want[i + m] + bm * v) % Q
        assert ints(a) == want
        az, qz = build_dividend(nq, m, b0, bm, seed=nq + m, zero_at=(0, 31, 32, nq - 2))
        assert ints(qz) == [0 if i in (0, 31, 32, nq - 2) else v for i, v in enumerate(qi)]
        keep = ~(qz == 0).all(axis=1)
        assert same(O.poly_binop("poly_div", az, binomial(m, b0, bm)), qz[keep])  # the reference squeezes zero coefficients out


# ---------------------------------------------------------------------------------------------- division by a binomial
@functools.lru_cache(maxsize=1)
def division_case(nq, m, b0, bm, seed):
    """(a, a with a remainder, q, b), read-only: built once for the consecutive cases of one shape"""
    a, q = build_dividend(nq, m, b0, bm, seed)
    a2 = a.copy()
    a2[0] = mont([ints(a[:1])[0] + 1])[0]                     # a non-zero remainder: the quotient is the same
    case = (a, a2, q, binomial(m, b0, bm))
    for x in case:
        x.setflags(write=False)
    return case


@pytest.fixture(scope="module", autouse=True)
def drop_cached_cases():
    yield
    division_case.cache_clear()
    evaluation_case.cache_clear()


ENTRIES = [(entry, dividend) for entry in ("host", "device") for dividend in ("exact", "remainder")]


def check_division(ctx, nq, m, b0, bm, path, segments, witness, seed, entries=ENTRIES):
    a, a2, q, b = division_case(nq, m, b0, bm, seed)
    want_stats = {"div_path": path, "chunks": (-(-nq // m) + 31) // 32, "segments": segments}
    for entry, dividend in entries:
        if witness and (entry, dividend) == ("host", "exact"):
            assert same(O.poly_binop("poly_div", a, b), q)
        got = (host_div if entry == "host" else dev_div)(ctx, a if dividend == "exact" else a2, b)
        assert ctx.poly_stats() == want_stats
        assert same(got, q), "%s, %s: first mismatches at %s" % (
            entry, dividend, np.nonzero((got != q).any(axis=1))[0][:4] if got.shape == q.shape else got.shape)


# nq, m, div_path, segments G, second witness (the oracle's long division)
DIV_SHAPES = [
    (2, 8, 1, 0, True),                     # one chunk; lanes r >= nq
    (96, 3, 1, 0, True),                    # one chunk, max_len == 32
    (97, 3, 2, 0, True),                    # plain carry; chains 1 and 2 end in an empty chunk
    (2048, 1, 2, 0, True),                  # plain carry, upper edge (64 chunks)
    (2049, 1, 3, 0, True),                  # workgroup carry, lower edge (65 chunks)
    (10243, 5, 3, 0, True),                 # workgroup carry, unequal chains
    (32768, 1, 3, 0, True),                 # workgroup carry, 1024 chunks: S = 1
    (32769, 1, 3, 0, True),                 # 1025 chunks: S = 2
    (131072, 1, 3, 0, True),                # workgroup carry, upper edge (4096 chunks)
    (131073, 1, 4, 5, True),                # segmented, G = 5
    (2097157, 16, 4, 5, True),              # segmented with m at its edge: 5 long + 11 short chains
    (2228229, 17, 3, 0, True),              # m > 16: workgroup carry with S = 5
    ((1 << 21) + 1, 1, 4, 64, True),        # segmented, G clamped to 64, S = 2 inside a segment
    (2048 * 4097 + 1, 4097, 2, 0, False),   # m > 4096: plain carry over 65 chunks (the oracle walks 4098 slots per step: minutes)
]
# the shapes of 2 M coefficients and more run one case per entry point and dividend (the first pays for the build and the witness)
DIV_CASES = [(s, [e]) for s in DIV_SHAPES if s[0] > (1 << 20) for e in ENTRIES] + [(s, ENTRIES) for s in DIV_SHAPES if s[0] <= (1 << 20)]
DIV_CASES.sort(key=lambda c: DIV_SHAPES.index(c[0]))


@gpu
@pytest.mark.parametrize("shape,entries", DIV_CASES,
                         ids=["%dx%d%s" % (s[0], s[1], "-%s-%s" % e[0] if len(e) == 1 else "") for s, e in DIV_CASES])
def test_division_by_a_random_binomial_takes_the_named_path(ctx, shape, entries):
    nq, m, path, segments, witness = shape
    rnd = random.Random(7 * nq + m)
    check_division(ctx, nq, m, rnd.randrange(1, Q), rnd.randrange(2, Q), path, segments, witness, seed=nq ^ m, entries=entries)


@gpu
@pytest.mark.parametrize("nq,m,path,segments", [(97, 3, 2, 0), (2049, 1, 3, 0), (131073, 1, 4, 5)])
@pytest.mark.parametrize("kind", ["c_x^m", "x^m-1", "x^m+1"])
def test_division_by_special_binomials(ctx, nq, m, path, segments, kind):
    """f = -b0 / bm is 0, 1 and -1"""
    rnd = random.Random(nq)
    b0, bm = {"c_x^m": (0, rnd.randrange(2, Q)), "x^m-1": (Q - 1, 1), "x^m+1": (1, 1)}[kind]
    if kind == "c_x^m" and nq == 97:                            # a[m:] / bm in Python ints
        a, _, q, _ = division_case(nq, m, b0, bm, 5)
        inv = pow(bm, Q - 2, Q)
        assert [v * inv % Q for v in ints(a[m:])] == ints(q) and ints(a[:m]) == [0] * m
    check_division(ctx, nq, m, b0, bm, path, segments, True, seed=5)


@gpu
def test_division_squeezes_zero_coefficients_at_chunk_and_segment_edges(ctx):
    """nq = 131073, m = 1: 4097 chunks in 5 segments of 820; zeros at the edges of chunk 0 / 1, of segment 0 / 1 (chunk 820 starts at
    index 26240) and next to the top; what is left comes back in order from both entry points"""
    nq, m = 131073, 1
    zero_at = (0, 31, 32, 26239, 26240, nq - 2)
    rnd = random.Random(77)
    b0, bm = rnd.randrange(1, Q), rnd.randrange(2, Q)
    a, q = build_dividend(nq, m, b0, bm, seed=78, zero_at=zero_at)
    b = binomial(m, b0, bm)
    keep = np.ones(nq, dtype=bool)
    keep[list(zero_at)] = False
    assert int((q == 0).all(axis=1).sum()) == len(zero_at)
    want = q[keep]
    assert same(O.poly_binop("poly_div", a, b), want)
    assert same(host_div(ctx, a, b), want) and ctx.poly_stats()["div_path"] == 4
    assert same(dev_div(ctx, a, b), want) and ctx.poly_stats()["div_path"] == 4


# ---------------------------------------------------------------------------------------------- general long division
def check_general(ctx, a, b, want, path=0):
    assert same(O.poly_binop("poly_div", a, b), want)
    assert same(host_div(ctx, a, b), want)
    if path is not None:
        assert ctx.poly_stats()["div_path"] == path
    assert same(dev_div(ctx, a, b), want)
    if path is not None:
        assert ctx.poly_stats()["div_path"] == path


@gpu
@pytest.mark.parametrize("nb", [1, 3, 1024, 1025, 1026, 2049])
def test_general_division_across_the_stride_loop(ctx, nb):
    """one workgroup of 1024 lanes walks the divisor: nb = 1 (a constant), a middle term, and 1024 / 1025 / 2049 slots (one turn of
    the stride loop, two, three).  Slot nb - 1 only clears the leading term, which nothing reads again, so 1026 is the first size at
    which the second turn decides a coefficient.  50 quotient coefficients keep the sequential loop short"""
    q = O.splitmix_scalars(50, 0x9E0 + nb)
    b = O.splitmix_scalars(nb, 0x9E1 + nb)
    a = O.poly_binop("poly_mul_fast", q, b)
    assert len(a) == 50 + nb - 1
    check_general(ctx, a, b, q)
    if nb == 1:                                                 # a / c in Python ints (a constant leaves no remainder)
        inv = pow(ints(b)[0], Q - 2, Q)
        assert [v * inv % Q for v in ints(a)] == ints(q)
        return
    a2 = a.copy()
    a2[0] = mont([ints(a[:1])[0] + 1])[0]                       # a non-zero remainder: the quotient is the same
    check_general(ctx, a2, b, q)


@gpu
def test_general_division_special_divisors_and_padding(ctx):
    q = O.splitmix_scalars(50, 0xAB1)
    rnd = random.Random(0xAB2)
    b = mont([0, rnd.randrange(1, Q), rnd.randrange(1, Q)])                  # b0 = 0 with a non-zero middle: not a binomial
    check_general(ctx, O.poly_binop("poly_mul_fast", q, b), b, q)
    pad = lambda x, k: np.concatenate([x, np.zeros((k, 4), dtype=np.uint64)])
    b = mont([rnd.randrange(1, Q) for _ in range(5)])
    a = O.poly_binop("poly_mul_fast", q, b)
    check_general(ctx, pad(a, 3), pad(b, 2), q)                              # trailing zeros are trimmed (polynomial.rs:325-339)
    b0, bm = rnd.randrange(1, Q), rnd.randrange(2, Q)                        # a binomial once trimmed
    b = pad(binomial(3, b0, bm), 2)
    a, qb = build_dividend(50, 3, b0, bm, seed=3)
    check_general(ctx, pad(a, 4), b, qb, path=1)
    short = pad(mont([1, 2]), 4)                                             # shorter than the divisor once trimmed: empty
    check_general(ctx, short, mont([1, 2, 3]), np.zeros((0, 4), dtype=np.uint64), path=None)


# ---------------------------------------------------------------------------------------------- evaluation
def evaluate(ctx, c, x_int, entry):
    x, out = mont([x_int])[0], np.zeros(4, dtype=np.uint64)
    if entry == "device":
        return ints(bp.DevicePolynomial(c, MONO, ctx).coeffs_evaluate(x))[0]
    ctx.check(ctx._lib.bp_poly_evaluate(ctx._h, c.ctypes.data, len(c), MONO, x.ctypes.data, bp.FR_MONT, out.ctypes.data), "bp_poly_evaluate")
    return ints(out)[0]


def evaluate_both(ctx, c, x_int):
    return evaluate(ctx, c, x_int, "host"), evaluate(ctx, c, x_int, "device")


@functools.lru_cache(maxsize=1)
def evaluation_case(n):
    """(coefficients, x, p(x) by the oracle), once for the two entry points"""
    c = O.splitmix_scalars(n, 0xE7A1 + n)
    c.setflags(write=False)
    x_int = random.Random(n).randrange(2, Q)
    return c, x_int, ints(O.poly_eval(c, mont([x_int])[0], fast=True))[0]


@gpu
@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4096 * 16 + 1, (1 << 20) + 1, 1 << 22, (1 << 22) + 1])
def test_evaluate_sizes(ctx, n, entry):
    """K = 16 coefficients per lane: n = 15 / 16 / 17 around one lane, 4096 * 16 + 1 a 17th workgroup with one coefficient,
    2^20 + 1 the 257th partial of the final sum, 2^22 the last size with K = 16 and 2^22 + 1 the first with K = 32"""
    c, x_int, want = evaluation_case(n)
    if n <= 17:
        assert want == horner(ints(c), x_int)
    assert evaluate(ctx, c, x_int, entry) == want


@gpu
def test_evaluate_special_points_past_the_k_switch(ctx):
    """n = 2^22 + 1 (K = 32), a PERIOD-periodic coefficient vector: x = 0 gives c_0, x = 1 the sum, x = q - 1 the alternating sum"""
    n = (1 << 22) + 1
    rnd = random.Random(0x5EE)
    t = [rnd.randrange(1, Q) for _ in range(PERIOD)]
    c = mont(t)[np.arange(n) % PERIOD]
    vals = (t * (n // PERIOD + 1))[:n]
    assert evaluate_both(ctx, c, 0) == (t[0], t[0])
    s = sum(vals) % Q
    assert evaluate_both(ctx, c, 1) == (s, s)
    alt = (sum(vals[0::2]) - sum(vals[1::2])) % Q
    assert evaluate_both(ctx, c, Q - 1) == (alt, alt)


@gpu
def test_evaluate_all_coefficients_q_minus_1(ctx):
    """every addition of the Horner steps and of the reductions wraps: -(x^n - 1) / (x - 1) in closed form"""
    n = (1 << 20) + 1
    c = np.tile(mont([Q - 1]), (n, 1))
    x = random.Random(0xA11).randrange(2, Q)
    want = (Q - 1) * (pow(x, n, Q) - 1) * pow(x - 1, Q - 2, Q) % Q
    assert evaluate_both(ctx, c, x) == (want, want)


# ---------------------------------------------------------------------------------------------- multiplication
def check_mul(ctx, a, b):
    want = O.poly_binop("poly_mul_fast", a, b)
    assert len(want) == len(a) + len(b) - 1
    host = (bp.Polynomial(a, MONO, ctx) * bp.Polynomial(b, MONO, ctx)).values
    assert same(host, want)
    assert same((bp.DevicePolynomial(a, MONO, ctx) * bp.DevicePolynomial(b, MONO, ctx)).values, want)
    x = random.Random(len(a)).randrange(2, Q)                    # independent of any transform: p(x) = a(x) b(x) in Python ints
    assert horner(ints(host), x) == horner(ints(a), x) * horner(ints(b), x) % Q


@gpu
@pytest.mark.parametrize("na,nb", [(1, 5000), (2048, 2049), (2048, 2050), (1 << 15, (1 << 15) + 1)])
def test_mul_at_the_transform_edges(ctx, na, nb):
    """a constant factor; product length exactly 2^12 (the largest single-pass transform) and 2^12 + 1 (the first multi-pass one,
    2^13 points); exactly 2^16"""
    check_mul(ctx, O.splitmix_scalars(na, 0x3A + na), O.splitmix_scalars(nb, 0x3B + nb))


@gpu
def test_mul_with_zero_leading_and_trailing_coefficients(ctx):
    """Mul trims nothing (polynomial.rs:272): the zero top coefficients of the product are part of the result"""
    a, b = O.splitmix_scalars(300, 0x3C), O.splitmix_scalars(257, 0x3D)
    a[:3] = 0
    a[-5:] = 0
    b[:1] = 0
    b[-2:] = 0
    check_mul(ctx, a, b)


# ---------------------------------------------------------------------------------------------- element-wise device entry points
SENTINEL = 0x5A5A5A5A5A5A5A5A


def out_buffer(ctx, n):
    import torch
    return torch.full((n + 2, 4), SENTINEL, dtype=torch.int64, device=torch.device("cuda", ctx.device))


def untouched_past(t, n):
    return bool((back(t[n:]) == SENTINEL).all())


@gpu
@pytest.mark.parametrize("nb", [1, 256, 300])
@pytest.mark.parametrize("na", [255, 256, 257, 70001])
def test_device_add_sub_lengths_and_in_place(ctx, na, nb):
    """workgroups of 256: operands that end on a block edge, one short of it, one past it, mid-block, and 274 blocks; the shorter
    operand counts as zero beyond its end (Monomial); Lagrange wants equal lengths (-6); d_out may be the longer operand itself"""
    lib, h = ctx._lib, ctx._h
    a, b = O.splitmix_scalars(na, 0xAD0 + na), O.splitmix_scalars(nb, 0xAD1 + nb)
    ai, bi = ints(a), ints(b)
    n = max(na, nb)
    ai, bi = ai + [0] * (n - na), bi + [0] * (n - nb)
    want = {0: mont([(x + y) % Q for x, y in zip(ai, bi)]), 1: mont([(x - y) % Q for x, y in zip(ai, bi)])}
    fns = {0: lib.bp_poly_add_device, 1: lib.bp_poly_sub_device}
    n_out = C.c_size_t()
    for basis in (MONO, LAG):
        for op in (0, 1):
            da, db, out = dev(ctx, a), dev(ctx, b), out_buffer(ctx, n)
            rc = fns[op](h, da.data_ptr(), na, db.data_ptr(), nb, basis, out.data_ptr(), C.byref(n_out))
            if basis == LAG and na != nb:
                assert rc == -6
                continue
            assert rc == 0 and n_out.value == n
            assert same(back(out[:n]), want[op]) and untouched_past(out, n)
            big = da if na >= nb else db                     # in place on the longer operand
            assert fns[op](h, da.data_ptr(), na, db.data_ptr(), nb, basis, big.data_ptr(), C.byref(n_out)) == 0 and n_out.value == n
            assert same(back(big), want[op])


@gpu
@pytest.mark.parametrize("n", [1, 257, 70001])
def test_device_scalar_op_both_bases_and_in_place(ctx, n):
    """Monomial Add / Sub touch values[0] only (polynomial.rs:62,123), Lagrange Add adds to every value and Lagrange Sub ADDS too
    (the reference's quirk, :126-128); Mul scales every value"""
    lib, h = ctx._lib, ctx._h
    a = O.splitmix_scalars(n, 0x5CA + n)
    ai = ints(a)
    s_int = random.Random(n).randrange(2, Q)
    s = mont([s_int])[0]
    for basis in (MONO, LAG):
        for op in (0, 1, 2):
            if op == 2:
                want = [v * s_int % Q for v in ai]
            elif basis == LAG:
                want = [(v + s_int) % Q for v in ai]
            else:
                want = [(ai[0] + s_int) % Q if op == 0 else (ai[0] - s_int) % Q] + ai[1:]
            want = mont(want)
            da, out = dev(ctx, a), out_buffer(ctx, n)
            assert lib.bp_poly_scalar_op_device(h, da.data_ptr(), n, basis, s.ctypes.data, op, out.data_ptr()) == 0
            assert same(back(out[:n]), want) and untouched_past(out, n)
            assert same(back(da), a)                                                      # the input is left alone
            assert lib.bp_poly_scalar_op_device(h, da.data_ptr(), n, basis, s.ctypes.data, op, da.data_ptr()) == 0
            assert same(back(da), want)                                                   # d_out == d_a


@gpu
@pytest.mark.parametrize("n", [1, 257, 70001])
def test_device_scale_powers(ctx, n):
    lib, h = ctx._lib, ctx._h
    a = O.splitmix_scalars(n, 0x50 + n)
    ai = ints(a)
    w8 = ints(bp.root_of_unity(8))[0]
    assert pow(w8, 8, Q) == 1 and pow(w8, 4, Q) == Q - 1
    for w in (0, 1, w8, random.Random(n).randrange(2, Q)):
        want, p = [], 1
        for v in ai:
            want.append(v * p % Q)
            p = p * w % Q
        da, out = dev(ctx, a), out_buffer(ctx, n)
        wm = mont([w])[0]
        assert lib.bp_poly_scale_powers_device(h, da.data_ptr(), n, wm.ctypes.data, out.data_ptr()) == 0
        assert same(back(out[:n]), mont(want)) and untouched_past(out, n)


# ---------------------------------------------------------------------------------------------- grand product past 256 scan tiles
GP_N = 1 << 20


@pytest.fixture(scope="module")
def gp_columns():
    """witness columns and the identity permutation sigma_j = k_j w^i (k = 1, 2, 3) over 2^20 rows; roots from the CPU oracle, the
    multiples 2 w^i and 3 w^i by limb-wise additions there (the Montgomery map is linear)"""
    n = GP_N
    roots = O.u64((n, 4))
    O.lib.ntt_roots_of_unity(O._p(roots), n)
    two = O.poly_binop("poly_add", roots, roots)
    three = O.poly_binop("poly_add", two, roots)
    assert ints(roots[:2]) == [1, ints(bp.root_of_unity(n))[0]] and ints(three[1:2])[0] == 3 * ints(roots[1:2])[0] % Q
    wit = [O.splitmix_scalars(n, seed) for seed in (0x6A, 0x6B, 0x6C)]
    for col in (roots, two, three, *wit):
        col.setflags(write=False)
    return wit, (roots, two, three)


def grand_product_both(ctx, wit, sig, beta, gamma):
    bm, gm = mont([beta])[0], mont([gamma])[0]
    host = bp.round_2_z(*wit, *sig, bm, gm, ctx=ctx)
    d = [bp.DevicePolynomial(x, LAG, ctx) for x in (*wit, *sig)]
    return host, bp.round_2_z_device(*d, bm, gm).values


@gpu
def test_grand_product_2p20_identity_permutation(ctx, gp_columns):
    """512 tiles of 2048: the scan of the tile products runs two tiles per lane.  Every numerator equals its denominator, so z is
    all ones -- only if every tile prefix times its suffix is the total"""
    wit, sig = gp_columns
    want = np.tile(mont([1]), (GP_N, 1))
    host, device = grand_product_both(ctx, wit, sig, 0xBE7A0123456789, 0x6A33A987654321)
    assert same(host, want), np.nonzero((host != want).any(axis=1))[0][:4]
    assert same(device, want), np.nonzero((device != want).any(axis=1))[0][:4]


@gpu
def test_grand_product_2p20_one_two_cycle(ctx, gp_columns):
    """(a, row 5) and (c, row n - 3) swapped, equal witness values there: z = 1 up to row 5, the ratio
    (a_5 + beta w^5 + gamma) / (a_5 + beta 3 w^(n-3) + gamma) on rows 6 .. n - 3 (carried across ~510 tiles), 1 after"""
    n = GP_N
    (a, b, c), (s1, s2, s3) = gp_columns
    c, s1, s3 = c.copy(), s1.copy(), s3.copy()
    c[n - 3] = a[5]
    s1[5], s3[n - 3] = s3[n - 3].copy(), s1[5].copy()
    beta, gamma = 0xBE7A0123456789, 0x6A33A987654321
    a5, w5, w3 = ints(a[5:6])[0], ints(s1[5:6])[0], ints(s3[n - 3: n - 2])[0]
    assert w3 == pow(ints(bp.root_of_unity(n))[0], 5, Q) and w5 == 3 * pow(ints(bp.root_of_unity(n))[0], n - 3, Q) % Q
    rho = (a5 + beta * w3 + gamma) * pow(a5 + beta * w5 + gamma, Q - 2, Q) % Q
    want = np.tile(mont([1]), (n, 1))
    want[6: n - 2] = mont([rho])[0]
    host, device = grand_product_both(ctx, (a, b, c), (s1, s2, s3), beta, gamma)
    assert same(host, want), np.nonzero((host != want).any(axis=1))[0][:4]
    assert same(device, want), np.nonzero((device != want).any(axis=1))[0][:4]


# ---------------------------------------------------------------------------------------------- canonical bytes >= q
def le(vals):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint8).copy()


def canonical_calls(ctx, v300, v256):
    """return codes of every host entry point that takes a BP_FR_BYTES_LE vector, fed v300 (v256 where a power of two is needed)"""
    lib, h, fmt = ctx._lib, ctx._h, bp.FR_BYTES_LE
    rnd = random.Random(300)
    A, V = le(v300), le(v256)
    S, L = le([rnd.randrange(1, Q) for _ in range(7)]), le([rnd.randrange(1, Q) for _ in range(600)])
    x = le([12345])
    out, r32, n = np.zeros(32 * 1024, dtype=np.uint8), np.zeros(32, dtype=np.uint8), C.c_size_t()
    p = lambda arr: arr.ctypes.data
    rc = {}
    rc["add a"] = lib.bp_poly_add(h, p(A), 300, p(S), 7, MONO, fmt, p(out), C.byref(n))
    rc["add b"] = lib.bp_poly_add(h, p(S), 7, p(A), 300, MONO, fmt, p(out), C.byref(n))
    rc["sub a"] = lib.bp_poly_sub(h, p(A), 300, p(S), 7, MONO, fmt, p(out), C.byref(n))
    rc["sub b"] = lib.bp_poly_sub(h, p(L), 600, p(A), 300, MONO, fmt, p(out), C.byref(n))
    rc["add lagrange"] = lib.bp_poly_add(h, p(A), 300, p(A), 300, LAG, fmt, p(out), C.byref(n))
    rc["scalar_op"] = lib.bp_poly_scalar_op(h, p(A), 300, LAG, p(x), 2, fmt, p(out))
    rc["scalar_op monomial add"] = lib.bp_poly_scalar_op(h, p(A), 300, MONO, p(x), 0, fmt, p(out))
    rc["mul a"] = lib.bp_poly_mul(h, p(A), 300, p(S), 7, MONO, fmt, p(out), C.byref(n))
    rc["mul b"] = lib.bp_poly_mul(h, p(S), 7, p(A), 300, MONO, fmt, p(out), C.byref(n))
    rc["div dividend"] = lib.bp_poly_div(h, p(A), 300, p(S), 7, MONO, fmt, p(out), C.byref(n))
    rc["div dividend, binomial"] = lib.bp_poly_div(h, p(A), 300, p(le([5, 0, 0, 7])), 4, MONO, fmt, p(out), C.byref(n))
    rc["div divisor"] = lib.bp_poly_div(h, p(L), 600, p(A), 300, MONO, fmt, p(out), C.byref(n))
    rc["evaluate"] = lib.bp_poly_evaluate(h, p(A), 300, MONO, p(x), fmt, p(r32))
    # grand product over 256 rows, identity permutation (valid for any witness): the vector is the witness a, then sigma_3
    w = ints(bp.root_of_unity(256))[0]
    roots = [pow(w, i, Q) for i in range(256)]
    cols = [le([rnd.randrange(1, Q) for _ in range(256)]) for _ in range(3)] + [le([k * v % Q for v in roots]) for k in (1, 2, 3)]
    scal = [le([v]) for v in (0xBE7A, 0x6A33A, 2, 3)]
    gp = lambda cs: lib.bp_grand_product(h, *[p(cc) for cc in cs], 256, *[p(s) for s in scal], fmt, p(out))
    rc["grand product, control"] = gp(cols)
    rc["grand product a"] = gp([V] + cols[1:])
    rc["grand product c"] = gp(cols[:2] + [V] + cols[3:])
    if any(v >= Q for v in v256):            # a sigma column with a foreign entry is no permutation: judged as input first, or not at all
        sig3 = ints_le(cols[5])
        sig3[0], sig3[-1] = v256[0], v256[-1]
        rc["grand product s3"] = gp(cols[:5] + [le(sig3)])
    data = V.copy()
    rc["ntt"] = lib.bp_ntt_fr(h, p(data), 8, 0, fmt, 1, 256)
    data = np.concatenate([V, V]).copy()
    rc["ntt batch"] = lib.bp_ntt_fr(h, p(data), 7, 0, fmt, 4, 128)
    return rc


def ints_le(buf):
    return [int.from_bytes(bytes(buf[i: i + 32]), "little") for i in range(0, len(buf), 32)]


@gpu
@pytest.mark.parametrize("at", [0, -1], ids=["first", "last"])
@pytest.mark.parametrize("value", [Q, 2**256 - 1], ids=["q", "2^256-1"])
def test_noncanonical_vector_elements_are_rejected(ctx, value, at):
    """BP_FR_BYTES_LE is the canonical encoding: Scalar::from_bytes rejects a value >= q (scalar.rs:264-288), a scalar ARGUMENT >= q
    is BP_ERR_BAD_SCALAR, and so is an element of a vector argument -- for every host entry point that takes one.  The largest
    canonical value in the same place is accepted, before and after (the status word does not stick)."""
    def vectors(v):
        a, b = [1 + i for i in range(300)], [1 + i for i in range(256)]
        a[at], b[at] = v, v
        return a, b
    good = canonical_calls(ctx, *vectors(Q - 1))
    assert all(rc == 0 for rc in good.values()), good
    bad = canonical_calls(ctx, *vectors(value))
    control = bad.pop("grand product, control")
    assert control == 0 and all(rc == -4 for rc in bad.values()), bad
    assert "vector element >= q" in ctx._lib.bp_last_error(ctx._h).decode()
    # two vectors of 128 at a stride of 256: what lies between them is not input (index 255), what lies in them is (index 0)
    data = np.concatenate([le(vectors(value)[1])] * 2)
    assert ctx._lib.bp_ntt_fr(ctx._h, data.ctypes.data, 7, 0, bp.FR_BYTES_LE, 2, 256) == (-4 if at == 0 else 0)
    again = canonical_calls(ctx, *vectors(Q - 1))
    assert all(rc == 0 for rc in again.values()), again

"""CPU checks of csrc/poly_rules.hpp, the host functions that decide what every Polynomial operator of the C ABI -- host form and
device form alike -- refuses and how large its result is; no GPU: the header is compiled for the host alone
(tests/cpp/poly_rules_host.hip).  Every expectation is a Python closed form of the reference's rule (polynomial.rs, utils.rs,
prover.rs), written out below; none comes from the header under test."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAGRANGE, MONOMIAL = 0, 1                                     # include/bp_msm_ntt.h
OK, INVALID_ARG, BASIS, LENGTH, DIV_ZERO, TOO_LARGE = 0, -1, -5, -6, -7, -10
POISON = 0xEEEEEEEE                                           # what an output holds before a call that may leave it alone
POISON_INT = POISON - 2**32                                   # ... read back through a signed int


@pytest.fixture(scope="module")
def pr(tmp_path_factory):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    so = str(tmp_path_factory.mktemp("poly_rules") / "libpolyrules.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O1", "-fPIC", "-shared",
                           os.path.join(ROOT, "tests", "cpp", "poly_rules_host.hip"), "-o", so])
    lib = C.CDLL(so)
    i32, sz, u64 = C.c_int, C.c_size_t, C.c_uint64
    pi, psz, pu32 = C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(C.c_uint32)
    for name, args in (("pr_addsub", [i32, sz, sz, psz, pi]), ("pr_scalar_op", [i32, i32, sz, pi, pi]), ("pr_action", [i32]),
                       ("pr_mul", [i32, sz, sz, pu32, psz, psz, pi]), ("pr_div", [sz, sz, psz, pi]), ("pr_div_basis", [i32, pi]),
                       ("pr_evaluate", [i32, pi]), ("pr_commit", [i32, pi]), ("pr_grand_product", [sz, pi]), ("pr_roots", [u64, pi])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = i32, args
    return lib


def call(fn, *args, outs=()):
    """-> (code, [outputs]): every refusal carries a text and BP_OK carries none"""
    outs = [t(POISON) for t in outs]
    text = C.c_int(-1)
    rc = fn(*args, *[C.byref(o) for o in outs], C.byref(text))
    assert text.value == (0 if rc == OK else 1), (args, rc, text.value)
    return rc, [o.value for o in outs]


@pytest.mark.parametrize("basis", [LAGRANGE, MONOMIAL])
@pytest.mark.parametrize("na,nb", [(3, 3), (3, 2), (2, 3), (0, 0), (0, 3), (3, 0), (1, 1), (2**40, 1)])
def test_addsub(pr, basis, na, nb):
    """polynomial.rs:85-89, 142-146: Lagrange operands must have one length; Monomial ones are padded to the longer"""
    rc, (n,) = call(pr.pr_addsub, basis, na, nb, outs=[C.c_size_t])
    if basis == LAGRANGE and na != nb:
        assert rc == LENGTH
    else:
        assert (rc, n) == (OK, max(na, nb))


@pytest.mark.parametrize("basis", [LAGRANGE, MONOMIAL])
@pytest.mark.parametrize("op", [-1, 0, 1, 2, 3])
@pytest.mark.parametrize("n", [0, 1, 3])
def test_scalar_op(pr, basis, op, n):
    """Mul<Scalar> multiplies every value; Lagrange Add AND Sub add s to every value (polynomial.rs:126-128); Monomial Add / Sub touch
    values[0] alone (:62, :123), which panics on an empty polynomial"""
    nothing, mul_all, add_all, first = [pr.pr_action(i) for i in range(4)]
    assert len({nothing, mul_all, add_all, first}) == 4
    rc, (action,) = call(pr.pr_scalar_op, basis, op, n, outs=[C.c_int])
    if op not in (0, 1, 2):
        want = (INVALID_ARG, None)
    elif op == 2:
        want = (OK, mul_all if n else nothing)
    elif basis == LAGRANGE:
        want = (OK, add_all if n else nothing)
    else:
        want = (OK, first) if n else (INVALID_ARG, None)
    assert rc == want[0] and action == (POISON_INT if want[1] is None else want[1]), (rc, action, want)


def mul_sizes():
    """(na, nb) with na + nb - 1 on, and one past, every threshold: 1, 2, 3, 2^k and 2^k + 1, and the cap 2^28"""
    targets = [1, 2, 3] + [t for k in (2, 3, 10, 27) for t in (2**k, 2**k + 1)] + [2**28 - 1, 2**28, 2**28 + 1, 2**29, 2**40]
    for t in targets:
        for na in sorted({1, (t + 1) // 2, t}):
            yield na, t + 1 - na
    yield from [(2**28, 1), (1, 2**28), (2**28 + 1, 1), (1, 2**28 + 1), (2**28, 2), (2**63, 2**63), (2**64 - 1, 2), (2**64 - 1, 2**64 - 1)]


@pytest.mark.parametrize("na,nb", sorted(set(mul_sizes())))
def test_mul_sizes(pr, na, nb):
    """polynomial.rs:248-272 and find_next_power_of_two (utils.rs:54-61): the product has na + nb - 1 coefficients and is computed
    at the smallest power of two of points that holds them; transforms end at 2^28.  Sizes only: nothing is allocated."""
    rc, (k, N, target) = call(pr.pr_mul, MONOMIAL, na, nb, outs=[C.c_uint32, C.c_size_t, C.c_size_t])
    t = na + nb - 1                                           # a Python integer: no wrap-around
    if t > 2**28:
        assert rc == TOO_LARGE
    else:
        want_k = (t - 1).bit_length()                         # smallest k with 2^k >= t
        assert 2**want_k >= t and (want_k == 0 or 2**(want_k - 1) < t)
        assert (rc, k, N, target) == (OK, want_k, 2**want_k, t)


@pytest.mark.parametrize("basis,na,nb,want", [(MONOMIAL, 0, 3, INVALID_ARG), (MONOMIAL, 3, 0, INVALID_ARG), (MONOMIAL, 0, 0, INVALID_ARG),
                                              (LAGRANGE, 3, 2, BASIS), (LAGRANGE, 0, 0, BASIS), (LAGRANGE, 2**28, 2**28, BASIS),
                                              (MONOMIAL, 1, 1, OK)])
def test_mul_refusals_in_order(pr, basis, na, nb, want):
    """the basis is looked at first (todo!() for Lagrange, polynomial.rs:176-246), then len - 1 underflows (:248-249)"""
    rc, (k, N, target) = call(pr.pr_mul, basis, na, nb, outs=[C.c_uint32, C.c_size_t, C.c_size_t])
    assert rc == want
    if want == OK:
        assert (k, N, target) == (0, 1, 1)


@pytest.mark.parametrize("basis", [LAGRANGE, MONOMIAL])
@pytest.mark.parametrize("na,nb", [(0, 0), (0, 1), (1, 1), (1, 2), (5, 2), (2, 2), (2, 3), (5, 0), (2**30, 1)])
def test_div(pr, basis, na, nb):
    """Div asks the basis first (polynomial.rs:319) and goes no further without Monomial; then, on the trimmed lengths: :347-348 (the
    zero divisor, whatever the dividend), :341-345 (a shorter dividend: the empty quotient), else one coefficient per degree of
    difference, plus one"""
    rc_basis, _ = call(pr.pr_div_basis, basis)
    if basis != MONOMIAL:
        assert rc_basis == BASIS
        return
    assert rc_basis == OK
    rc, (nq,) = call(pr.pr_div, na, nb, outs=[C.c_size_t])
    if nb == 0:
        assert rc == DIV_ZERO
    else:
        assert (rc, nq) == (OK, na - nb + 1 if na >= nb else 0)


def test_monomial_only(pr):
    """coeffs_evaluate (polynomial.rs:35) and Setup::commit (setup.rs:34) assert the Monomial basis"""
    for fn in (pr.pr_evaluate, pr.pr_commit):
        assert call(fn, MONOMIAL)[0] == OK and call(fn, LAGRANGE)[0] == BASIS


@pytest.mark.parametrize("n", [0, 1, 2**25 - 1, 2**25, 2**25 + 1, 2**40])
def test_grand_product(pr, n):
    assert call(pr.pr_grand_product, n)[0] == (TOO_LARGE if n > 2**25 else OK)


@pytest.mark.parametrize("order", [0, 1, 2, 3, 2**28 - 1, 2**28, 2**28 + 1, 2**32, 2**64 - 1])
def test_roots(pr, order):
    """root_of_unity divides 2^32 by group_order (utils.rs:39-43): zero panics; the vector ends where the transforms end, at 2^28"""
    assert call(pr.pr_roots, order)[0] == (INVALID_ARG if order == 0 else TOO_LARGE if order > 2**28 else OK)

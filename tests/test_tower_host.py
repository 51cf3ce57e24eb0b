"""CPU checks of csrc/tower.hpp and csrc/g2_host.hpp (no GPU): the headers compiled for the host alone (tests/cpp/tower_host.hip)
against tests/tower_model.py -- schoolbook polynomial arithmetic in Python integers -- on the reference's own literals
(tests/golden/pairing_kats.json), on edge operands (0, 1, p - 1 in the coefficients) and on seeded random ones.  Every comparison is
exact.  The same lines run in the kernels of pairing_kernels.hpp; tests/test_gpu_pairing.py compares those with the host byte for byte."""
import ctypes as C
import itertools
import random

import pytest

from tests import pairing_cases as PC
from tests import tower_model as T

P, Q = PC.P, PC.Q
EDGE = (0, 1, P - 1)


@pytest.fixture(scope="module")
def tw(tmp_path_factory):
    so = PC.build_shim(tmp_path_factory.mktemp("tower_host"))
    if so is None:
        pytest.skip("hipcc not available")
    lib = C.CDLL(so)
    cp, i32 = C.c_char_p, C.c_int
    for name, res, args in (("tw_fp2", i32, [cp, cp, cp, cp]), ("tw_fp6", i32, [cp, cp, cp, cp, cp, cp]), ("tw_fp12", i32, [cp, cp, cp, cp, i32, cp]),
                            ("tw_ell", None, [cp, cp, cp, cp]), ("tw_g2_decode", i32, [cp, cp, C.POINTER(i32)]), ("tw_g2_on_curve", i32, [cp]),
                            ("tw_g2_is_torsion_free", i32, [cp]), ("tw_g2_op", i32, [i32, cp, cp, cp, cp]), ("tw_g2_prepare", i32, [cp, cp])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def rnd_f2(r):
    return (r.randrange(P), r.randrange(P))


def rnd_f6(r):
    return tuple(rnd_f2(r) for _ in range(3))


def rnd_f12(r):
    return (rnd_f6(r), rnd_f6(r))


def f2_operands():
    r = random.Random(2)
    lit = PC.kat("fp2.rs", "test_multiplication")
    return [tuple(c) for c in itertools.product(EDGE, repeat=2)] + [(lit[0], lit[1]), (lit[2], lit[3])] + [rnd_f2(r) for _ in range(6)]


def f6_operands():
    r = random.Random(6)
    lit = PC.kat("fp6.rs", "test_arithmetic")
    ops = [tuple((lit[6 * k + 2 * j], lit[6 * k + 2 * j + 1]) for j in range(3)) for k in range(3)]
    ops += [tuple((e, e) for _ in range(3)) for e in EDGE]
    ops += [tuple((EDGE[(i + j) % 3], EDGE[(i + 2 * j + 1) % 3]) for j in range(3)) for i in range(3)]           # mixed edges
    ops += [((0, 0), (0, 0), (1, 0)), ((0, 0), (P - 1, 1), (0, 0))]
    return ops + [rnd_f6(r) for _ in range(5)]


def f12_operands():
    r = random.Random(12)
    lit = PC.kat("fp12.rs", "test_arithmetic")
    ops = [T.f12_unflat(lit[12 * k: 12 * k + 12]) for k in range(3)]
    ops += [T.f12_unflat([e] * 12) for e in EDGE]
    ops += [T.f12_unflat([EDGE[(i + k * k) % 3] for k in range(12)]) for i in range(3)]
    ops += [T.F12_ONE, T.f12_unflat([0] * 9 + [1, 0, 0])]
    return ops + [rnd_f12(r) for _ in range(4)]


def c2(tw, op, a, b=T.F2_ZERO):
    out = C.create_string_buffer(96)
    assert tw.tw_fp2(op.encode(), PC.f2_bytes(a), PC.f2_bytes(b), out) == 0
    return PC.f2_from(out.raw)


def c6(tw, op, a, b=T.F6_ZERO, s0=T.F2_ZERO, s1=T.F2_ZERO):
    out = C.create_string_buffer(288)
    assert tw.tw_fp6(op.encode(), PC.f6_bytes(a), PC.f6_bytes(b), PC.f2_bytes(s0), PC.f2_bytes(s1), out) == 0
    return PC.f6_from(out.raw)


def c12(tw, op, a, b=T.F12_ZERO, line=(T.F2_ZERO,) * 3, in_place=0):
    out = C.create_string_buffer(576)
    rc = tw.tw_fp12(op.encode(), PC.f12_bytes(a), PC.f12_bytes(b), b"".join(PC.f2_bytes(c) for c in line), in_place, out)
    assert rc >= 0
    return PC.f12_from(out.raw), rc


# ---- Fp2
def test_fp2_on_the_references_literals(tw):
    a = PC.kat("fp2.rs", "test_squaring")
    assert c2(tw, "square", (a[0], a[1])) == (a[2], a[3])
    for name, op in (("test_multiplication", "mul"), ("test_addition", "add"), ("test_subtraction", "sub")):
        v = PC.kat("fp2.rs", name)
        assert c2(tw, op, (v[0], v[1]), (v[2], v[3])) == (v[4], v[5]), name
    v = PC.kat("fp2.rs", "test_negation")
    assert c2(tw, "neg", (v[0], v[1])) == (v[2], v[3])
    v = PC.kat("fp2.rs", "test_inversion")
    assert c2(tw, "invert", (v[0], v[1])) == (v[2], v[3])
    assert T.f2_inv((v[0], v[1])) == (v[2], v[3])                  # the model agrees with the reference too


def test_fp2_against_the_model(tw):
    ops = f2_operands()
    for a in ops:
        assert c2(tw, "square", a) == T.f2_mul(a, a)
        assert c2(tw, "neg", a) == T.f2_neg(a)
        assert c2(tw, "mul_by_nonresidue", a) == T.f2_mul(a, T.XI)
        assert c2(tw, "conjugate", a) == T.f2_conj(a)
        assert c2(tw, "invert", a) == (T.f2_inv(a) if a != T.F2_ZERO else T.F2_ZERO)
        for b in ops:
            assert c2(tw, "add", a, b) == T.f2_add(a, b)
            assert c2(tw, "sub", a, b) == T.f2_sub(a, b)
            assert c2(tw, "mul", a, b) == T.f2_mul(a, b)
    for a in ops[:4] + ops[-3:]:
        assert c2(tw, "frobenius", a) == T.f2_pow(a, P)


# ---- Fp6
def test_fp6_against_the_model(tw):
    ops, f2s = f6_operands(), f2_operands()
    for i, a in enumerate(ops):
        assert c6(tw, "square", a) == T.f6_mul(a, a)
        assert c6(tw, "mul_by_nonresidue", a) == T.f6_mul_by_v(a)
        assert c6(tw, "neg", a) == T.f6_neg(a)
        if a != T.F6_ZERO:
            assert c6(tw, "invert", a) == T.f6_inv(a) and T.f6_mul(a, T.f6_inv(a)) == T.F6_ONE
        for b in ops:
            assert c6(tw, "mul", a, b) == T.f6_mul(a, b)
            assert c6(tw, "add", a, b) == T.f6_add(a, b) and c6(tw, "sub", a, b) == T.f6_sub(a, b)
        for j in range(3):
            s0, s1 = f2s[(3 * i + j) % len(f2s)], f2s[(5 * i + 2 * j + 1) % len(f2s)]
            assert c6(tw, "mul_by_1", a, s1=s1) == T.f6_mul(a, (T.F2_ZERO, s1, T.F2_ZERO))
            assert c6(tw, "mul_by_01", a, s0=s0, s1=s1) == T.f6_mul(a, (s0, s1, T.F2_ZERO))
    assert c6(tw, "invert", T.F6_ZERO) == T.F6_ZERO
    for a in ops[:3] + ops[-2:]:
        assert c6(tw, "frobenius", a) == T.f6_pow(a, P)


# ---- Fp12
@pytest.mark.parametrize("in_place", [0, 1])
def test_fp12_against_the_model(tw, in_place):
    ops, f2s = f12_operands(), f2_operands()
    for i, a in enumerate(ops):
        assert c12(tw, "square", a, in_place=in_place)[0] == T.f12_mul(a, a)
        assert c12(tw, "conjugate", a, in_place=in_place)[0] == T.f12_conj(a)
        assert c12(tw, "is_one", a)[1] == (1 if a == T.F12_ONE else 0)
        for b in ops:
            assert c12(tw, "mul", a, b, in_place=in_place)[0] == T.f12_mul(a, b)
        line = (f2s[i % len(f2s)], f2s[(2 * i + 3) % len(f2s)], f2s[(7 * i + 1) % len(f2s)])
        assert c12(tw, "mul_by_014", a, line=line, in_place=in_place)[0] == T.f12_mul(a, T.f12_sparse_014(*line))
    assert c12(tw, "one", ops[0], in_place=in_place)[0] == T.F12_ONE


def test_fp12_inversion_and_frobenius(tw):
    ops = f12_operands()
    for a in ops:
        if a == T.F12_ZERO:
            continue
        inv = c12(tw, "invert", a)[0]
        assert inv == T.f12_inv(a) and T.f12_mul(inv, a) == T.F12_ONE
        assert c12(tw, "invert", a, in_place=1)[0] == inv
    assert c12(tw, "invert", T.F12_ZERO)[0] == T.F12_ZERO
    for a in ops[:3] + ops[-2:]:
        assert c12(tw, "frobenius", a)[0] == T.f12_pow(a, P)
        assert c12(tw, "frobenius", a, in_place=1)[0] == T.f12_pow(a, P)


def test_cyclotomic_square_and_exponentiation(tw):
    """on elements already raised to (p^6 - 1)(p^2 + 1), where the compressed squaring is defined"""
    for a in f12_operands()[:3] + f12_operands()[-3:]:
        e = T.f12_mul(T.f12_conj(a), T.f12_inv(a))                # a^(p^6 - 1)
        e = T.f12_mul(T.f12_pow(e, P * P), e)                      # ^(p^2 + 1)
        assert T.f12_mul(e, T.f12_conj(e)) == T.F12_ONE            # unitary: in the cyclotomic subgroup
        for in_place in (0, 1):
            assert c12(tw, "cyclotomic_square", e, in_place=in_place)[0] == T.f12_mul(e, e)
            assert c12(tw, "cyclotomic_exp", e, in_place=in_place)[0] == T.f12_conj(T.f12_pow(e, T.BLS_X_ABS))
        assert c12(tw, "square", e)[0] == T.f12_mul(e, e)


def test_ell_is_the_sparse_product_with_the_scaled_line(tw):
    r = random.Random(3)
    for a in f12_operands()[:4]:
        line = [rnd_f2(r) for _ in range(3)]
        px, py = r.randrange(P), r.randrange(P)
        out = C.create_string_buffer(576)
        tw.tw_ell(PC.f12_bytes(a), b"".join(PC.f2_bytes(c) for c in line), PC.fp_bytes(px) + PC.fp_bytes(py), out)
        c1 = (line[1][0] * px % P, line[1][1] * px % P)
        c0 = (line[0][0] * py % P, line[0][1] * py % P)
        assert PC.f12_from(out.raw) == T.f12_mul(a, T.f12_sparse_014(line[2], c1, c0))


# ---- G2 on the host
def g2_op(tw, op, a, b=None, z=T.F2_ONE):
    out = C.create_string_buffer(192)
    assert tw.tw_g2_op(op, T.g2_enc192(a), T.g2_enc192(b), PC.f2_bytes(z), out) == 0
    return T.g2_dec192(out.raw)


def test_g2_group_law_against_the_model_and_the_references_literals(tw):
    G = PC.G2
    assert T.g2_on_curve(G) and T.g2_mul(G, Q) is None
    v = PC.kat("g2.rs", "test_doubling")
    twoG = ((v[0], v[1]), (v[2], v[3]))
    assert T.g2_double(G) == twoG and g2_op(tw, 1, G) == twoG
    lit = PC.kat("g2.rs", "test_projective_addition")
    zs = [T.F2_ONE, (lit[0], lit[1]), (P - 1, 1)]
    pts = [None, G, twoG, T.g2_neg(G), T.g2_mul(G, 3), T.g2_mul(G, Q - 1), T.g2_mul(G, 0x1234567)]
    for z in zs:
        for a in pts:
            assert g2_op(tw, 1, a, None, z) == T.g2_double(a)
            for b in pts:
                assert g2_op(tw, 0, a, b, z) == T.g2_add(a, b), (pts.index(a), pts.index(b))


def test_g2_codec_curve_and_subgroup(tw):
    G = PC.G2
    out, inf = C.create_string_buffer(192), C.c_int(-1)
    assert tw.tw_g2_decode(T.g2_enc192(G), out, C.byref(inf)) == 1 and inf.value == 0
    assert (PC.f2_from(out.raw[:96]), PC.f2_from(out.raw[96:])) == G
    assert tw.tw_g2_decode(PC.ID192, out, C.byref(inf)) == 1 and inf.value == 1
    enc = T.g2_enc192(G)
    for bad in (bytes([enc[0] | 0x80]) + enc[1:], bytes([enc[0] | 0x20]) + enc[1:], bytes([enc[0] | 0x40]) + enc[1:],     # flags
                P.to_bytes(48, "big") + enc[48:], enc[:48] + P.to_bytes(48, "big") + enc[96:], enc[:144] + (P + 1).to_bytes(48, "big"),
                bytes([0x40]) + bytes(190) + b"\x01"):
        assert tw.tw_g2_decode(bad, out, C.byref(inf)) == 0
    outside, off = T.g2_find_points()
    assert T.g2_on_curve(outside) and not T.g2_on_curve(off)
    assert tw.tw_g2_on_curve(T.g2_enc192(G)) == 1 and tw.tw_g2_on_curve(T.g2_enc192(outside)) == 1 and tw.tw_g2_on_curve(T.g2_enc192(off)) == 0
    assert tw.tw_g2_on_curve(PC.ID192) == 1
    assert tw.tw_g2_is_torsion_free(T.g2_enc192(G)) == 1 and tw.tw_g2_is_torsion_free(T.g2_enc192(outside)) == 0
    assert tw.tw_g2_is_torsion_free(PC.ID192) == 1


def test_prepared_lines_vanish_on_the_points_they_pass_through(tw):
    """line k of the table of Q is the tangent at T or the chord through T and Q, as l2 + l1 x v + l0 y v w up to a factor of Fp2:
    evaluated at (x, y) in Fp2 -- the untwisted coordinates are a scaling away -- it is zero at T (and at Q for a chord)"""
    Qp = T.g2_mul(PC.G2, 5)
    out = C.create_string_buffer(68 * 3 * 96)
    assert tw.tw_g2_prepare(T.g2_enc192(Qp), out) == 0 and tw.tw_g2_prepare(PC.ID192, out) == -1
    assert tw.tw_g2_prepare(T.g2_enc192(Qp), out) == 0
    lines = [tuple(PC.f2_from(out.raw[96 * (3 * k + j): 96 * (3 * k + j) + 96]) for j in range(3)) for k in range(68)]
    cur, k = Qp, 0
    half_x = T.BLS_X_ABS >> 1

    def at(line, pt):                                               # l2 + l1 x + l0 y
        return T.f2_add(T.f2_add(line[2], T.f2_mul(line[1], pt[0])), T.f2_mul(line[0], pt[1]))
    for b in range(61, -2, -1):
        assert at(lines[k], cur) == T.F2_ZERO and lines[k][0] != T.F2_ZERO
        cur, k = T.g2_double(cur), k + 1
        if b >= 0 and (half_x >> b) & 1:
            assert at(lines[k], cur) == T.F2_ZERO and at(lines[k], Qp) == T.F2_ZERO
            cur, k = T.g2_add(cur, Qp), k + 1
    assert k == 68 and cur == T.g2_mul(Qp, T.BLS_X_ABS)


def test_the_hard_exponent_written_in_pairing_hpp_is_three_times_the_cyclotomic_cofactor():
    """the comment above pairing_final_exponentiation, in integers: l0 + l1 p + l2 p^2 + l3 p^3 = 3 (p^4 - p^2 + 1) / q"""
    x = -T.BLS_X_ABS
    l3 = (x - 1) ** 2
    l2 = x * l3
    l1 = x * l2 - l3
    l0 = x * l1 + 3
    assert (P ** 4 - P ** 2 + 1) % Q == 0
    assert l0 + l1 * P + l2 * P ** 2 + l3 * P ** 3 == 3 * (P ** 4 - P ** 2 + 1) // Q

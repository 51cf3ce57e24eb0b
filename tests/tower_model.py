"""The BLS12-381 extension tower and G2 in Python integers: the ground truth of the pairing tests, independent of the C++ headers.

Fp2 = Fp[u] / (u^2 + 1), Fp6 = Fp2[v] / (v^3 - (u + 1)), Fp12 = Fp6[w] / (w^2 - v).  Elements are nested tuples of ints in [0, p):
Fp2 (a, b) = a + b u; Fp6 (c0, c1, c2) of Fp2; Fp12 (c0, c1) of Fp6.  Every product is the schoolbook polynomial product followed by
the reduction by the defining polynomial -- no Karatsuba, no sparse forms -- and the Frobenius map is x ** p by square-and-multiply.
G2 is the curve y^2 = x^3 + 4 (u + 1) over Fp2 in affine coordinates, None for the identity."""
from tests.bigint_model import P, Q

BLS_X_ABS = 0xD201000000010000


# ---- Fp2
F2_ZERO, F2_ONE = (0, 0), (1, 0)
XI = (1, 1)                                                      # u + 1, the non-residue that defines Fp6


def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2_neg(a):
    return (-a[0] % P, -a[1] % P)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_conj(a):
    return (a[0], -a[1] % P)


def f2_inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], P - 2, P)
    return (a[0] * n % P, -a[1] * n % P)


# ---- Fp6: polynomials of degree < 3 in v over Fp2
F6_ZERO, F6_ONE = (F2_ZERO,) * 3, (F2_ONE, F2_ZERO, F2_ZERO)


def f6_add(a, b):
    return tuple(f2_add(x, y) for x, y in zip(a, b))


def f6_sub(a, b):
    return tuple(f2_sub(x, y) for x, y in zip(a, b))


def f6_neg(a):
    return tuple(f2_neg(x) for x in a)


def f6_mul(a, b):
    t = [F2_ZERO] * 5
    for i in range(3):
        for j in range(3):
            t[i + j] = f2_add(t[i + j], f2_mul(a[i], b[j]))
    return (f2_add(t[0], f2_mul(XI, t[3])), f2_add(t[1], f2_mul(XI, t[4])), t[2])      # v^3 = xi


def f6_mul_by_v(a):
    return (f2_mul(XI, a[2]), a[0], a[1])


def f6_inv(a):
    """by the adjugate of the multiplication matrix: a^-1 = (A, B, C) / (a0 A + xi (a2 B + a1 C))"""
    a0, a1, a2 = a
    A = f2_sub(f2_mul(a0, a0), f2_mul(XI, f2_mul(a1, a2)))
    B = f2_sub(f2_mul(XI, f2_mul(a2, a2)), f2_mul(a0, a1))
    C = f2_sub(f2_mul(a1, a1), f2_mul(a0, a2))
    d = f2_inv(f2_add(f2_mul(a0, A), f2_mul(XI, f2_add(f2_mul(a2, B), f2_mul(a1, C)))))
    return (f2_mul(A, d), f2_mul(B, d), f2_mul(C, d))


# ---- Fp12: a + b w, w^2 = v
F12_ZERO, F12_ONE = (F6_ZERO, F6_ZERO), (F6_ONE, F6_ZERO)


def f12_add(a, b):
    return (f6_add(a[0], b[0]), f6_add(a[1], b[1]))


def f12_sub(a, b):
    return (f6_sub(a[0], b[0]), f6_sub(a[1], b[1]))


def f12_mul(a, b):
    return (f6_add(f6_mul(a[0], b[0]), f6_mul_by_v(f6_mul(a[1], b[1]))), f6_add(f6_mul(a[0], b[1]), f6_mul(a[1], b[0])))


def f12_conj(a):
    return (a[0], f6_neg(a[1]))


def f12_inv(a):
    d = f6_inv(f6_sub(f6_mul(a[0], a[0]), f6_mul_by_v(f6_mul(a[1], a[1]))))
    return (f6_mul(a[0], d), f6_neg(f6_mul(a[1], d)))


def _pow(one, mul, a, e):
    r = one
    for bit in bin(e)[2:]:
        r = mul(r, r)
        if bit == "1":
            r = mul(r, a)
    return r


def f2_pow(a, e):
    return _pow(F2_ONE, f2_mul, a, e)


def f6_pow(a, e):
    return _pow(F6_ONE, f6_mul, a, e)


def f12_pow(a, e):
    return _pow(F12_ONE, f12_mul, a, e)


def f12_sparse_014(c0, c1, c4):
    """the Fp12 element c0 + c1 v + c4 v w that mul_by_014 multiplies by"""
    return ((c0, c1, F2_ZERO), (F2_ZERO, c4, F2_ZERO))


def f12_flat(a):
    """the twelve Fp coefficients in memory order: c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1"""
    return [c for h in a for f2 in h for c in f2]


def f12_unflat(c):
    return tuple(tuple((c[6 * h + 2 * k], c[6 * h + 2 * k + 1]) for k in range(3)) for h in range(2))


# ---- G2, affine
G2_B = (4, 4)                                                    # 4 (u + 1)


def g2_on_curve(pt):
    if pt is None:
        return True
    x, y = pt
    return f2_mul(y, y) == f2_add(f2_mul(f2_mul(x, x), x), G2_B)


def g2_neg(pt):
    return None if pt is None else (pt[0], f2_neg(pt[1]))


def g2_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if a[1] != b[1] or a[1] == F2_ZERO:
            return None
        x2 = f2_mul(a[0], a[0])
        lam = f2_mul(f2_add(f2_add(x2, x2), x2), f2_inv(f2_add(a[1], a[1])))
    else:
        lam = f2_mul(f2_sub(b[1], a[1]), f2_inv(f2_sub(b[0], a[0])))
    x = f2_sub(f2_sub(f2_mul(lam, lam), a[0]), b[0])
    return (x, f2_sub(f2_mul(lam, f2_sub(a[0], x)), a[1]))


def g2_double(a):
    return g2_add(a, a)


def g2_mul(pt, k):
    r = None
    for bit in bin(k)[2:] if k else "":
        r = g2_add(r, r)
        if bit == "1":
            r = g2_add(r, pt)
    return r


def g2_enc192(pt):
    """G2Affine::to_uncompressed: x.c1 | x.c0 | y.c1 | y.c0, big-endian; the identity is 0x40 and zeros"""
    if pt is None:
        return bytes([0x40]) + bytes(191)
    (x0, x1), (y0, y1) = pt
    return b"".join(v.to_bytes(48, "big") for v in (x1, x0, y1, y0))


def g2_dec192(b):
    if b[0] & 0x40:
        return None
    v = [int.from_bytes(b[48 * i: 48 * i + 48], "big") for i in range(4)]
    return ((v[1], v[0]), (v[3], v[2]))


def g2_find_points(seed=1):
    """(a curve point outside the prime-order subgroup, a pair (x, y) off the curve): x = seed + k u for the first k that works"""
    k = 0
    while True:
        k += 1
        x = (seed, k)
        rhs = f2_add(f2_mul(f2_mul(x, x), x), G2_B)
        y = f2_sqrt(rhs)
        if y is None:
            continue
        pt = (x, y)
        assert g2_on_curve(pt)
        if g2_mul(pt, Q) is not None:
            return pt, (x, f2_add(y, F2_ONE))


def f2_sqrt(a):
    """a square root of a in Fp2 or None (p = 3 mod 4): with n = sqrt(norm), x0^2 = (a0 + n) / 2 or (a0 - n) / 2"""
    if a == F2_ZERO:
        return F2_ZERO
    norm = (a[0] * a[0] + a[1] * a[1]) % P
    n = pow(norm, (P + 1) // 4, P)
    if n * n % P != norm:
        return None
    half = pow(2, P - 2, P)
    for cand in ((a[0] + n) * half % P, (a[0] - n) * half % P):
        x0 = pow(cand, (P + 1) // 4, P)
        if x0 * x0 % P != cand:
            continue
        if x0 == 0:
            continue
        x1 = a[1] * pow(2 * x0, P - 2, P) % P
        if f2_mul((x0, x1), (x0, x1)) == a:
            return (x0, x1)
    return None

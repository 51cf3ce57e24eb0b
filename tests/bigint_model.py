"""Independent big-integer model of the mathematics (NOT a port of the Rust, NOT the oracle):
plain Python ints, affine short-Weierstrass formulas, textbook DFT.  Used to cross-check the
C oracle and to derive closed-form answers for the GPU tests."""

Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
GX = 0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB
GY = 0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1
ROOT_OF_UNITY = pow(7, (Q - 1) >> 32, Q)


def inv(a, m):
    return pow(a, m - 2, m)


def ec_add(p1, p2):
    """affine addition on y^2 = x^3 + 4; None = identity"""
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    x1, y1 = p1
    x2, y2 = p2
    if x1 == x2:
        if (y1 + y2) % P == 0:
            return None
        lam = 3 * x1 * x1 * inv(2 * y1, P) % P
    else:
        lam = (y2 - y1) * inv(x2 - x1, P) % P
    x3 = (lam * lam - x1 - x2) % P
    return x3, (lam * (x1 - x3) - y1) % P


def ec_mul(k, pt=(GX, GY)):
    k %= Q
    acc = None
    while k:
        if k & 1:
            acc = ec_add(acc, pt)
        pt = ec_add(pt, pt)
        k >>= 1
    return acc


def enc96(pt):
    if pt is None:
        return bytes([0x40]) + bytes(95)
    return pt[0].to_bytes(48, "big") + pt[1].to_bytes(48, "big")


def enc48(pt):
    if pt is None:
        return bytes([0xC0]) + bytes(47)
    b = bytearray(pt[0].to_bytes(48, "big"))
    b[0] |= 0x80
    if pt[1] > (P - 1) // 2:
        b[0] |= 0x20
    return bytes(b)


def dec48(b):
    """G1Affine::from_compressed (g1.rs:324-388): y = sqrt(x^3 + 4) with the sign bit choosing the larger root"""
    if b[0] & 0x40:
        return None
    x = int.from_bytes(bytes([b[0] & 0x1F]) + bytes(b[1:48]), "big")
    y = pow((x * x * x + 4) % P, (P + 1) // 4, P)            # p = 3 mod 4
    assert y * y % P == (x * x * x + 4) % P
    if (y > (P - 1) // 2) != bool(b[0] & 0x20):
        y = P - y
    return (x, y)


def omega(n):
    return pow(ROOT_OF_UNITY, (1 << 32) // n, Q)


def dft(vals, inverse=False):
    n = len(vals)
    w = omega(n)
    if inverse:
        w = inv(w, Q)
    out = []
    for x in range(n):
        s = 0
        for y, v in enumerate(vals):
            s += v * pow(w, x * y, Q)
        s %= Q
        if inverse:
            s = s * inv(n, Q) % Q
        out.append(s)
    return out


def splitmix64(state):
    state = (state + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return state, z ^ (z >> 31)


def splitmix_scalar(i, seed):
    """element i of the synthetic scalar stream"""
    s = (seed + 0x9E3779B97F4A7C15 * 8 * i) & 0xFFFFFFFFFFFFFFFF
    v = 0
    for k in range(8):
        s, z = splitmix64(s)
        v |= z << (64 * k)
    return v % Q


# ---- limb-level models of the product's three Montgomery products and of its lazy add / subtract / normalise steps ---------------
# Written from the comments of bigint.hpp, fp28.hpp, g1_28.hpp and fr29.hpp and from the definition of Montgomery arithmetic; they
# return the answer AND a set of tags naming the rare branches the case went through (tests/adversarial.py counts those tags).
# `bug=` switches on one of three deliberate mistakes, used only to show that the adversarial tables can tell a wrong model apart.

M28 = (1 << 28) - 1
M29 = (1 << 29) - 1
R384, R256, R392, R261 = 1 << 384, 1 << 256, 1 << 392, 1 << 261
H_COFACTOR = 0x396C8C005555E1568C00AAAB0000AAAB


def digits(v, w, n):
    """n little-endian digits of w bits; the top digit absorbs what is left (as the headers' normalised forms do)"""
    assert v >= 0
    mask = (1 << w) - 1
    return [(v >> (w * i)) & mask for i in range(n - 1)] + [v >> (w * (n - 1))]


def undigits(l, w):
    return sum(int(x) << (w * i) for i, x in enumerate(l))


def sat_reduce_once(t, m, tags=None, bug=None):
    """Mont::reduce_once: t < 2m -> t mod m"""
    assert 0 <= t < 2 * m
    if tags is not None:
        tags.add("final_sub_taken" if t >= m else "final_sub_not_taken")
        if t == m:
            tags.add("operand_eq_modulus")
    if bug == "skip_sub_when_equal" and t == m:
        return t
    return t - m if t >= m else t


def sat_mont_mul(a, b, m, nlimbs, tags=None, bug=None):
    """a b R^-1 mod m with R = 2^(32 nlimbs): the product-scanning loop's t = (a b + mu m) / R < 2m, then one conditional subtraction"""
    R = 1 << (32 * nlimbs)
    mu = (-a * b * pow(m, -1, R)) % R
    t = (a * b + mu * m) >> (32 * nlimbs)
    assert t >> (32 * nlimbs) == 0            # no carry leaves the top word: t < 2m < 2^(32N)
    return sat_reduce_once(t, m, tags, bug)


P28D = digits(P, 28, 14)
Q29D = digits(Q, 29, 9)
INV28 = (-pow(P, -1, 1 << 28)) % (1 << 28)
INV29 = (-pow(Q, -1, 1 << 29)) % (1 << 29)


def kp_digit(K, i):
    return digits(K * P, 28, 14)[i]


def kp_spread(K, S):
    """K p with every limb >= 2^S - 2^(S-28), value unchanged (fp28.hpp kp_spread)"""
    d, up, down = digits(K * P, 28, 14), 1 << S, 1 << (S - 28)
    r = [d[0] + up] + [d[i] + up - down for i in range(1, 13)] + [d[13] - down]
    assert undigits(r, 28) == K * P and min(r) >= 0
    return r


def mont_cols(terms, mod_d, inv, w, tags=None, bug=None, tag="mul28"):
    """sum of products a b (+ c d ...) / 2^(w n) mod m on n limbs of w bits, column by column as mul28 / mul28_2 / fr29_mul run it.
    terms: list of (a_limbs, b_limbs).  Returns the n output limbs (w bits each, the top one what is left)."""
    n, mask = len(mod_d), (1 << w) - 1
    m, out, acc, peak = [0] * n, [0] * n, 0, 0
    for k in range(2 * n - 1):
        lo, hi = max(0, k - n + 1), min(k, n - 1)
        for a, b in terms:
            acc += sum(a[i] * b[k - i] for i in range(lo, hi + 1))
        acc += sum(m[i] * mod_d[k - i] for i in range(lo, min(hi, k - 1) + 1))
        if k < n:
            m[k] = (acc * inv) & mask
            if bug == "mask_m7" and k == 7:
                m[k] &= (1 << 27) - 1
            if tags is not None:
                if m[k] == 0:
                    tags.add("%s_m%d_zero" % (tag, k))
                if m[k] == mask:
                    tags.add("%s_m%d_max" % (tag, k))
            acc += m[k] * mod_d[0]
            peak = max(peak, acc)
            assert acc < 1 << 64, "column overflow"
            if bug is None:
                assert acc & mask == 0
            acc >>= w
        else:
            peak = max(peak, acc)
            assert acc < 1 << 64, "column overflow"
            out[k - n] = acc & mask
            acc >>= w
    out[n - 1] = acc
    assert acc < 1 << 32
    if tags is not None:
        tags.add(("%s_peak" % tag, peak))
    return out


def mont_value(v, m, bits):
    """(v + mu m) / 2^bits for the mu that makes it exact: the value-level twin of mont_cols (v = a b + c d ...)"""
    R = 1 << bits
    mu = (-v * pow(m, -1, R)) % R
    return (v + mu * m) >> bits


# lazy 14 x 28 limbs: plain lists; every helper checks the u32 range the header's static_asserts promise
def f28_add(a, b):
    r = [x + y for x, y in zip(a, b)]
    assert max(r) < 1 << 32
    return r


def f28_mulk(a, k):
    r = [x * k for x in a]
    assert max(r) < 1 << 32
    return r


def f28_norm(a, tags=None, bug=None):
    """norm28: one-hop carry"""
    r = [a[0] & M28] + [(a[i] & M28) + (a[i - 1] >> 28) for i in range(1, 13)] + [a[13] + (a[12] >> 28)]
    if bug == "drop_carry_12":
        r[13] = a[13]
    if tags is not None:
        for i in range(13):
            if a[i] >> 28:
                tags.add("norm28_carry_limb%d" % i)
    assert max(r) < 1 << 32
    return r


def f28_sub(K, S, a, b):
    """sub28<K, S>: a - b + K p limb by limb, no borrows"""
    c = kp_spread(K, S)
    assert all(c[i] >= b[i] for i in range(14)), "spread form does not dominate the subtrahend"
    r = [a[i] + (c[i] - b[i]) for i in range(14)]
    assert max(r) < 1 << 32
    return r


def f28_neg(K, S, b):
    return f28_sub(K, S, [0] * 14, b)


def f28_mul(a, b, tags=None, bug=None):
    if tags is None and bug is None:
        return digits(mont_value(undigits(a, 28) * undigits(b, 28), P, 392), 28, 14)
    return mont_cols([(a, b)], P28D, INV28, 28, tags, bug, "mul28")


def f28_mul2(a, b, c, d, tags=None):
    if tags is None:
        return digits(mont_value(undigits(a, 28) * undigits(b, 28) + undigits(c, 28) * undigits(d, 28), P, 392), 28, 14)
    return mont_cols([(a, b), (c, d)], P28D, INV28, 28, tags, None, "mul28_2")


def sub_exact(a, k, w, tags=None, tag="sub"):
    """fr29_sub_exact / canon28: a - k with a borrow chain over signed limbs; returns (limbs, borrow_out)"""
    mask, borrow, r = (1 << w) - 1, 0, []
    for i in range(len(a)):
        t = a[i] - k[i] + borrow
        assert -(1 << 31) <= t < 1 << 31
        r.append(t & mask)
        borrow = t >> w
        if tags is not None and borrow < 0:
            tags.add("%s_borrow_limb%d" % (tag, i))
    return r, (1 if borrow < 0 else 0)


def f28_canon(a, tags=None):
    t, borrow = sub_exact(a, P28D, 28, tags, "canon28")
    return a if borrow else t


def fp_to_28(x_mont):
    """fp_to_28: x 2^384 -> x 2^392 mod p, re-sliced"""
    return digits(x_mont * 256 % P, 28, 14)


def fp_from_28(a):
    """fp_from_28: lazy x 2^392 -> canonical x 2^384"""
    v = undigits(a, 28)
    assert v < 1 << 384
    return v * pow(256, -1, P) % P


# lazy 9 x 29 limbs
def fr29_carry(a):
    r, c = [], 0
    for i in range(9):
        t = a[i] + c
        assert t < 1 << 32
        r.append(t & M29 if i < 8 else t)
        c = t >> 29
    return r


def fr29_add_lazy(u, v, tags=None):
    s = [x + y for x, y in zip(u, v)]
    sv = undigits(s, 29)
    if tags is not None:
        tags.add("fr29_sum_lt_2q" if sv < 2 * Q else ("fr29_sum_eq_2q" if sv == 2 * Q else "fr29_sum_gt_2q"))
    t, borrow = sub_exact(s, digits(2 * Q, 29, 9), 29, tags, "fr29_sub")
    return fr29_carry(s) if borrow else t


def fr29_spread(k, up, down):
    d = digits(k * Q, 29, 9)
    r = [d[0] + up] + [d[i] + up - down for i in range(1, 8)] + [d[8] - down]
    assert undigits(r, 29) == k * Q
    return r


def fr29_sub_lazy(u, v):
    c = fr29_spread(4, 1 << 29, 1)
    assert all(c[i] >= v[i] for i in range(9))
    return [u[i] + (c[i] - v[i]) for i in range(9)]


def fr29_mul(a, w, tags=None):
    assert max(a) < 0xC0000000 and max(w) <= M29 and undigits(a, 29) < R261
    if tags is None:
        return digits(mont_value(undigits(a, 29) * undigits(w, 29), Q, 261), 29, 9)
    return mont_cols([(a, w)], Q29D, INV29, 29, tags, None, "fr29_mul")


def fr29_butterfly(u, v, w, tags=None):
    return fr29_add_lazy(u, v, tags), fr29_mul(fr29_sub_lazy(u, v), w)


def fr29_reduce8(x, tags=None):
    c = fr29_carry(x)
    t, borrow = sub_exact(c, digits(4 * Q, 29, 9), 29, tags, "fr29_sub")
    y = c if borrow else t
    t, borrow = sub_exact(y, digits(2 * Q, 29, 9), 29, tags, "fr29_sub")
    return y if borrow else t


def fr29_radix4(a, w, tags=None):
    a0, a1, a2, a3 = a
    s02 = [x + y for x, y in zip(a0, a2)]
    s13 = [x + y for x, y in zip(a1, a3)]
    d02 = fr29_mul(fr29_sub_lazy(a0, a2), w[0])
    d13 = fr29_mul(fr29_sub_lazy(a1, a3), w[1])
    c8 = fr29_spread(8, 1 << 30, 2)
    assert all(c8[i] >= s13[i] for i in range(9))
    x = [p + q for p, q in zip(s02, s13)]
    d = [s02[i] + (c8[i] - s13[i]) for i in range(9)]
    return [fr29_reduce8(x, tags), fr29_mul(d, w[2]), fr29_add_lazy(d02, d13, tags), fr29_mul(fr29_sub_lazy(d02, d13), w[2])]


# ---- the complete formulas of Renes-Costello-Batina on plain residues (eprint 2015/1060, algorithms 7, 8, 9 with b3 = 12) ---------
def rcb_add(a, b):
    X1, Y1, Z1 = a
    X2, Y2, Z2 = b
    t0, t1, t2 = X1 * X2 % P, Y1 * Y2 % P, Z1 * Z2 % P
    t3 = ((X1 + Y1) * (X2 + Y2) - t0 - t1) % P
    t4 = ((Y1 + Z1) * (Y2 + Z2) - t1 - t2) % P
    y3 = ((X1 + Z1) * (X2 + Z2) - t0 - t2) % P
    t0, t2 = 3 * t0 % P, 12 * t2 % P
    z3, t1, y3 = (t1 + t2) % P, (t1 - t2) % P, 12 * y3 % P
    return (t3 * t1 - t4 * y3) % P, (t1 * z3 + y3 * t0) % P, (z3 * t4 + t0 * t3) % P


def rcb_add_mixed(a, b):
    """b affine (x, y), not the identity"""
    X1, Y1, Z1 = a
    X2, Y2 = b
    t0, t1 = X1 * X2 % P, Y1 * Y2 % P
    t3 = ((X2 + Y2) * (X1 + Y1) - t0 - t1) % P
    t4 = (Y2 * Z1 + Y1) % P
    y3 = (X2 * Z1 + X1) % P
    t0, t2 = 3 * t0 % P, 12 * Z1 % P
    z3, t1, y3 = (t1 + t2) % P, (t1 - t2) % P, 12 * y3 % P
    return (t3 * t1 - t4 * y3) % P, (t1 * z3 + y3 * t0) % P, (z3 * t4 + t0 * t3) % P


def rcb_double(a):
    X, Y, Z = a
    t0 = Y * Y % P
    z3 = 8 * t0 % P
    t1 = Y * Z % P
    t2 = 12 * Z * Z % P
    x3 = t2 * z3 % P
    y3 = (t0 + t2) % P
    z3 = t1 * z3 % P
    t0 = (t0 - 3 * t2) % P
    y3 = (x3 + t0 * y3) % P
    return 2 * t0 * (X * Y % P) % P, y3, z3


def proj_to_affine(a):
    """None for the identity"""
    X, Y, Z = a
    if Z % P == 0:
        return None
    zi = pow(Z, -1, P)
    return X * zi % P, Y * zi % P


def ec_mul_any(k, pt):
    """k * pt for any non-negative k (ec_mul reduces k mod q first, which is wrong outside the subgroup)"""
    acc = None
    while k:
        if k & 1:
            acc = ec_add(acc, pt)
        pt = ec_add(pt, pt)
        k >>= 1
    return acc

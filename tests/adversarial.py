"""Adversarial case tables for the device check (tests/devcheck): for every dc_<name> entry point a list of input rows (32-bit words,
as the wrapper reads them) and the expected output rows, computed with Python integers only (tests/bigint_model.py).
Random cases are a minority; the rest is built to reach the rare branches of the arithmetic headers, and every case records which of
them it takes (Table.tags): tests/test_devcheck_host.py asserts that each predicate is hit often enough, without a GPU.
Everything is seeded: the tables are the same on every machine, so a failing (entry point, case index) can be replayed."""
import random

import numpy as np

from tests import bigint_model as M
from tests.bigint_model import P, Q, M28, M29, digits, undigits

# entry point -> (input words, output words) per case: the ABI of tests/devcheck/devcheck.hip
ENTRY = {}
for _f, _n in (("fp", 12), ("fr", 8)):
    for _op, _iw in (("mul", 2), ("sqr", 1), ("add", 2), ("sub", 2), ("neg", 1), ("from_mont", 1), ("to_mont", 1), ("pow", 2), ("invert", 1)):
        ENTRY["%s_%s" % (_f, _op)] = (_iw * _n, _n)
ENTRY.update({
    "fp28_roundtrip": (12, 12), "fp28_to": (12, 14), "fp28_from": (14, 12), "fp28_mul": (28, 14), "fp28_mul2": (56, 14),
    "fp28_chain": (56, 14), "fp28_neg_mul2": (56, 14), "fp28_mulk12": (14, 28), "fp28_canon": (14, 14), "fp28_invert": (14, 14),
    "fp_invert_via28": (12, 12),
    "g1_add": (72, 36), "g1_add_mixed": (60, 36), "g1_double": (36, 36), "g1_mul_scalar": (44, 36), "g1_mul_small": (38, 36),
    "g1_to_affine": (36, 24),
    "g1_28_add_mixed_raw": (70, 42), "g1_28_add_raw": (84, 42), "g1_28_double_raw": (42, 42), "g1_28_is_identity": (42, 1),
    "g1_28_add_mixed": (62, 50), "g1_28_add": (73, 36), "g1_28_double": (37, 36), "g1_28_mul_small": (38, 36), "g1_28_add_coop": (85, 42),
    "fr29_from_sat": (8, 9), "fr29_to_sat_canonical": (9, 8), "fr29_mul": (18, 9), "fr29_add_lazy": (18, 9), "fr29_sub_lazy": (18, 9),
    "fr29_butterfly": (28, 18), "fr29_radix4": (64, 36), "fr29_reduce8": (9, 9), "fr29_twiddle_from_mont": (8, 9),
    "fp_sqrt": (12, 13), "fp_lex_largest": (12, 1), "g1_decode48": (12, 25), "g1_encode48": (24, 12), "g1_mul_by_x": (36, 36),
    "g1_is_torsion_free": (24, 1),
    "radix_digits": (26, 41),
})

# bounds of the header's lazy types, as devcheck_bounds() reports them (filled by set_bounds before the tables are built)
BOUNDS = {}
BOUND_NAMES = ["C28", "PtY28", "M28", "F28n", "MxT3s", "MxT1s", "MxT4", "MxY3", "MxNy3", "CoopSum"]


def set_bounds(flat):
    for i, n in enumerate(BOUND_NAMES):
        BOUNDS[n] = (int(flat[2 * i]), int(flat[2 * i + 1]))
    assert BOUNDS["C28"] == (M28 + 8, 6) and BOUNDS["PtY28"] == (M28 + 8, 2) and BOUNDS["M28"] == (M28, 2) and BOUNDS["F28n"] == (M28, 1)


class Table:
    def __init__(self, name):
        self.name, self.rows, self.want, self.tags, self.loose, self.peaks = name, [], [], [], [], []

    def add(self, row, want, tags=(), loose=False):
        iw, ow = ENTRY[self.name]
        assert len(row) == iw and len(want) == ow, (self.name, len(row), len(want))
        assert all(0 <= int(x) < 1 << 32 for x in row) and all(0 <= int(x) < 1 << 32 for x in want), self.name
        self.rows.append([int(x) for x in row])
        self.want.append([int(x) for x in want])
        self.tags.append(set(t for t in tags if isinstance(t, str)))
        self.loose.append(loose)
        self.peaks += [t[1] for t in tags if isinstance(t, tuple)]

    def arrays(self):
        return np.array(self.rows, dtype=np.uint32), np.array(self.want, dtype=np.uint32)


def w32(v, n):
    assert 0 <= v < 1 << (32 * n)
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


# ---- values ------------------------------------------------------------------------------------------------------------------
def limb_pattern(rnd, w, n, m):
    """a value below m whose radix-2^w limbs are drawn per limb from {0, 1, 2^(w-1), 2^w - 1, random}"""
    pick = lambda: rnd.choice([0, 1, 1 << (w - 1), (1 << w) - 1, rnd.randrange(1 << w)])
    v = undigits([pick() for _ in range(n)], w)
    v &= (1 << m.bit_length()) - 1
    return v if v < m else v - m if v < 2 * m else v % m


def specials(m):
    return [0, 1, 2, m - 1, m - 2, (m - 1) // 2, (m + 1) // 2, (m - 1) // 2 - 1, 3, 4]


def powers(m):
    out = []
    for k in range(m.bit_length()):
        out += [(1 << k) % m, ((1 << k) - 1) % m, (m - (1 << k)) % m]
    return out


def patterned(rnd, m, count, n32):
    out = []
    for i in range(count):
        w, n = [(32, n32), (28, (32 * n32 + 27) // 28), (29, (32 * n32 + 28) // 29)][i % 3]
        out.append(limb_pattern(rnd, w, n, m))
    return out


def small_order_elements(m):
    """elements of small multiplicative order: the running power of an inversion or square-root ladder passes through 1 and m - 1"""
    out = [1, m - 1]
    g = 2
    while True:                                                    # a cube root of unity (3 divides both p - 1 and q - 1)
        c = pow(g, (m - 1) // 3, m)
        if c != 1:
            break
        g += 1
    out += [c, c * c % m, m - c, m - c * c % m]
    if m == Q:                                                     # 2^32 divides q - 1: orders 4 .. 64
        for k in range(2, 7):
            out.append(pow(7, (Q - 1) >> k, Q))
    return out


# ---- saturated Montgomery fields (bigint.hpp / fields.hpp) ----------------------------------------------------------------------
def field_tables(f, m, n32, rnd, T):
    R = 1 << (32 * n32)
    Ri = pow(R, -1, m)
    mont = lambda x: x * R % m
    base = specials(m) + patterned(rnd, m, 150, n32) + [rnd.randrange(m) for _ in range(40)]
    allv = base + powers(m)
    t_mul, t_sqr, t_add, t_sub, t_neg = (Table("%s_%s" % (f, op)) for op in ("mul", "sqr", "add", "sub", "neg"))
    t_fm, t_tm, t_pow, t_inv = (Table("%s_%s" % (f, op)) for op in ("from_mont", "to_mont", "pow", "invert"))

    def mul_case(a, b):
        tags = set()
        r = M.sat_mont_mul(a, b, m, n32, tags)
        assert r == a * b * Ri % m
        t_mul.add(w32(a, n32) + w32(b, n32), w32(r, n32), ["sat_" + t for t in tags])

    for i, a in enumerate(base):                                   # operands are raw limbs: any value below the modulus
        mul_case(a, base[(i * 7 + 3) % len(base)])
        mul_case(a, m - 1 - a if a else 0)
    # chosen products: b = t R / a makes the RESULT a chosen pattern, which reaches the final subtraction from both sides
    targets = [0, 1, 2, m - 1, m - 2, (m - 1) // 2] + [(1 << k) % m for k in range(0, m.bit_length(), 13)] + \
              [((1 << k) - 1) % m for k in range(7, m.bit_length(), 17)] + patterned(rnd, m, 12, n32)
    for a in [x for x in base if x][:70]:
        for t in targets:
            b = t * R * pow(a, -1, m) % m
            assert a * b * Ri % m == t
            mul_case(a, b)
    for a in allv:
        tags = set()
        t_sqr.add(w32(a, n32), w32(M.sat_mont_mul(a, a, m, n32, tags), n32), ["sat_" + t for t in tags])
        t_neg.add(w32(a, n32), w32((m - a) % m, n32))
        t_fm.add(w32(a, n32), w32(a * Ri % m, n32))
        t_tm.add(w32(a, n32), w32(a * R % m, n32))

    def add_case(a, b):
        tags = set()
        r = M.sat_reduce_once(a + b, m, tags)
        t_add.add(w32(a, n32) + w32(b, n32), w32(r, n32), ["sat_add_" + t for t in tags])
        t_sub.add(w32(a, n32) + w32(b, n32), w32((a - b) % m, n32), ["sat_sub_borrow" if a < b else ("sat_sub_zero" if a == b else "sat_sub_plain")])

    for i, a in enumerate(allv):
        add_case(a, allv[(i * 5 + 1) % len(allv)])
        if i % 3 == 0:
            add_case(a, (m - a) % m)                               # the sum is exactly the modulus (or 0 + 0)
            add_case(a, (m - a + 1) % m)
            add_case(a, (m - a - 1) % m)
            add_case(a, a)
    # powers: any exponent of 32 N bits; few cases (each is up to 32 N squarings and as many products)
    exps = [0, 1, 2, 3, m - 1, m - 2, (m - 1) // 2, (m + 1) // 4 if m % 4 == 3 else (m - 1) // 4, R - 1, 1 << (32 * n32 - 1)] + patterned(rnd, R, 10, n32)
    bases = [0, 1, m - 1, 2] + small_order_elements(m)[2:5] + patterned(rnd, m, 8, n32) + [rnd.randrange(m) for _ in range(3)]
    for i, a in enumerate(bases):
        for e in exps[i % 2::2] + [exps[0], exps[8]]:
            t_pow.add(w32(mont(a), n32) + w32(e, n32), w32(mont(pow(a, e, m)), n32))
    for a in [0] + small_order_elements(m) + specials(m)[1:] + patterned(rnd, m, 60, n32) + [(1 << k) % m for k in range(0, m.bit_length(), 9)] + \
            [rnd.randrange(m) for _ in range(20)]:
        # the operand is the Montgomery image a R; so is the answer
        t_inv.add(w32(mont(a), n32), w32(mont(pow(a, -1, m)) if a else 0, n32), ["inv_zero"] if a == 0 else [])
    for t in (t_mul, t_sqr, t_add, t_sub, t_neg, t_fm, t_tm, t_pow, t_inv):
        T[t.name] = t


# ---- 14 x 28 lazy limbs ------------------------------------------------------------------------------------------------------------
def in_contract(l, bound):
    lb, vb = bound
    return len(l) == 14 and all(0 <= x <= lb for x in l) and undigits(l, 28) < vb * P


def lazy28(rnd, bound, style=None):
    """14 limbs within F28<LB, VB>: every limb <= LB, value < VB p, limbs pushed towards LB wherever the bound allows"""
    lb, vb = bound
    style = style or rnd.choice(["edge", "edge", "high", "top", "random", "push"])
    if style == "top":                                             # just below VB p, normalised, then push
        l = digits(vb * P - 1 - rnd.choice([0, 1, 2, rnd.randrange(1 << 40)]), 28, 14)
        style = "push_all"
    elif style in ("push", "push_all"):
        l = digits(rnd.randrange(vb * P), 28, 14)
    if style in ("push", "push_all"):                              # move k 2^28 from limb i+1 into limb i
        for i in range(13):
            if style == "push_all" or rnd.random() < 0.5:
                k = min((lb - l[i]) >> 28, l[i + 1])
                l[i] += k << 28
                l[i + 1] -= k
        assert in_contract(l, bound)
        return l
    if style == "random":
        l = [rnd.randrange(lb + 1) for _ in range(13)]
    elif style == "high":
        l = [lb - rnd.choice([0, 0, 1, rnd.randrange(16)]) for _ in range(13)]
    elif style == "low":
        l = [rnd.choice([0, 0, 1, rnd.randrange(16)]) for _ in range(13)]
    else:
        l = [rnd.choice([0, 1, 1 << 27, M28, min(lb, 1 << 28), lb, lb - 1, rnd.randrange(lb + 1)]) for _ in range(13)]
    room = (vb * P - 1 - undigits(l, 28)) >> 364                   # the largest top limb that keeps the value below VB p
    assert room >= 0
    l.append(min(lb, rnd.choice([0, room, room, max(room - 1, 0), rnd.randrange(room + 1)])))
    assert in_contract(l, bound)
    return l


def steer28(rnd, a, bound, targets):
    """b within `bound` such that the reduction digits m[k] of mul28(a, b) take the values targets[k]; a[0] odd.  None if the top limb
    that would be needed leaves the bound."""
    assert a[0] & 1
    lb, vb = bound
    ai = pow(a[0], -1, 1 << 28)
    pi = pow(M.INV28, -1, 1 << 28)
    b, m, acc = [], [], 0
    for k in range(14):
        part = sum(a[i] * b[k - i] for i in range(1, k + 1)) + sum(m[i] * M.P28D[k - i] for i in range(k)) + acc
        if k in targets:
            want = targets[k] * pi & M28                           # acc mod 2^28 that yields m[k] = target
            bk = (want - part) * ai & M28
        else:
            bk = rnd.randrange(1 << 28)
        if k == 13:
            room = (vb * P - 1 - undigits(b, 28)) >> 364
            if k in targets:
                if bk > room:
                    return None
            else:
                bk = rnd.randrange(room + 1)
        b.append(bk)
        acc = part + a[0] * bk
        m.append(acc * M.INV28 & M28)
        acc = (acc + m[k] * M.P28D[0]) >> 28
    assert in_contract(b, bound)
    return b


def fp28_tables(rnd, T):
    C28, M28b, F28n = BOUNDS["C28"], BOUNDS["M28"], BOUNDS["F28n"]
    R = 1 << 384
    t = Table("fp28_roundtrip")
    t2 = Table("fp28_to")
    for a in specials(P) + patterned(rnd, P, 200, 12) + powers(P)[::5] + [rnd.randrange(P) for _ in range(40)]:
        t.add(w32(a, 12), w32(a, 12))
        t2.add(w32(a, 12), M.fp_to_28(a))
    T[t.name], T[t2.name] = t, t2
    t = Table("fp28_from")                                         # lazy limbs in (value < 6p < 2^384), canonical saturated limbs out
    for i in range(400):
        l = lazy28(rnd, C28)
        t.add(l, w32(M.fp_from_28(l), 12))
    for k in range(6):                                             # exact multiples of p are the zero they represent
        for l in (digits(k * P, 28, 14), digits(k * P + 1, 28, 14), digits((k + 1) * P - 1, 28, 14)):
            t.add(l, w32(M.fp_from_28(l), 12))
    T[t.name] = t

    t = Table("fp28_mul")

    def mul_case(a, b):
        tags = set()
        r = M.f28_mul(a, b, tags)
        v = undigits(r, 28)
        assert r == M.f28_mul(a, b) and v < 2 * P
        tags.add("mul28_out_ge_p" if v >= P else "mul28_out_lt_p")
        t.add(a + b, r, tags)

    for i in range(300):
        mul_case(lazy28(rnd, C28), lazy28(rnd, C28))
    for i in range(100):                                           # canonical operands, as stored SRS coordinates meet an accumulator
        mul_case(M.fp_to_28(limb_pattern(rnd, 28, 14, P)), lazy28(rnd, C28))
    for k in range(14):                                            # a reduction digit of 0 and of 2^28 - 1 at every position
        for target in (0, M28):
            done = 0
            while done < 9:
                a = lazy28(rnd, C28)
                a[0] |= 1
                b = steer28(rnd, a, C28, {k: target}) if in_contract(a, C28) else None
                if b is not None:
                    mul_case(a, b)
                    done += 1
    for i in range(12):                                            # all digits steered at once
        a = lazy28(rnd, C28, "random")
        a[0] |= 1
        b = steer28(rnd, a, C28, {k: rnd.choice([0, M28]) for k in range(13)}) if in_contract(a, C28) else None
        if b is not None:
            mul_case(a, b)
    # chosen products in the 28-bit domain: the value of the result is a chosen residue
    R392 = 1 << 392
    for i in range(120):
        av = limb_pattern(rnd, 28, 14, P) or 1
        tv = rnd.choice([0, 1, P - 1, P - 2, (1 << rnd.randrange(381)) % P, ((1 << rnd.randrange(2, 381)) - 1) % P])
        mul_case(digits(av, 28, 14), digits(tv * R392 * pow(av, -1, P) % P, 28, 14))
    T[t.name] = t

    t = Table("fp28_mul2")
    for i in range(300):
        ops = [lazy28(rnd, C28, "high" if i % 3 == 0 else None) for _ in range(4)]
        tags = set()
        r = M.f28_mul2(*ops, tags)
        assert r == M.f28_mul2(*ops)
        t.add(sum(ops, []), r, tags)
    T[t.name] = t

    t = Table("fp28_chain")                                        # norm28(sub28<8,30>(mul28(a + b, c + d), add28(t0, t1)))
    for i in range(300):
        a, b, c, d = (lazy28(rnd, C28, "high" if i % 4 == 0 else None) for _ in range(4))
        tags = set()
        t0, t1 = M.f28_mul(a, c), M.f28_mul(b, d)
        r = M.f28_norm(M.f28_sub(8, 30, M.f28_mul(M.f28_add(a, b), M.f28_add(c, d)), M.f28_add(t0, t1)), tags)
        t.add(a + b + c + d, r, tags)
    T[t.name] = t

    t = Table("fp28_neg_mul2")                                     # mul28_2(t3s, t1s, t4, neg28<128,29>(y3)) on the mixed addition's own types
    peak_bound = 0
    for i in range(400):
        st = "high" if i % 2 == 0 else None
        t3s, t1s, t4, y3 = lazy28(rnd, BOUNDS["MxT3s"], st), lazy28(rnd, BOUNDS["MxT1s"], st), lazy28(rnd, BOUNDS["MxT4"], st), lazy28(rnd, BOUNDS["MxY3"], "low" if i % 4 == 0 else st)      # a small y3 makes 128 p - y3 large
        ny3 = M.f28_neg(128, 29, y3)
        assert in_contract(ny3, (BOUNDS["MxNy3"][0], BOUNDS["MxNy3"][1] + 1))          # (0, 128 p]: the header's bound counts the closed end
        tags = set()
        r = M.f28_mul2(t3s, t1s, t4, ny3, tags)
        if max(p[1] for p in tags if isinstance(p, tuple)) * 10 >= mul28_2_static_bound() * 7:
            tags.add("mul28_2_column_ge_70pct_of_static_bound")
        t.add(t3s + t1s + t4 + y3, r, tags)
    T[t.name] = t

    t = Table("fp28_mulk12")
    for i in range(300):
        a = lazy28(rnd, C28)
        tags = set()
        mk = M.f28_mulk(a, 12)
        t.add(a, mk + M.f28_norm(mk, tags), tags)
    T[t.name] = t

    t = Table("fp28_canon")                                        # M28: limbs < 2^28, value < 2p
    vals = [0, 1, P - 1, P, P + 1, 2 * P - 1, 2 * P - 2] + [P + x for x in patterned(rnd, P, 60, 12)] + patterned(rnd, P, 60, 12)
    for k in range(14):                                            # a borrow out of limb k: limbs 0..k of the operand below those of p
        for j in range(9):
            lo = rnd.randrange(undigits(M.P28D[:k + 1], 28))
            hi = rnd.randrange(1, (2 * P) >> (28 * (k + 1))) if k < 13 else 0
            v = lo + (hi << (28 * (k + 1)))
            if v < 2 * P:
                vals.append(v)
    for v in vals:
        l = digits(v, 28, 14)
        assert in_contract(l, M28b)
        tags = set()
        t.add(l, M.f28_canon(l, tags), tags)
    T[t.name] = t

    t = Table("fp28_invert")                                       # x 2^392 (value < 2p) -> x^-1 2^392, a chain of mul28: its own representative
    tv = Table("fp_invert_via28")
    R392m = R392 % P
    for a in [0] + small_order_elements(P) + specials(P)[1:] + patterned(rnd, P, 40, 12) + [rnd.randrange(P) for _ in range(10)]:
        for lazy in (0, 1):
            v = a * R392m % P + lazy * P                           # the same residue, also as the representative in [p, 2p)
            x = digits(v, 28, 14)
            r = digits(R392m, 28, 14)                              # One28
            e = P - 2
            for bit in range(380, -1, -1):
                r = M.f28_mul(r, r)
                if (e >> bit) & 1:
                    r = M.f28_mul(r, x)
            assert undigits(r, 28) % P == (pow(a, -1, P) * R392m % P if a else 0)
            t.add(x, r)
        tv.add(w32(a * R % P, 12), w32(pow(a, -1, P) * R % P if a else 0, 12))
    T[t.name], T[tv.name] = t, tv


# ---- G1 ------------------------------------------------------------------------------------------------------------------------
R384 = 1 << 384
mont = lambda x: x * R384 % P
G = (M.GX, M.GY)
ID = (0, 1, 0)


def proj_words(p):
    return w32(mont(p[0]), 12) + w32(mont(p[1]), 12) + w32(mont(p[2]), 12)


def aff_words(a):
    return [0] * 24 if a is None else w32(mont(a[0]), 12) + w32(mont(a[1]), 12)


def lift(a, z=1):
    return ID if a is None else (a[0] * z % P, a[1] * z % P, z % P)


def sqrt_p(a):
    s = pow(a, (P + 1) // 4, P)
    return s if s * s % P == a % P else None


def curve_points(rnd):
    """(subgroup points, curve points outside the subgroup); x limb-patterned where a pattern lies on the curve"""
    sub = [M.ec_mul(k) for k in (1, 2, 3, 4, 5, 7, 8, 15, 16, 255, Q - 1, Q - 2, (Q - 1) // 2, 1 << 64)]
    out = []
    tries = 0
    while len(out) < 24:
        x = limb_pattern(rnd, [32, 28][tries % 2], [12, 14][tries % 2], P)
        tries += 1
        y = sqrt_p(x * x * x + 4)
        if y is None:
            continue
        pt = (x, rnd.choice([y, P - y]))
        out.append(pt)                                            # a random curve point lies in the subgroup with probability 1 / h
        if len(out) % 4 == 0:
            sub.append(M.ec_mul_any(M.H_COFACTOR, pt))             # cofactor clearing brings it in
    assert all(M.ec_mul_any(Q, p) is None for p in sub) and all(M.ec_mul_any(Q, p) is not None for p in out)
    return sub, out


def neg(a):
    return None if a is None else (a[0], (P - a[1]) % P)


def scalar_mul_model(p, k, nbits, acc=ID):
    for i in range(nbits - 1, -1, -1):
        acc = M.rcb_double(acc)
        if (k >> i) & 1:
            acc = M.rcb_add(acc, p)
    return acc


def g1_tables(rnd, T, sub, out):
    zs = [1, 2, P - 1, 1 << 380, (1 << 381) % P, rnd.randrange(1, P), limb_pattern(rnd, 32, 12, P) or 1]
    pts = sub + out[:6]
    ids = [ID, (0, P - 1, 0), (0, rnd.randrange(1, P), 0)]
    pairs = []
    for i, a in enumerate(pts):                                    # P + P, P + (-P), P + O, O + P, O + O, P + Q, in several projective forms
        z1, z2 = zs[i % len(zs)], zs[(i + 3) % len(zs)]
        b = pts[(i + 5) % len(pts)]
        pairs += [(lift(a, z1), lift(a, z2)), (lift(a, z1), lift(neg(a), z2)), (lift(a, z1), ids[i % 3]), (ids[i % 3], lift(a, z2)), (lift(a, z1), lift(b, z2))]
    pairs += [(x, y) for x in ids for y in ids]
    t, tm, td, ta = Table("g1_add"), Table("g1_add_mixed"), Table("g1_double"), Table("g1_to_affine")
    for a, b in pairs:
        r = M.rcb_add(a, b)
        assert M.proj_to_affine(r) == M.ec_add(M.proj_to_affine(a), M.proj_to_affine(b))
        t.add(proj_words(a) + proj_words(b), proj_words(r), ["g1_add_" + kind(a, b)])
        ba = M.proj_to_affine(b)
        rm = a if ba is None else M.rcb_add_mixed(a, ba)           # the affine identity (0, 0) leaves the accumulator as it is
        tm.add(proj_words(a) + aff_words(ba), proj_words(rm), ["g1_add_mixed_" + kind(a, b)])
        for x in (a, r):
            td.add(proj_words(x), proj_words(M.rcb_double(x)))
            ta.add(proj_words(x), aff_words(M.proj_to_affine(x)))
    T.update({x.name: x for x in (t, tm, td, ta)})

    t = Table("g1_mul_scalar")
    ks = [0, 1, 2, Q - 1, Q - 2, (Q - 1) // 2, 1 << 254, (1 << 254) - 1, (1 << 255) - 1] + patterned(rnd, Q, 12, 8) + [rnd.randrange(Q) for _ in range(6)]
    for i, k in enumerate(ks):                                     # 8 limbs, bits 0..254 used (as the header's loop reads them)
        for p in (lift(pts[i % len(pts)], zs[i % len(zs)]), lift(G), ID)[:2 if i > 8 else 3]:
            t.add(proj_words(p) + w32(k, 8), proj_words(scalar_mul_model(p, k, 255)))
    T[t.name] = t
    t = Table("g1_mul_small")
    t28 = Table("g1_28_mul_small")
    for i, (k, nb) in enumerate([(0, 1), (1, 1), (0, 8), (1, 8), (255, 8), (2, 2), (3, 2), (0xFFFF, 16), (0x8000, 16), (0xD0000, 20), (0xFFFFFFFF, 32), (0x80000001, 32),
                                 (5, 3), (12345, 14), (1, 32)] + [(rnd.randrange(1 << 20), 20) for _ in range(8)]):
        for p in (lift(pts[i % len(pts)], zs[i % len(zs)]), ID if i % 4 == 0 else lift(G)):
            t.add(proj_words(p) + [k, nb], proj_words(scalar_mul_model(p, k, nb)))
            if i % 2 == 0 or nb <= 8:
                t28.add(proj_words(p) + [k, nb], proj28_out(mul_small28_model(to28(p), k, nb)))
    T[t.name], T[t28.name] = t, t28
    return pairs


def kind(a, b):
    pa, pb = M.proj_to_affine(a), M.proj_to_affine(b)
    if pa is None and pb is None:
        return "O+O"
    if pa is None:
        return "O+P"
    if pb is None:
        return "P+O"
    if pa == pb:
        return "P+P"
    if pa == neg(pb):
        return "P-P"
    return "P+Q"


# ---- the group law on lazy limbs (g1_28.hpp), limb by limb --------------------------------------------------------------------------
ONE28 = digits((1 << 392) % P, 28, 14)
ID28 = ([0] * 14, ONE28, [0] * 14)


def to28(p):
    return tuple(M.fp_to_28(mont(c)) for c in p)


def proj28_out(p):
    return sum((w32(M.fp_from_28(c), 12) for c in p), [])


def add_mixed28_model(acc, x2, y2, tags=None):
    X1, Y1, Z1 = acc
    t0, t1 = M.f28_mul(X1, x2), M.f28_mul(Y1, y2)
    t3 = M.f28_mul(M.f28_add(x2, y2), M.f28_add(X1, Y1))
    t3s = M.f28_norm(M.f28_sub(8, 30, t3, M.f28_add(t0, t1)), tags)
    t4 = M.f28_add(M.f28_mul(y2, Z1), Y1)
    y3a = M.f28_norm(M.f28_add(M.f28_mul(x2, Z1), X1), tags)
    t0x3 = M.f28_mulk(t0, 3)
    t2 = M.f28_norm(M.f28_mulk(Z1, 12), tags)
    z3 = M.f28_add(t1, t2)
    t1s = M.f28_sub(80, 29, t1, t2)
    y3 = M.f28_norm(M.f28_mulk(y3a, 12), tags)
    for v, b in ((t3s, "MxT3s"), (t1s, "MxT1s"), (t4, "MxT4"), (y3, "MxY3")):
        assert in_contract(v, BOUNDS[b]), b
    return (M.f28_mul2(t3s, t1s, t4, M.f28_neg(128, 29, y3)), M.f28_mul2(t1s, z3, y3, t0x3), M.f28_mul2(z3, t4, t0x3, t3s))


def add28_model(a, b, tags=None):
    t0, t1, t2 = M.f28_mul(a[0], b[0]), M.f28_mul(a[1], b[1]), M.f28_mul(a[2], b[2])
    cross = lambda i, j, u, v: M.f28_norm(M.f28_sub(8, 30, M.f28_mul(M.f28_add(a[i], a[j]), M.f28_add(b[i], b[j])), M.f28_add(u, v)), tags)
    t3, t4, y3a = cross(0, 1, t0, t1), cross(1, 2, t1, t2), cross(0, 2, t0, t2)
    t0x3 = M.f28_mulk(t0, 3)
    t2b = M.f28_norm(M.f28_mulk(t2, 12), tags)
    z3 = M.f28_add(t1, t2b)
    t1s = M.f28_sub(32, 29, t1, t2b)
    y3 = M.f28_norm(M.f28_mulk(y3a, 12), tags)
    return (M.f28_mul2(t3, t1s, t4, M.f28_neg(128, 29, y3)), M.f28_mul2(t1s, z3, y3, t0x3), M.f28_mul2(z3, t4, t0x3, t3))


def double28_model(p, tags=None):
    X, Y, Z = p
    t0 = M.f28_mul(Y, Y)
    z8 = M.f28_mulk(t0, 8)
    t1 = M.f28_mul(Y, Z)
    t2 = M.f28_norm(M.f28_mulk(M.f28_mul(Z, Z), 12), tags)
    x3 = M.f28_mul(t2, z8)
    y3 = M.f28_add(t0, t2)
    zo = M.f28_mul(t1, z8)
    t0s = M.f28_sub(80, 30, t0, M.f28_mulk(t2, 3))
    yo = M.f28_add(x3, M.f28_mul(t0s, y3))
    xo = M.f28_mulk(M.f28_mul(t0s, M.f28_mul(X, Y)), 2)
    r = (M.f28_norm(xo, tags), M.f28_norm(yo, tags), M.f28_norm(zo, tags))
    assert all(in_contract(c, BOUNDS["C28"]) for c in r)
    return r


def mul_small28_model(p, k, nbits):
    acc = ID28
    for i in range(nbits - 1, -1, -1):
        acc = double28_model(acc)
        if (k >> i) & 1:
            acc = add28_model(acc, p)
    return acc


def pt_y_signed_model(y, negate):
    return M.f28_norm(M.f28_sub(2, 29, [0] * 14, y)) if negate else list(y)


def lazy_point28(rnd, p, style=None):
    """a projective point as three C28 coordinates: the canonical residues of `p` plus a multiple of p below 6p, limbs pushed up"""
    C28 = BOUNDS["C28"]
    out = []
    for c in to28(p):
        v = undigits(c, 28) + rnd.randrange(6) * P
        l = digits(v, 28, 14)
        for i in range(13):
            if rnd.random() < 0.7:
                k = min((C28[0] - l[i]) >> 28, l[i + 1])
                l[i] += k << 28
                l[i + 1] -= k
        assert in_contract(l, C28)
        out.append(l)
    return tuple(out)


def g1_28_tables(rnd, T, pairs, sub, out):
    C28 = BOUNDS["C28"]
    flat = lambda p: p[0] + p[1] + p[2]
    t_add, t_coop, t_dbl, t_mix, t_id = Table("g1_28_add_raw"), Table("g1_28_add_coop"), Table("g1_28_double_raw"), Table("g1_28_add_mixed_raw"), Table("g1_28_is_identity")
    # raw forms.  Curve points in lazy representations, and arbitrary in-contract limbs: the formulas are polynomial maps, the device
    # must compute them on ANY operand within the type's bounds, on the curve or not
    raw_pairs = [(lazy_point28(rnd, a), lazy_point28(rnd, b)) for a, b in pairs]
    raw_pairs += [(tuple(lazy28(rnd, C28, st) for _ in range(3)), tuple(lazy28(rnd, C28, st) for _ in range(3))) for st in ["high", "edge", "top", None] * 20]
    for i, (a, b) in enumerate(raw_pairs):
        tags = set()
        r = add28_model(a, b, tags)
        t_add.add(flat(a) + flat(b), flat(r), tags)
        t_coop.add(flat(a) + flat(b) + [1], flat(r))             # the cooperative split gives the same limbs
        if i % 4 == 0:                                           # chains: the sum goes back in as the first operand, as in the bucket reduction
            x = r
            for reps in range(2, 8):
                x = add28_model(x, b)
                if reps in (2, 7):
                    t_coop.add(flat(a) + flat(b) + [reps], flat(x))
        t_dbl.add(flat(a), flat(double28_model(a, tags)), tags)
        for p in (a, r):
            zero = undigits(p[2], 28) % P == 0
            t_id.add(flat(p), [1 if zero else 0], ["is_identity28_" + ("yes" if zero else "no")])
    for k in range(6):                                             # Z = k p: lazy forms of zero
        p = (lazy28(rnd, C28), lazy28(rnd, C28), digits(k * P, 28, 14))
        t_id.add(flat(p), [1], ["is_identity28_yes", "is_identity28_lazy_zero"] if k else ["is_identity28_yes"])
        p = (p[0], p[1], digits(k * P + 1, 28, 14))
        t_id.add(flat(p), [0], ["is_identity28_no"])
    # the mixed form is never fed an identity POINT (the kernels select around it): b is always a finite point here.
    # The accumulator may be anything, the identity included.
    pts = sub + out[:6]
    for i, (a, _) in enumerate(raw_pairs):
        if i < len(pairs):
            b = pts[i % len(pts)]
            if i % 3 == 0 and M.proj_to_affine(pairs[i][0]) is not None:
                b = M.proj_to_affine(pairs[i][0])                  # acc + the very same point, and its negative (below)
            x2, y = M.fp_to_28(mont(b[0])), M.fp_to_28(mont(b[1]))
            y2 = pt_y_signed_model(y, i % 2 == 1)
        else:
            x2, y2 = lazy28(rnd, BOUNDS["F28n"]), lazy28(rnd, BOUNDS["PtY28"])
        tags = set()
        t_mix.add(flat(a) + x2 + y2, flat(add_mixed28_model(a, x2, y2, tags)), tags)
    T.update({x.name: x for x in (t_add, t_coop, t_dbl, t_mix, t_id)})
    # chains from saturated operands, 1 / 2 / 7 operations
    t_madd, t_cadd, t_cdbl = Table("g1_28_add_mixed"), Table("g1_28_add"), Table("g1_28_double")
    for i, (a, b) in enumerate(pairs):
        reps = (1, 2, 7)[i % 3]
        x, y = to28(a), to28(b)
        for _ in range(reps):
            x = add28_model(x, y)
        t_cadd.add(proj_words(a) + proj_words(b) + [reps], proj28_out(x))
        x = to28(a)
        for _ in range(reps):
            x = double28_model(x)
        t_cdbl.add(proj_words(a) + [reps], proj28_out(x))
        ba = M.proj_to_affine(b)
        if ba is None:
            continue                                               # see above: never the identity point
        for negate in (0, 1):
            x = to28(a)
            ys = pt_y_signed_model(M.fp_to_28(mont(ba[1])), negate)
            for _ in range(reps):
                x = add_mixed28_model(x, M.fp_to_28(mont(ba[0])), ys)
            want_pt = M.proj_to_affine(a)
            for _ in range(reps):
                want_pt = M.ec_add(want_pt, neg(ba) if negate else ba)
            got = tuple(M.fp_from_28(c) * pow(R384, -1, P) % P for c in x)
            assert M.proj_to_affine(got) == want_pt                 # the limb model agrees with the affine group law
            t_madd.add(proj_words(a) + aff_words(ba) + [negate, reps], proj28_out(x) + ys)
    T.update({x.name: x for x in (t_madd, t_cadd, t_cdbl)})


# ---- 9 x 29 lazy limbs (fr29.hpp) ---------------------------------------------------------------------------------------------------
def fr29_tables(rnd, T):
    R = 1 << 256
    d29 = lambda v: digits(v, 29, 9)
    two_q = 2 * Q
    vals2q = [0, 1, Q - 1, Q, Q + 1, two_q - 1, two_q - 2] + [limb_pattern(rnd, 29, 9, two_q) for _ in range(80)] + [rnd.randrange(two_q) for _ in range(30)]
    t, t2, t3 = Table("fr29_from_sat"), Table("fr29_to_sat_canonical"), Table("fr29_twiddle_from_mont")
    for v in [0, 1, R - 1, R - 2, 1 << 255] + patterned(rnd, R, 120, 8) + powers(Q)[::7]:
        t.add(w32(v, 8), d29(v))                                   # any 256-bit value
    for v in vals2q:
        t2.add(d29(v), w32(v % Q, 8), ["fr29_canon_sub" if v >= Q else "fr29_canon_keep"])
    for v in specials(Q) + patterned(rnd, Q, 100, 8) + powers(Q)[::9]:
        t3.add(w32(v, 8), d29(v * 32 % Q))
    T.update({x.name: x for x in (t, t2, t3)})

    t_add, t_sub = Table("fr29_add_lazy"), Table("fr29_sub_lazy")
    pairs = []
    for s in (two_q - 1, two_q, two_q + 1, 4 * Q - 2):              # u + v on and around the 2q boundary
        for i in range(12):
            u = min(two_q - 1, max(s - (two_q - 1), limb_pattern(rnd, 29, 9, two_q)))
            pairs.append((u, s - u))
    for i in range(12):
        u = limb_pattern(rnd, 29, 9, two_q)
        pairs += [(u, u), (0, two_q - 1) if i % 2 else (u, two_q - 1 - u), (two_q - 1, 0)]       # u - v = 0, -(2q - 1), 2q - 1
    for k in range(9):                                             # a borrow out of limb k of the exact subtraction s - 2q
        for j in range(9):
            lo = rnd.randrange(undigits(digits(two_q, 29, 9)[:k + 1], 29))
            hi = rnd.randrange(1, (4 * Q) >> (29 * (k + 1))) if k < 8 else 0
            s = lo + (hi << (29 * (k + 1)))
            if s <= 4 * Q - 2:
                u = min(two_q - 1, max(s - (two_q - 1), 0, min(s, rnd.randrange(two_q))))
                pairs.append((u, s - u))
    pairs += [(vals2q[i], vals2q[(i * 3 + 1) % len(vals2q)]) for i in range(len(vals2q))]
    for u, v in pairs:
        assert 0 <= u < two_q and 0 <= v < two_q
        tags = set()
        t_add.add(d29(u) + d29(v), M.fr29_add_lazy(d29(u), d29(v), tags), tags)
        t_sub.add(d29(u) + d29(v), M.fr29_sub_lazy(d29(u), d29(v)))
    T[t_add.name], T[t_sub.name] = t_add, t_sub

    t = Table("fr29_mul")                                          # a: limbs < 1.5 * 2^31, value < 2^261; w: normalised, < q
    ws = [0, 1, Q - 1, (1 << 261) % Q] + [limb_pattern(rnd, 29, 9, Q) for _ in range(40)]
    for i in range(400):
        st = i % 4
        if st == 0:
            a = M.fr29_sub_lazy(d29(rnd.choice(vals2q)), d29(rnd.choice(vals2q)))      # what the butterflies feed it
        elif st == 1:
            a = d29(limb_pattern(rnd, 29, 9, 1 << 261))
        else:                                                      # limbs towards the bound 0xBFFFFFFF, value kept below 2^261
            a = [rnd.choice([0xBFFFFFFF, 0xBFFFFFFE, 1 << 31, M29, rnd.randrange(0xC0000000)]) for _ in range(8)]
            room = ((1 << 261) - 1 - undigits(a, 29)) >> 232
            a.append(rnd.choice([room, rnd.randrange(room + 1)]))
        w = d29(rnd.choice(ws)) if i % 3 else d29(rnd.randrange(Q))
        tags = set()
        r = M.fr29_mul(a, w, tags)
        assert r == M.fr29_mul(a, w)
        t.add(a + w, r, tags)
    T[t.name] = t

    t = Table("fr29_butterfly")
    for i, (u, v) in enumerate(pairs[:200]):
        for reps in (1, 2, 7):
            if reps > 1 and i % 3:
                continue
            w = d29(ws[i % len(ws)])
            a, b = d29(u), d29(v)
            for _ in range(reps):
                a, b = M.fr29_butterfly(a, b, w)
            t.add(d29(u) + d29(v) + w + [reps], a + b)
    T[t.name] = t

    t = Table("fr29_radix4")
    quads = [[rnd.choice([0, two_q - 1, Q, Q - 1, Q + 1, two_q - 2, 1]) for _ in range(4)] for _ in range(60)]
    quads += [[limb_pattern(rnd, 29, 9, two_q) for _ in range(4)] for _ in range(60)] + [[rnd.randrange(two_q) for _ in range(4)] for _ in range(20)]
    quads += [[c] * 4 for c in (0, 1, Q - 1, two_q - 1)]
    for i, qd in enumerate(quads):
        w = [d29(ws[(i + j) % len(ws)]) for j in range(3)]
        a = [d29(x) for x in qd]
        tags = set()
        lazy = M.fr29_radix4(a, w, tags)
        u0, u2 = M.fr29_butterfly(a[0], a[2], w[0], tags)
        u1, u3 = M.fr29_butterfly(a[1], a[3], w[1], tags)
        b0, b1 = M.fr29_butterfly(u0, u1, w[2], tags)
        b2, b3 = M.fr29_butterfly(u2, u3, w[2], tags)
        row = sum(a, []) + sum(w, [])
        t.add(row + [1], sum(lazy, []), tags)
        t.add(row + [0], b0 + b1 + b2 + b3)
        assert [undigits(x, 29) % Q for x in lazy] == [undigits(x, 29) % Q for x in (b0, b1, b2, b3)]
    T[t.name] = t

    t = Table("fr29_reduce8")                                      # limbs < 2^31, value < 8q
    for i in range(300):
        if i % 3 == 0:
            v = rnd.choice([0, two_q - 1, two_q, two_q + 1, 4 * Q - 1, 4 * Q, 4 * Q + 1, 6 * Q - 1, 6 * Q, 6 * Q + 1, 8 * Q - 1, Q, 3 * Q, 5 * Q, 7 * Q])
            x = d29(v)
        elif i % 3 == 1:
            x = d29(limb_pattern(rnd, 29, 9, 8 * Q))
        else:                                                      # sums of four normalised values, unreduced
            x = [sum(c) for c in zip(*[d29(rnd.choice(vals2q)) for _ in range(4)])]
        for j in range(8):                                         # push limbs up: move k 2^29 from limb j+1 into limb j, limbs stay below 2^31
            if rnd.random() < 0.5:
                k = min(((1 << 31) - 1 - x[j]) >> 29, x[j + 1])
                x[j] += k << 29
                x[j + 1] -= k
        assert max(x) < 1 << 31 and undigits(x, 29) < 8 * Q
        tags = set()
        t.add(x, M.fr29_reduce8(x, tags), tags)
    T[t.name] = t


# ---- g1_check.hpp -------------------------------------------------------------------------------------------------------------------
def bytes_to_words(b):
    return [int.from_bytes(b[4 * j:4 * j + 4], "little") for j in range(12)]


def decode_model(b):
    """(affine point or None, reason) as g1_decode48 answers: from_compressed_unchecked of zkcrypto/bls12_381"""
    flags = b[0] >> 5
    x = int.from_bytes(bytes([b[0] & 0x1F]) + bytes(b[1:]), "big")
    if not flags & 4 or x >= P:
        return None, 1
    if flags & 2:
        return None, (1 if (flags & 1) or x else 0)
    y = sqrt_p((x * x * x + 4) % P)
    if y is None:
        return None, 2
    if (y > (P - 1) // 2) != bool(flags & 1):
        y = (P - y) % P
    return (x, y), 0


def check_tables(rnd, T, sub, out):
    half = (P - 1) // 2
    t = Table("fp_sqrt")                                           # Montgomery in and out; the value is a^((p+1)/4) whether or not it is a root
    vals = [0, 1, 4, P - 1, 2, 3] + small_order_elements(P) + [x * x % P for x in patterned(rnd, P, 60, 12)] + patterned(rnd, P, 50, 12)
    nonres = [v for v in range(2, 40) if sqrt_p(v) is None][:8]
    for a in vals + nonres + [P - x * x % P for x in patterned(rnd, P, 10, 12) if x]:
        s = pow(a, (P + 1) // 4, P)
        ok = s * s % P == a
        t.add(w32(mont(a), 12), w32(mont(s), 12) + [1 if ok else 0], ["sqrt_residue" if ok else "sqrt_nonresidue"])
    T[t.name] = t
    t = Table("fp_lex_largest")                                    # canonical (not Montgomery) limbs
    for y in [0, 1, half - 1, half, half + 1, half + 2, P - 1, P - 2] + patterned(rnd, P, 120, 12) + powers(P)[::11]:
        tags = []
        if abs(y - half) <= 1:
            tags.append("lex_near_half_" + ("yes" if y > half else "no"))
        t.add(w32(y, 12), [1 if y > half else 0], tags)
    T[t.name] = t

    t, te = Table("g1_decode48"), Table("g1_encode48")
    recs = []
    pts = sub + out
    for i, pt in enumerate(pts):                                   # a valid x under all 8 flag combinations
        for flags in range(8) if i < 10 else (4, 5):
            b = bytearray(pt[0].to_bytes(48, "big"))
            b[0] |= flags << 5
            recs.append(bytes(b))
    xs_bad = []
    x = 5
    while len(xs_bad) < 10:                                        # x^3 + 4 a non-residue
        x = limb_pattern(rnd, 32, 12, P)
        if sqrt_p((x * x * x + 4) % P) is None:
            xs_bad.append(x)
    for x in xs_bad + [P - 1, P, P + 1, 0, 1, (1 << 381) - 1, P + (1 << 200)]:
        for flags in range(8):
            b = bytearray((x & ((1 << 381) - 1)).to_bytes(48, "big")) if x >= 1 << 381 else bytearray(x.to_bytes(48, "big"))
            b[0] |= flags << 5
            recs.append(bytes(b))
    for flags in range(8):                                         # the infinity encoding, with stray bits in every byte position class
        for stray in (0, 1, 1 << 100, 1 << 376, 1 << 380):
            b = bytearray(stray.to_bytes(48, "big"))
            b[0] |= flags << 5
            recs.append(bytes(b))
    for b in recs:
        pt, reason = decode_model(b)
        t.add(bytes_to_words(b), aff_words(pt) + [reason], ["decode_reason_%d" % reason, "decode_identity"] if reason == 0 and pt is None else ["decode_reason_%d" % reason])
    # encode: both signs of every point, the identity, and decode(encode) closes
    for pt in pts:
        for q in (pt, neg(pt)):
            b = M.enc48(q)
            assert decode_model(b) == (q, 0)
            te.add(aff_words(q), bytes_to_words(b), ["encode_sort_%d" % (1 if q[1] > half else 0)])
    te.add([0] * 24, bytes_to_words(M.enc48(None)))
    T[t.name], T[te.name] = t, te

    t, tf = Table("g1_mul_by_x"), Table("g1_is_torsion_free")
    X_ABS = 0xD201000000010000
    for i, pt in enumerate([None] + sub[:10] + out[:8]):
        for z in (1, P - 1) if i < 6 else (1 + i,):
            p = lift(pt, z)
            acc = p
            for b in range(62, -1, -1):
                acc = M.rcb_double(acc)
                if (X_ABS >> b) & 1:
                    acc = M.rcb_add(acc, p)
            assert M.proj_to_affine(acc) == (M.ec_mul_any(X_ABS, pt) if pt else None)
            t.add(proj_words(p), proj_words(acc))
    for pt in [None] + sub + [neg(p) for p in sub[:6]]:
        tf.add(aff_words(pt), [1], ["torsion_free_yes"])
    for pt in out + [neg(p) for p in out[:6]]:
        tf.add(aff_words(pt), [0], ["torsion_free_no"])
    T[t.name], T[tf.name] = t, tf


# ---- msm_digits.hpp -----------------------------------------------------------------------------------------------------------------
def windows_of(c):
    W = max(2, (255 + c - 1) // c)
    while True:
        bias = sum(1 << (c * w + c - 1) for w in range(W - 1))
        if c * (W - 1) < 288 and ((Q - 1 + bias) >> (c * (W - 1))) <= 1 << (c - 1):
            return W
        W += 1


def radix_of(c, W):
    """the radix msm_radix_compute picks (0: power-of-two windows), with m = ceil(2^512 / R^W) and the bias"""
    lo, hi = 4, 1 << 31
    while lo < hi:                                                 # smallest even R with R^W > 2^256
        mid = (lo + hi) // 2 & ~1
        if mid ** W > 1 << 256:
            hi = mid
        else:
            lo = mid + 2
    R = lo
    if R > 0.9 * (1 << c):
        return 0, 0, 0
    best, best_bits = 0, 99
    cand = R
    while cand <= R + R // 50:
        if not cand ** W < (1 << 256) + (0xE6666666 << 224):
            break
        bits = bin(cand).count("1")
        if bits < best_bits:
            best, best_bits = cand, bits
        cand += 2
    if not best:
        return 0, 0, 0
    return best, -(-(1 << 512) // best ** W), sum((best // 2) * best ** w for w in range(W - 1))


def radix_tables(rnd, T):
    t = Table("radix_digits")
    for c in [13, 14, 18, 19, 20, 21, 22, 23, 24]:
        W = windows_of(c)
        R, m, bias = radix_of(c, W)
        if R == 0:
            continue
        if c == 20:
            assert (W, R) == (13, 0xD0000)
        r2 = random.Random(c)
        ks = [0, 1, 2, R // 2 - 1, R // 2, R // 2 + 1, R - 1, R, R + 1, Q - 1, Q - 2, Q // 2, Q // 3, 2 ** 254, 2 ** 254 - 1, 2 ** 200 + 1]
        for j in range(1, W):
            for tt in (1, R // 2, R // 2 + 1, R - 1, r2.randrange(1, R)):
                for e in (-2, -1, 0, 1, 2):
                    ks.append((tt * R ** j + e) % Q)
        for j in range(W):
            ks.append(((R // 2) * R ** j) % Q)
            ks.append((sum((R // 2) * R ** i for i in range(j + 1))) % Q)
            ks.append((sum((R // 2 - 1) * R ** i for i in range(j + 1))) % Q)
        ks += [r2.randrange(Q) for _ in range(700)]
        ks += [r2.randrange(2 ** r2.randrange(1, 255)) for _ in range(150)]
        bad = [Q, Q + 1, 2 ** 255, 2 ** 256 - 1, 2 ** 256 - 2 ** 200] + [r2.randrange(Q, 2 ** 256) for _ in range(150)]
        for k in ks + bad:
            kb = k + bias
            d = [(kb // R ** w) % R - R // 2 for w in range(W - 1)] + [kb // R ** (W - 1)]
            ok = 1 if kb < 1 << 256 and d[W - 1] <= R // 2 else 0
            want = [x & 0xFFFFFFFF for x in d] + [0x7FFFFFFF] * (40 - W) + [ok]
            if k < Q:
                assert ok == 1 and sum(v * R ** w for w, v in enumerate(d)) == k
            # k >= q is not a scalar: the cutter may refuse it or cut it, but never leaves the live buckets (tests/test_radix_digits.py);
            # such rows are compared by that rule, not digit by digit
            t.add(w32(k, 8) + [R] + w32(m, 8) + w32(bias, 8) + [W], want, loose=k >= Q)
    T[t.name] = t


def radix_row_ok(row, got):
    """the rule for a row with k >= q: refused, or every digit within +-R/2 and the top one non-negative"""
    R, W = row[8], row[25]
    if got[40] == 0:
        return True
    d = [x - (1 << 32) if x >> 31 else x for x in got[:W]]
    return got[40] == 1 and all(abs(v) <= R // 2 for v in d) and d[W - 1] >= 0


# ---- all of it ------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def tables(bounds):
    """name -> Table for every entry point; `bounds` is what devcheck_bounds() wrote"""
    if "T" in _CACHE:
        return _CACHE["T"]
    set_bounds(bounds)
    T = {}
    rnd = random.Random(0xDEC0DE)
    field_tables("fp", P, 12, rnd, T)
    field_tables("fr", Q, 8, rnd, T)
    fp28_tables(rnd, T)
    sub, out = curve_points(rnd)
    pairs = g1_tables(rnd, T, sub, out)
    g1_28_tables(rnd, T, pairs, sub, out)
    fr29_tables(rnd, T)
    check_tables(rnd, T, sub, out)
    radix_tables(rnd, T)
    _CACHE["T"] = T
    return T


# predicate -> the entry points whose cases may hit it.  Every one needs MIN_HITS cases unless listed in BOUNDED (a smaller number is
# all that exists) or UNREACHABLE (with the proof).
MIN_HITS = 8


def required_predicates():
    req = []
    for f in ("fp", "fr"):
        req += [(f + "_mul", "sat_final_sub_taken"), (f + "_mul", "sat_final_sub_not_taken"), (f + "_add", "sat_add_final_sub_taken"),
                (f + "_add", "sat_add_final_sub_not_taken"), (f + "_add", "sat_add_operand_eq_modulus"), (f + "_sub", "sat_sub_borrow"), (f + "_sub", "sat_sub_zero")]
    req += [("fr29_add_lazy", p) for p in ("fr29_sum_lt_2q", "fr29_sum_eq_2q", "fr29_sum_gt_2q")]
    req += [("fr29_add_lazy", "fr29_sub_borrow_limb%d" % k) for k in range(9)]
    req += [("fp28_canon", "canon28_borrow_limb%d" % k) for k in range(14)]
    req += [("fp28_mul", "mul28_out_ge_p"), ("fp28_mul", "mul28_out_lt_p")]
    req += [("fp28_mul", "mul28_m%d_%s" % (k, e)) for k in range(14) for e in ("zero", "max")]
    req += [("fp28_mulk12", "norm28_carry_limb%d" % k) for k in range(13)]
    req += [("fp28_chain", "norm28_carry_limb%d" % k) for k in range(13)]
    req += [("g1_decode48", "decode_reason_%d" % k) for k in range(3)] + [("fp28_neg_mul2", "mul28_2_column_ge_70pct_of_static_bound")]
    req += [("g1_is_torsion_free", "torsion_free_yes"), ("g1_is_torsion_free", "torsion_free_no")]
    req += [("fp_sqrt", "sqrt_residue"), ("fp_sqrt", "sqrt_nonresidue")]
    req += [("g1_28_is_identity", "is_identity28_yes"), ("g1_28_is_identity", "is_identity28_no")]
    req += [("g1_add", "g1_add_" + k) for k in ("P+P", "P-P", "P+O", "O+P", "O+O", "P+Q")]
    req += [("fr29_to_sat_canonical", "fr29_canon_sub"), ("fr29_to_sat_canonical", "fr29_canon_keep")]
    return req


# only three integers lie within 1 of (p - 1) / 2, one of them above it: each is in the table once
BOUNDED = {("fp_lex_largest", "lex_near_half_yes"): 1, ("fp_lex_largest", "lex_near_half_no"): 2,
           ("g1_28_is_identity", "is_identity28_lazy_zero"): 5,   # Z = p, 2p, ..., 5p: the non-zero multiples of p below 6p
           ("g1_decode48", "decode_identity"): 1}                 # one byte string encodes the identity

UNREACHABLE = {
    "sat_mul_operand_eq_modulus": "t = (a b + mu m) / R equals m only if m divides a b, i.e. a = 0 or b = 0 for operands below m, and then mu = 0 and t = 0",
    "sat_carry_out_of_top_word": "t < 2m and a + b < 2m, and 2m < 2^(32N) for both fields (q < 2^255, p < 2^381): no carry leaves the top word",
    "decode_reason_3": "g1_decode48 never answers G1_NOT_IN_SUBGROUP: the kernels set it from g1_is_torsion_free (counted as torsion_free_no)",
    "mul28_2_column_in_top_sixteenth_of_2^64": "the static_assert's own column bound for the widest instantiation (g1_28.hpp:92: 14 A B + 14 C D + 14 * 2^56 + 2^40 = 0.60 * 2^64) "
                                               "is below 15/16 * 2^64; and the top limb of a value below VB p is far below LB, so 2 of the 14 products of the widest column are small "
                                               "and no operands within the bounds exceed 12/14 of that bound: mul28_2_column_ge_70pct_of_static_bound is required instead",
}


def mul28_2_static_bound():
    """the left-hand side of mul28_2's static_assert for the instantiation of g1_28.hpp:92"""
    a, b, c, d = BOUNDS["MxT3s"][0], BOUNDS["MxT1s"][0], BOUNDS["MxT4"][0], BOUNDS["MxNy3"][0]
    return 14 * a * b + 14 * c * d + (14 << 56) + (1 << 40)


def check_unreachable():
    """the numeric half of the proofs in UNREACHABLE"""
    assert mul28_2_static_bound() * 16 < 15 << 64          # the widest instantiation's proven column bound is below 15/16 of 2^64
    assert 2 * P < 1 << 384 and 2 * Q < 1 << 256


def run_table(lib, table):
    """one dc_<name> call over the whole table; returns (number of cases compared, list of mismatch descriptions).  Raises on a non-zero
    status: the caller launches nothing more."""
    import ctypes
    rows, want = table.arrays()
    got = np.zeros_like(want)
    fn = getattr(lib, "dc_" + table.name)
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    rc = fn(got.ctypes.data, rows.ctypes.data, len(rows))
    if rc != 0:
        raise RuntimeError("dc_%s returned status %d" % (table.name, rc))
    bad, compared = [], 0
    for k in range(len(rows)):
        ok = radix_row_ok(table.rows[k], [int(x) for x in got[k]]) if table.loose[k] else bool((got[k] == want[k]).all())
        compared += 1
        if not ok:
            hexs = lambda a: " ".join("%08x" % int(x) for x in a)
            bad.append("dc_%s case %d\n  in   %s\n  got  %s\n  want %s" % (table.name, k, hexs(rows[k]), hexs(got[k]), hexs(want[k])))
    return compared, bad

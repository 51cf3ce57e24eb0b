"""Each kernel of csrc/prover_kernels.hpp ALONE on the card, on inputs that satisfy nothing, against Python integers
(tests/provercheck/libprovercheck.so: the product's header, unchanged, built with the product's flags for gfx950 and launched with
the product's launch shapes).  Inside a proof these kernels only ever see a satisfying witness, where the identity they evaluate ties
most terms together, and their index edges show only through the proof's bytes; here every element of every output is compared with
the formula written out below, at the smallest shapes that reach each branch, on uniform random values, all 0, all q - 1 and 1.
Expected values never come from the library or the oracle.  Every output buffer comes back whole: its body was filled with the byte
0xA5 before the launch (so "wrote zero" differs from "wrote nothing") and 8 more elements lie behind it, which must come back as
they were.  No element is skipped or filtered.  A missing library is built; if that fails the test FAILS -- it never skips.  After a
non-zero HIP status nothing more is launched."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from tests import bigint_model as M

pytestmark = pytest.mark.gpu
Q = M.Q
R = 1 << 256
MARGIN = 8
POISON = int.from_bytes(b"\xA5" * 32, "little")               # the image of an element nobody wrote: above q, so no result has it
DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "provercheck")
STATE = {"dead": None}
COMPARED = {}
KERNELS = ("fr_mul_table_pad", "fr_blind", "fr_poke_add", "fr_lincomb", "quotient_coset", "fr_gather_stride", "fr_fold_scale", "coset_recombine")


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(DIR, "libprovercheck.so")
    if not os.path.exists(so):
        try:
            subprocess.check_call(["make", "-C", DIR, "-s", "libprovercheck.so"])
        except Exception as e:                                   # noqa: BLE001 -- any failure to build is a failure of the test
            pytest.fail("tests/provercheck/libprovercheck.so is missing and could not be built with hipcc: %r" % (e,))
    lib = C.CDLL(so)
    assert lib.pc_margin() == MARGIN
    return lib


# ---- Python integers <-> the memory image of fr_t (Montgomery form, four little-endian u64) -------------------------------------
def mont(vals):
    a = np.frombuffer(b"".join((v % Q * R % Q).to_bytes(32, "little") for v in vals), dtype=np.uint64).copy() if len(vals) else np.zeros(0, dtype=np.uint64)
    return a.reshape(-1, 4)


def images(arr):
    b = arr.tobytes()
    return [int.from_bytes(b[32 * i: 32 * i + 32], "little") for i in range(len(b) // 32)]


def run(lib, kernel, entry, count, want, what, *args):
    """one launch through libprovercheck: `count` body elements + the margin come back; all of them are compared with `want` (Python
    integers; None = an element the kernel must not write) and with the margin's fill.  Arrays in args go in as pointers (args keeps them alive over the call)."""
    if STATE["dead"]:
        pytest.fail("not launched: %s" % STATE["dead"])          # after a failed launch nothing more is started on the card
    out = np.zeros((count + MARGIN, 4), dtype=np.uint64)
    fn = getattr(lib, entry)
    fn.restype = C.c_int
    rc = fn(*[C.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else a for a in list(args) + [out]])
    if rc != 0:
        STATE["dead"] = "%s returned HIP status %d (%s)" % (entry, rc, what)
        raise RuntimeError(STATE["dead"])
    got = images(out)
    assert len(want) == count and len(got) == count + MARGIN
    expect = [POISON if v is None else v % Q * R % Q for v in want] + [POISON] * MARGIN
    bad = [i for i in range(count + MARGIN) if got[i] != expect[i]]
    COMPARED[kernel] = COMPARED.get(kernel, 0) + len(got)
    assert not bad, "%s %s: %d of %d elements differ, first at index %d (body = %d): got %064x, want %064x" % (
        kernel, what, len(bad), len(got), bad[0], count, got[bad[0]], expect[bad[0]])


def report(kernel, launches):
    print("pc_%s: %d elements (margins included) compared over %d launches" % (kernel, COMPARED[kernel], launches))


def column(rnd, cls, k):
    """k values of one class: uniform random, all 0, all q - 1, all 1"""
    return [rnd.randrange(Q) for _ in range(k)] if cls == "random" else [{"zero": 0, "minus_one": Q - 1, "one": 1}[cls]] * k


def nonzero(rnd, k):
    return [rnd.randrange(1, Q) for _ in range(k)]


SZ = C.c_size_t


# ---- fr_mul_table_pad: out[i] = in[i] tbl[i] below len, exactly 0 from len to n_out -----------------------------------------
def test_fr_mul_table_pad(lib):
    rnd, launches = random.Random(1), 0
    for length, n_out in ((0, 1), (1, 1), (10, 64), (255, 256), (256, 256), (257, 512), (258, 1024)):
        for cls_in, cls_tbl in (("random", "random"), ("zero", "random"), ("random", "zero"), ("minus_one", "minus_one"), ("one", "random"), ("random", "one")):
            cap = length + 3                                     # three non-zero elements behind len in both inputs: never multiplied in
            a, t = column(rnd, cls_in, length) + nonzero(rnd, 3), column(rnd, cls_tbl, length) + nonzero(rnd, 3)
            want = [a[i] * t[i] if i < length else 0 for i in range(n_out)]
            run(lib, "fr_mul_table_pad", "pc_mul_table_pad", n_out, want, "len %d n_out %d %s x %s" % (length, n_out, cls_in, cls_tbl),
                mont(a), mont(t), SZ(cap), SZ(length), SZ(n_out))
            launches += 1
    report("fr_mul_table_pad", launches)


# ---- fr_blind: out = base + (c0 + c1 x + c2 x^2)(x^n - 1): n + k coefficients, lanes n + k .. n + 8 write nothing -----------
def test_fr_blind(lib):
    rnd, launches = random.Random(2), 0
    for n in (8, 256, 512):
        for k in (2, 3):
            for cls_base, cls_c in (("random", "random"), ("random", "zero"), ("random", "minus_one"), ("zero", "random"), ("zero", "minus_one"),
                                    ("minus_one", "random"), ("minus_one", "minus_one"), ("one", "one"), ("zero", "zero")):
                base, c = column(rnd, cls_base, n), column(rnd, cls_c, 3)
                if k == 2:
                    c[2] = rnd.randrange(1, Q)                   # not part of a two-term blinding: must be ignored
                want = list(base) + [0] * k
                for j in range(k):
                    want[j] -= c[j]                              # base = 0 there: the subtraction borrows
                    want[n + j] += c[j]
                run(lib, "fr_blind", "pc_blind", n + k, want, "n %d k %d base %s c %s" % (n, k, cls_base, cls_c), mont(base), SZ(n), mont(c), C.c_uint32(k))
                launches += 1
    report("fr_blind", launches)


# ---- fr_poke_add: p[0] += v, nothing else ----------------------------------------------------------------------------------
def test_fr_poke_add(lib):
    rnd, launches = random.Random(3), 0
    for p0, v in ((Q - 1, 1), (1, Q - 1), (0, 0), (Q - 1, Q - 1), (0, Q - 1), (rnd.randrange(Q), rnd.randrange(Q)), (rnd.randrange(Q), 0)):
        p1 = rnd.randrange(1, Q)
        run(lib, "fr_poke_add", "pc_poke_add", 2, [p0 + v, p1], "%x + %x" % (p0, v), mont([p0, p1]), mont([v]))
        launches += 1
    report("fr_poke_add", launches)


# ---- fr_lincomb: out[i] = sum_k c_k p_k[i] [i < len_k] + constant [i == 0] ---------------------------------------------------
@pytest.mark.parametrize("terms", [0, 1, 15, 16])
def test_fr_lincomb(lib, terms):
    rnd, launches = random.Random(40 + terms), 0
    for n_out in (1, 11, 256, 257, 520):
        options = sorted({0, 1, max(n_out - 3, 0), n_out})
        cap = n_out + 5                                          # every polynomial lies in a larger allocation: poison behind its len
        for cls in ("random", "zero", "minus_one", "one"):
            # every length option at every term count: terms >= 15 cycle through them in one launch, one term takes them in turn
            shifts = range(len(options)) if terms == 1 else (rnd.randrange(4),)
            for shift in shifts:
                lens = [options[(k + shift) % len(options)] for k in range(terms)]
                polys = [column(rnd, cls, lens[k]) + nonzero(rnd, cap - lens[k]) for k in range(terms)]
                coef = column(rnd, "random" if cls == "zero" else cls, terms)
                const = column(rnd, "random" if cls in ("zero", "one") else cls, 1)[0]
                want = [sum(coef[k] * polys[k][i] for k in range(terms) if i < lens[k]) + (const if i == 0 else 0) for i in range(n_out)]
                flat = mont([v for p in polys for v in p])
                lens_a = np.array(lens + [0], dtype=np.uint64)
                run(lib, "fr_lincomb", "pc_lincomb", n_out, want, "terms %d n_out %d lens %s %s" % (terms, n_out, lens, cls),
                    flat, SZ(cap), lens_a, mont(coef + [0]), mont([const]), C.c_int(terms), SZ(n_out))
                launches += 1
    report("fr_lincomb", launches)


# ---- quotient_coset: prover.rs:370-450 term by term ------------------------------------------------------------------------------
WIT = ("a", "b", "c", "z", "PI")
PRE = ("ql", "qr", "qm", "qo", "qc", "s1", "s2", "s3", "L1")


def quotient_formula(v, N, alpha, beta, gamma, zh_inv, zshift):
    out = []
    for i in range(N):
        a, b, c, z, pi = (v[k][i] for k in WIT)
        zw = v["z"][(i + zshift) % N]                            # z(w X): zshift places further ROUND the coset
        x = v["xs"][i]
        gate = a * v["ql"][i] + b * v["qr"][i] + a * b * v["qm"][i] + c * v["qo"][i] + pi + v["qc"][i]
        perm = ((a + beta * x + gamma) * (b + 2 * beta * x + gamma) * (c + 3 * beta * x + gamma) * z
                - (a + beta * v["s1"][i] + gamma) * (b + beta * v["s2"][i] + gamma) * (c + beta * v["s3"][i] + gamma) * zw)
        first = (z - 1) * v["L1"][i]
        out.append((gate + alpha * perm + alpha * alpha * first) % Q * zh_inv[i & 3])
    return out


@pytest.mark.parametrize("N,zshift", [(32, 4), (256, 4), (1024, 4), (8, 1), (256, 1), (512, 1)])
def test_quotient_coset(lib, N, zshift):
    rnd, launches = random.Random(500 + N + zshift), 0
    names = WIT + PRE + ("xs",)

    def launch(v, ch, zh_inv, what):
        wit = mont([x for k in WIT for x in v[k]])
        pre = mont([x for k in PRE for x in v[k]])
        run(lib, "quotient_coset", "pc_quotient_coset", N, quotient_formula(v, N, *ch, zh_inv, zshift), "N %d zshift %d %s" % (N, zshift, what),
            wit, pre, mont(v["xs"]), SZ(N), mont(ch[:1]), mont(ch[1:2]), mont(ch[2:]), mont(zh_inv), C.c_uint32(zshift))

    def challenges():
        ch = nonzero(rnd, 3)
        zh = nonzero(rnd, 1) * 4 if zshift == 1 else nonzero(rnd, 4)     # one coset s_j <w_n>: X^n - 1 is one value; g <w_4n>: four
        assert zshift == 1 or len(set(zh)) == 4
        return ch, zh

    # inputs that satisfy nothing, per value class; the challenges stay random so that no term is switched off by them
    for cls in ("random", "zero", "minus_one", "one"):
        ch, zh = challenges()
        launch({k: column(rnd, cls, N) for k in names}, ch, zh, cls)
        launches += 1
    ch, zh = [Q - 1] * 3, [Q - 1] * 4                                # and the challenges themselves at q - 1 and at 1 on random columns
    launch({k: column(rnd, "random", N) for k in names}, ch, zh, "challenges q - 1")
    launch({k: column(rnd, "random", N) for k in names}, [1, 1, 1], [1] * 4, "challenges 1")
    launches += 2
    # z == 1: the first-row term vanishes and z(w X) = z
    v = {k: column(rnd, "random", N) for k in names}
    v["z"] = [1] * N
    ch, zh = challenges()
    launch(v, ch, zh, "z = 1")
    launches += 1
    # the wrap of z(w X): z is zero except in its first zshift places, which only the LAST zshift lanes read as z(w X)
    v = {k: column(rnd, "random", N) for k in names}
    v["z"] = nonzero(rnd, zshift) + [0] * (N - zshift)
    ch, zh = challenges()
    want = quotient_formula(v, N, *ch, zh, zshift)
    without = quotient_formula(dict(v, z=[0] * N), N, *ch, zh, zshift)
    assert all(want[i] != without[i] for i in range(N - zshift, N))                 # the expected values do depend on the wrapped read
    launch(v, ch, zh, "z(wX) wraps")
    launches += 1
    # one input column alive at a time, the others all 0 and then all 1: each column is tied to its own term
    for alive in names:
        for rest in (0, 1):
            v = {k: [rest] * N for k in names}
            v[alive] = nonzero(rnd, N)
            ch, zh = challenges()
            launch(v, ch, zh, "only %s alive, the rest %d" % (alive, rest))
            launches += 1
    report("quotient_coset", launches)


# ---- fr_gather_stride: out[i] = in[stride i + offset] --------------------------------------------------------------------------
def test_fr_gather_stride(lib):
    rnd, launches = random.Random(6), 0
    for n in (1, 255, 256, 257):
        for offset in range(4):
            for cls in ("random", "zero", "minus_one"):
                src = column(rnd, cls, 4 * n)
                run(lib, "fr_gather_stride", "pc_gather_stride", n, [src[4 * i + offset] for i in range(n)], "n %d offset %d %s" % (n, offset, cls),
                    mont(src), SZ(4 * n), SZ(4), SZ(offset), SZ(n))
                launches += 1
    report("fr_gather_stride", launches)


# ---- fr_fold_scale: out[i] = (c[i] + c[i + n] s^n) s^i, coefficients from len on are zero ------------------------------------
@pytest.mark.parametrize("n", [8, 256, 512])
def test_fr_fold_scale(lib, n):
    rnd, launches = random.Random(70 + n), 0
    for length in (0, 1, n - 1, n, n + 1, n + 3, 2 * n - 1):
        for cls in ("random", "zero", "minus_one", "one"):
            cap = 2 * n + 2                                      # non-zero elements behind len: c[i] and c[i + n] there count as zero
            c = column(rnd, cls, length) + nonzero(rnd, cap - length)
            if cls == "random":                                  # a real coset shift: spow[i] = s^i and s_n = s^n
                s = rnd.randrange(2, Q)
                spow, s_n = [pow(s, i, Q) for i in range(n)], pow(s, n, Q)
            else:
                spow, s_n = column(rnd, cls if cls != "zero" else "random", n), column(rnd, cls if cls != "zero" else "random", 1)[0]
            want = [((c[i] if i < length else 0) + (c[i + n] * s_n if i + n < length else 0)) * spow[i] for i in range(n)]
            run(lib, "fr_fold_scale", "pc_fold_scale", n, want, "n %d len %d %s" % (n, length, cls), mont(c), SZ(cap), SZ(length), SZ(n), mont([s_n]), mont(spow))
            launches += 1
    report("fr_fold_scale", launches)


# ---- coset_recombine: t from its four residues w_j = t mod (x^n - G i4^j) ------------------------------------------------------
def test_coset_recombine(lib):
    rnd, launches = random.Random(8), 0
    for n in (1, 8, 256, 512):
        i4 = pow(M.omega(4 * n), n, Q)
        assert i4 * i4 % Q == Q - 1
        for cls, G in (("random", pow(7, n, Q)), ("random", rnd.randrange(2, Q)), ("zero", pow(7, n, Q)), ("minus_one", pow(7, n, Q)), ("one", pow(7, n, Q)),
                       ("random", 1), ("random", Q - 1)):
            t = column(rnd, cls, 4 * n)                          # t_m = t[m n .. (m + 1) n)
            w = [sum(pow(G, m, Q) * pow(i4, j * m, Q) * t[m * n + i] for m in range(4)) % Q for j in range(4) for i in range(n)]
            scale = [pow(pow(G, m, Q) * 4, Q - 2, Q) for m in range(4)]
            run(lib, "coset_recombine", "pc_coset_recombine", 4 * n, t, "n %d G %x %s" % (n, G, cls), mont(w), SZ(n), mont(scale), mont([pow(i4, Q - 2, Q)]))
            launches += 1
    report("coset_recombine", launches)


def test_every_kernel_was_compared():
    print("prover kernel check: %s" % ", ".join("%s %d" % (k, COMPARED.get(k, 0)) for k in KERNELS))
    assert STATE["dead"] is None and all(COMPARED.get(k, 0) > 0 for k in KERNELS)

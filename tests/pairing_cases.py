"""Shared ground truth of the pairing tests (not a test module): the reference's literals (tests/golden/pairing_kats.json), byte
forms for the Python model (tests/tower_model.py), pairs with KNOWN verdicts, and the host shim's build.

Pairs.  The crate's fixture holds i G for i < 1000 as 96-byte records, so with the setup secret tau = 7 the pair
(A, B) = (a G, (7 a + delta) G) is two fixture records for a <= 140: x_2 = 7 G2, and the check passes iff delta = 0 -- no
expectation comes from the code under test, and no elliptic-curve arithmetic runs in Python to build a case."""
import json
import os
import random
import subprocess

from tests import bigint_model as M
from tests import tower_model as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
P, Q = M.P, M.Q
RP = 1 << 384
KATS = json.load(open(os.path.join(GOLDEN, "pairing_kats.json")))
ID96, ID192 = bytes([0x40]) + bytes(95), bytes([0x40]) + bytes(191)
TAU = 7


def fp_of(limbs):
    """a literal of the reference (six 64-bit Montgomery limbs) as the integer it stands for"""
    return sum(int(x, 16) << (64 * i) for i, x in enumerate(limbs)) * pow(RP, -1, P) % P


def kat(fname, name):
    """the Fp literals of one extracted function, as integers, in source order"""
    return [fp_of(l) for l in KATS[fname][name]["fp"]]


def fp_bytes(v):
    """memory image of an Fp: Montgomery form, 48 little-endian bytes"""
    return (v * RP % P).to_bytes(48, "little")


def fp_from(b):
    return int.from_bytes(b, "little") * pow(RP, -1, P) % P


def f2_bytes(a):
    return fp_bytes(a[0]) + fp_bytes(a[1])


def f6_bytes(a):
    return b"".join(f2_bytes(c) for c in a)


def f12_bytes(a):
    return b"".join(f6_bytes(h) for h in a)


def f2_from(b):
    return (fp_from(b[:48]), fp_from(b[48:96]))


def f6_from(b):
    return tuple(f2_from(b[96 * k: 96 * k + 96]) for k in range(3))


def f12_from(b):
    return (f6_from(b[:288]), f6_from(b[288:576]))


def g2_generator():
    v = kat("g2.rs", "G2Affine::generator")
    return ((v[0], v[1]), (v[2], v[3]))


G2 = g2_generator()
GT_GENERATOR = b"".join(fp_bytes(v) for v in kat("pairings.rs", "Gt::generator"))      # pairing(G1 generator, G2 generator)
GT_ONE = f12_bytes(T.F12_ONE)


def fixture96():
    blob = open(os.path.join(GOLDEN, "g1_uncompressed_valid_test_vectors.dat"), "rb").read()
    assert len(blob) == 96000
    return [blob[96 * i: 96 * i + 96] for i in range(1000)]


FX96 = fixture96()
KINDS = ("valid", "invalid", "both_identity", "a_identity", "b_identity")


def mixed_pairs(n, seed):
    """n pairs for x_2 = TAU G2 with their verdicts: a seeded mix of the five kinds, each present once n >= 5"""
    rnd = random.Random(seed)
    kinds = [KINDS[i % 5] for i in range(n)]
    rnd.shuffle(kinds)
    pairs, truth = [], []
    for kind in kinds:
        a = rnd.randrange(1, 141)
        A, B = FX96[a], FX96[TAU * a]
        if kind == "invalid":
            B = FX96[TAU * a + rnd.randrange(1, 13)]
        elif kind == "both_identity":
            A, B = ID96, ID96
        elif kind == "a_identity":
            A = ID96
        elif kind == "b_identity":
            B = ID96
        pairs.append(A + B)
        truth.append(kind in ("valid", "both_identity"))
    return b"".join(pairs), truth


def off_curve96():
    """a canonical (x, y) that misses the curve: the generator with y + 1"""
    return M.GX.to_bytes(48, "big") + (M.GY + 1).to_bytes(48, "big")


def outside_subgroup96():
    """a point of y^2 = x^3 + 4 outside the prime-order subgroup (the cofactor is ~2^126: the first curve point found by x is one)"""
    x = 0
    while True:
        x += 1
        rhs = (x * x * x + 4) % P
        y = pow(rhs, (P + 1) // 4, P)
        if y * y % P != rhs:
            continue
        acc, pt, k = None, (x, y), Q                                # [q] P without reducing q (bigint_model.ec_mul reduces its scalar)
        while k:
            if k & 1:
                acc = M.ec_add(acc, pt)
            pt, k = M.ec_add(pt, pt), k >> 1
        if acc is not None:
            return x.to_bytes(48, "big") + y.to_bytes(48, "big")


def build_shim(tmp_dir):
    """tests/cpp/tower_host.hip compiled for the host alone; None where there is no hipcc"""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        return None
    so = os.path.join(str(tmp_dir), "libtower_host.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O1", "-fPIC", "-shared",
                           os.path.join(ROOT, "tests", "cpp", "tower_host.hip"), "-o", so])
    return so

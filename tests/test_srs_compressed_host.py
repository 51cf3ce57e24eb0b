"""CPU checks of the compressed-SRS path (bp_srs_load_compressed48 / bp_srs_check_subgroup / bp_srs_export_compressed48), no GPU:
the entry points refuse bad arguments, and the __host__ __device__ arithmetic the kernels run (csrc/g1_check.hpp: square root,
compressed decode / encode, mul_by_x, is_torsion_free) is compiled for the host with the device's column multiplier and compared
with plain Python integers (tests/bigint_model.py) and the crate's own 1000-point fixture."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import baby_plonk_rust_amd as bp
from baby_plonk_rust_amd import _lib
from tests import bigint_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
P = M.P
R = 1 << 384
X_ABS = 0xD201000000010000                   # |x| of the BLS parameter x = -0xd201000000010000
H = 0x396C8C005555E1568C00AAAB0000AAAB       # cofactor of E(Fp) over G1
SIZE_MAX = 2**64 - 1


def limbs(v, n=12):
    return np.array([(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)], dtype=np.uint32)


def unlimbs(a):
    return sum(int(x) << (32 * i) for i, x in enumerate(a))


def mont(v):
    return limbs(v * R % P)


def unmont(a):
    return unlimbs(a) * pow(R, -1, P) % P


def dev_affine(pt):
    """device affine form: x | y Montgomery, the identity (0, 0)"""
    return np.zeros(24, dtype=np.uint32) if pt is None else np.concatenate([mont(pt[0]), mont(pt[1])])


def from_dev_affine(a):
    return None if not a.any() else (unmont(a[:12]), unmont(a[12:]))


def ec_mul_unreduced(k, pt):
    """double-and-add WITHOUT reducing k mod r (bigint_model.ec_mul does, so [r]P through it is always O)"""
    acc = None
    while k:
        if k & 1:
            acc = M.ec_add(acc, pt)
        pt = M.ec_add(pt, pt)
        k >>= 1
    return acc


def random_curve_point(rnd):
    while True:
        x = rnd.randrange(P)
        rhs = (x ** 3 + 4) % P
        y = pow(rhs, (P + 1) // 4, P)
        if y * y % P == rhs:
            return (x, y if rnd.random() < 0.5 else P - y)


@pytest.fixture(scope="module")
def gc(tmp_path_factory):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    so = str(tmp_path_factory.mktemp("g1_check") / "libg1check.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O1", "-fPIC", "-shared",
                           os.path.join(ROOT, "tests", "cpp", "g1_check_host.hip"), "-o", so])
    lib = C.CDLL(so)
    vp = C.c_void_p
    for name, res, args in (("gc_fp_sqrt", C.c_int, [vp, vp]), ("gc_fp_beta", None, [vp]), ("gc_decode48", C.c_uint32, [vp, vp]),
                            ("gc_encode48", None, [vp, vp]), ("gc_mul_by_x", None, [vp, vp]), ("gc_is_torsion_free", C.c_int, [vp])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def decode(gc, rec):
    buf, out = np.frombuffer(bytes(rec), dtype=np.uint8).copy(), np.zeros(24, dtype=np.uint32)
    reason = gc.gc_decode48(out.ctypes.data, buf.ctypes.data)
    return reason, from_dev_affine(out)


def encode(gc, pt):
    a, out = dev_affine(pt), np.zeros(48, dtype=np.uint8)
    gc.gc_encode48(out.ctypes.data, a.ctypes.data)
    return bytes(out)


def torsion_free(gc, pt):
    a = dev_affine(pt)
    return bool(gc.gc_is_torsion_free(a.ctypes.data))


def test_entry_points_refuse_null_arguments():
    """BP_ERR_INVALID_ARG on a NULL context or NULL buffers, first_bad = SIZE_MAX whenever it is given"""
    lib = bp.load()
    h, bad = C.c_uint64(), C.c_size_t(7)
    buf = np.zeros(48, dtype=np.uint8)
    assert lib.bp_srs_load_compressed48(None, buf.ctypes.data, 1, 1, C.byref(h), C.byref(bad)) == -1 and bad.value == SIZE_MAX
    assert lib.bp_srs_load_compressed48(None, None, 1, 0, C.byref(h), None) == -1
    assert lib.bp_srs_load_compressed48(None, buf.ctypes.data, 1, 1, None, None) == -1
    bad.value = 7
    assert lib.bp_srs_check_subgroup(None, 1, 0, 1, C.byref(bad)) == -1 and bad.value == SIZE_MAX
    assert lib.bp_srs_check_subgroup(None, 1, 0, 1, None) == -1
    assert lib.bp_srs_export_compressed48(None, 1, 0, 1, buf.ctypes.data) == -1
    assert lib.bp_srs_export_compressed48(None, 1, 0, 1, None) == -1
    assert _lib.SRS_CHECK_SUBGROUP == 1
    assert "#define BP_SRS_CHECK_SUBGROUP 1u" in open(os.path.join(ROOT, "include", "bp_msm_ntt.h")).read()


def test_fp_sqrt_against_pow(gc):
    rnd = random.Random(71)
    vals = [0, 1, 4, P - 1, P - 4, (P - 1) // 2, 2, 3] + [rnd.randrange(P) for _ in range(120)]
    vals += [v * v % P for v in vals[:40]]                       # certain residues
    residues = 0
    for v in vals:
        s = np.zeros(12, dtype=np.uint32)
        ok = gc.gc_fp_sqrt(s.ctypes.data, mont(v).ctypes.data)
        want = pow(v, (P + 1) // 4, P)
        assert unmont(s) == want, v
        is_res = want * want % P == v
        assert bool(ok) == is_res, v
        residues += is_res
    assert 40 < residues < len(vals) - 40                         # both kinds were exercised


def test_decode_and_encode_the_crate_fixture(gc):
    """g1_decode48 over the crate's 1000 compressed points (i G, point 0 = identity) gives the uncompressed twin; g1_encode48 gives
    the compressed records back"""
    comp = open(os.path.join(GOLDEN, "g1_compressed_valid_test_vectors.dat"), "rb").read()
    unc = open(os.path.join(GOLDEN, "g1_uncompressed_valid_test_vectors.dat"), "rb").read()
    for i in range(0, 1000, 3):
        rec, u = comp[48 * i: 48 * i + 48], unc[96 * i: 96 * i + 96]
        reason, pt = decode(gc, rec)
        assert reason == 0, i
        assert M.enc96(pt) == u, i
        assert encode(gc, pt) == rec, i
        assert M.enc48(pt) == rec and M.dec48(rec) == pt, i


def test_decode_rejection_rules(gc):
    """from_compressed_unchecked (g1.rs:337-390): reason 1 for the encoding, 2 for no square root; the sort flag picks -P"""
    rnd = random.Random(72)
    pt = M.ec_mul(12345)
    good = M.enc48(pt)
    assert decode(gc, good) == (0, pt)
    flipped = bytes([good[0] ^ 0x20]) + good[1:]
    assert decode(gc, flipped) == (0, (pt[0], P - pt[1]))
    assert decode(gc, bytes([0xC0]) + bytes(47)) == (0, None)
    cases = [bytes([good[0] & 0x7F]) + good[1:],                  # compression flag cleared
             bytes([good[0] | 0x40]) + good[1:],                  # infinity flag with x != 0
             bytes([0xE0]) + bytes(47), bytes([0x40]) + bytes(47), bytes(48),
             bytes([0x80 | (P >> 376)]) + (P % (1 << 376)).to_bytes(47, "big"),                    # masked x = p
             bytes([0x9F]) + bytes([0xFF] * 47)]                                                   # masked x = 2^381 - 1
    for c in cases:
        assert decode(gc, c) == (1, None), c.hex()
    n_bad = 0
    while n_bad < 20:
        x = rnd.randrange(P)
        rhs = (x ** 3 + 4) % P
        if pow(rhs, (P - 1) // 2, P) == P - 1:                   # x^3 + 4 is a non-residue
            rec = bytearray(x.to_bytes(48, "big"))
            rec[0] |= 0x80 | (0x20 if rnd.random() < 0.5 else 0)
            assert decode(gc, rec) == (2, None), x
            n_bad += 1


def derive_beta():
    """beta = g^((p-1)/3) for a non-cube g, of beta and beta^2 the one with phi(G) = -[x^2] G -- recomputed from the group law"""
    g = 2
    while pow(g, (P - 1) // 3, P) == 1:
        g += 1
    b = pow(g, (P - 1) // 3, P)
    assert b != 1 and b * b * b % P == 1
    G = (M.GX, M.GY)
    x2g = ec_mul_unreduced(X_ABS * X_ABS, G)
    match = [c for c in (b, b * b % P) if x2g == (c * M.GX % P, (P - M.GY) % P)]
    assert len(match) == 1
    return match[0]


def test_beta_in_the_header_is_rederived(gc):
    out = np.zeros(12, dtype=np.uint32)
    gc.gc_fp_beta(out.ctypes.data)
    assert unlimbs(out) == derive_beta()


def test_mul_by_x_and_subgroup_check(gc):
    """g1_mul_by_x = [|x|] P; g1_is_torsion_free on i G, on random curve points (almost none lie in G1), on [h] times them"""
    rnd = random.Random(73)
    for pt in (M.ec_mul(1), M.ec_mul(rnd.randrange(M.Q)), random_curve_point(rnd), None):
        a = np.zeros(36, dtype=np.uint32)
        if pt is None:
            a[12:24] = mont(1)                                     # (0 : 1 : 0)
        else:
            a[:12], a[12:24], a[24:] = mont(pt[0]), mont(pt[1]), mont(1)
        out = np.zeros(36, dtype=np.uint32)
        gc.gc_mul_by_x(out.ctypes.data, a.ctypes.data)
        z = unmont(out[24:])
        want = ec_mul_unreduced(X_ABS, pt) if pt is not None else None
        if want is None:
            assert z == 0
        else:
            zi = pow(z, P - 2, P)
            assert (unmont(out[:12]) * zi % P, unmont(out[12:24]) * zi % P) == want
    for i in [0, 1, 2, 3, 999] + [rnd.randrange(1, M.Q) for _ in range(6)]:
        assert torsion_free(gc, M.ec_mul(i)), i
    outside = [random_curve_point(rnd) for _ in range(12)]
    for q in outside:
        assert ec_mul_unreduced(M.Q, q) is not None                # really outside G1: [r] Q != O
        assert not torsion_free(gc, q)
        hq = M.ec_mul(H, q)                                       # H < r: ec_mul's reduction leaves it alone
        assert ec_mul_unreduced(M.Q, hq) is None
        assert torsion_free(gc, hq)
        assert not torsion_free(gc, M.ec_add(hq, q))         # in G1 + outside = outside

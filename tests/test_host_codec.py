"""CPU checks of csrc/host_codec.hpp, the host code that decides every byte the C ABI takes or returns (points in 96 and 48 bytes,
scalars in both formats, root_of_unity), no GPU: the header is compiled for the host alone (tests/cpp/host_codec_host.hip) and
compared with the crate's two 1000-point fixtures, plain Python integers and tests/bigint_model.py.  No expectation comes from the
code under test: inputs are built from Python integers too (projective points with a random z)."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from tests import bigint_model as M
from tests.test_srs_compressed_host import ec_mul_unreduced, random_curve_point

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
P, Q = M.P, M.Q
RP, RQ = 1 << 384, 1 << 256                  # the Montgomery radices of Fp and Fr
FR_BYTES_LE, FR_MONT = 0, 1                  # include/bp_msm_ntt.h
ID48, ID96 = bytes([0xC0]) + bytes(47), bytes([0x40]) + bytes(95)
POISON = bytes([0xEE])                       # what the wrappers fill an output with before a call that may refuse


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    so = str(tmp_path_factory.mktemp("host_codec") / "libhostcodec.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O1", "-fPIC", "-shared",
                           os.path.join(ROOT, "tests", "cpp", "host_codec_host.hip"), "-o", so])
    lib = C.CDLL(so)
    cp, i32, u64 = C.c_char_p, C.c_int, C.c_uint64
    for name, res, args in (("hc_compress_block", i32, []), ("hc_decode96", i32, [cp, cp]), ("hc_encode96", None, [cp, cp]),
                            ("hc_on_curve", i32, [cp]), ("hc_compress48", None, [cp, cp]), ("hc_batch_to_affine", None, [cp, cp, i32]),
                            ("hc_compress48_many", None, [cp, cp, i32]), ("hc_fr_is_canonical", i32, [cp]),
                            ("hc_fr_from_bytes", i32, [cp, cp, i32]), ("hc_fr_to_bytes", None, [cp, cp, i32]),
                            ("hc_fr_from_u64", None, [cp, u64]), ("hc_fr_pow_u64", None, [cp, cp, u64]),
                            ("hc_root_of_unity", i32, [cp, u64])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


@pytest.fixture(scope="module")
def vectors():
    """the crate's fixtures: record i is i G (record 0 the identity), uncompressed and compressed"""
    unc = open(os.path.join(GOLDEN, "g1_uncompressed_valid_test_vectors.dat"), "rb").read()
    comp = open(os.path.join(GOLDEN, "g1_compressed_valid_test_vectors.dat"), "rb").read()
    assert len(unc) == 96000 and len(comp) == 48000
    return [unc[96 * i: 96 * i + 96] for i in range(1000)], [comp[48 * i: 48 * i + 48] for i in range(1000)]


def fp_mont(v):
    return (v * RP % P).to_bytes(48, "little")


def fr_mont(v):
    return (v * RQ % Q).to_bytes(32, "little")


def fr_unmont(b):
    return int.from_bytes(b, "little") * pow(RQ, -1, Q) % Q


def point_of(rec96):
    """the affine pair of an uncompressed record as Python integers; None for the identity record"""
    if rec96[0] & 0x40:
        return None
    return int.from_bytes(rec96[:48], "big"), int.from_bytes(rec96[48:], "big")


def proj(pt, z=1, junk=(0, 1)):
    """memory image of g1_proj for pt scaled by z; the identity is (junk_x : junk_y : 0)"""
    if pt is None:
        return fp_mont(junk[0]) + fp_mont(junk[1]) + fp_mont(0)
    return fp_mont(pt[0] * z % P) + fp_mont(pt[1] * z % P) + fp_mont(z)


def affine(pt):
    return bytes(96) if pt is None else fp_mont(pt[0]) + fp_mont(pt[1])


def decode96(hc, rec):
    out = C.create_string_buffer(144)
    return bool(hc.hc_decode96(out, bytes(rec))), out.raw


def encode96(hc, p144):
    out = C.create_string_buffer(96)
    hc.hc_encode96(out, p144)
    return out.raw


def compress48(hc, p144):
    out = C.create_string_buffer(48)
    hc.hc_compress48(out, p144)
    return out.raw


def compress48_many(hc, projs):
    out = C.create_string_buffer(48 * len(projs) + 16)                # 16 guard bytes behind the last record
    out.raw = bytes(48 * len(projs)) + bytes([0xA5] * 16)
    hc.hc_compress48_many(out, b"".join(projs), len(projs))
    assert out.raw[48 * len(projs):] == bytes([0xA5] * 16)
    return [out.raw[48 * j: 48 * j + 48] for j in range(len(projs))]


def test_all_fixture_points_in_96_and_48_bytes(hc, vectors):
    """decode96 gives (x R, y R, R) of the record's integers; encode96 gives the record back; compress48 of the same point -- as
    decoded, and rescaled by a random z -- is the compressed fixture's record"""
    unc, comp = vectors
    rnd = random.Random(81)
    for i in range(1000):
        ok, p = decode96(hc, unc[i])
        assert ok, i
        pt = point_of(unc[i])
        assert (pt is None) == (i == 0)
        assert p == proj(pt), i
        assert encode96(hc, p) == unc[i], i
        assert compress48(hc, p) == comp[i], i
        scaled = proj(pt, rnd.randrange(1, P), (rnd.randrange(P), rnd.randrange(P)))
        assert encode96(hc, scaled) == unc[i], i
        assert compress48(hc, scaled) == comp[i], i
    assert unc[0] == ID96 and comp[0] == ID48


def test_sign_bit_of_compress48_is_y_above_minus_y(hc):
    """one sign rule: set iff y > p - y.  (0, 2) and (0, p - 2) are on the curve -- x = 0 with either sign -- and no affine point has
    y = 0 (x^3 = -4 has no root: p = 1 mod 3 and (-4)^((p-1)/3) != 1), so y = 0 is fed in as limbs only"""
    assert pow(P - 4, (P - 1) // 3, P) != 1
    for pt in ((0, 2), (0, P - 2), (5, 0), (5, (P - 1) // 2), (5, (P + 1) // 2), (5, P - 1), (5, 1)):
        want = bytearray(pt[0].to_bytes(48, "big"))
        want[0] |= 0x80 | (0x20 if pt[1] > (P - pt[1]) % P else 0)
        assert compress48(hc, proj(pt)) == bytes(want), pt
        assert compress48_many(hc, [proj(pt, 3)]) == [bytes(want)], pt
    assert hc.hc_on_curve(affine((0, 2))) and hc.hc_on_curve(affine((0, P - 2))) and not hc.hc_on_curve(affine((5, 1)))


def test_batch_to_affine_one_inversion_many_points(hc, vectors):
    """host_batch_to_affine: (x / z, y / z) in Montgomery limbs, the identity as (0, 0), for any k (no bound of its own)"""
    unc, _ = vectors
    rnd = random.Random(82)
    for k in (0, 1, 2, 5, 16, 17, 40):
        pts = [None if rnd.random() < 0.2 else point_of(unc[rnd.randrange(1, 1000)]) for _ in range(k)]
        out = C.create_string_buffer(96 * k + 16)
        out.raw = bytes([0xEE] * (96 * k)) + bytes([0xA5] * 16)
        hc.hc_batch_to_affine(out, b"".join(proj(pt, rnd.randrange(1, P), (rnd.randrange(P), rnd.randrange(P))) for pt in pts), k)
        assert out.raw == b"".join(affine(pt) for pt in pts) + bytes([0xA5] * 16), k


def test_compress48_many_equals_the_per_point_records(hc, vectors):
    """consecutive fixture batches of every size up to and past the block (one inversion per block of 16), each point under its own
    random z: the records are the compressed fixture's"""
    unc, comp = vectors
    block = hc.hc_compress_block()
    assert block == 16
    rnd = random.Random(83)
    at = 1
    for k in (1, 2, 3, 7, 16, block, block + 1, 2 * block, 2 * block + 1):
        projs = [proj(point_of(unc[i]), rnd.randrange(1, P)) for i in range(at, at + k)]
        assert compress48_many(hc, projs) == comp[at: at + k], k
        at += k
    assert compress48_many(hc, []) == []


def test_compress48_many_with_identities(hc, vectors):
    """the identity first, in the middle, last and in every slot, as (0 : 1 : 0) and as (x : y : 0); also on both sides of a block
    boundary.  Its record is 0xc0 and 47 zeros, the others are untouched by it"""
    unc, comp = vectors
    rnd = random.Random(84)
    for k in (1, 2, 3, 7, 16, 17):
        base = rnd.randrange(1, 1000 - k)
        slots = {0, k // 2, k - 1}
        for holes in [{s} for s in sorted(slots)] + [slots, set(range(k))] + ([{15, 16}] if k == 17 else []):
            projs, want = [], []
            for j in range(k):
                if j in holes:
                    projs.append(proj(None, junk=(0, 1) if rnd.random() < 0.5 else (rnd.randrange(P), rnd.randrange(P))))
                    want.append(ID48)
                else:
                    projs.append(proj(point_of(unc[base + j]), rnd.randrange(1, P)))
                    want.append(comp[base + j])
            assert compress48_many(hc, projs) == want, (k, holes)
    assert compress48(hc, proj(None)) == ID48 and compress48(hc, proj(None, junk=(7, 9))) == ID48
    assert encode96(hc, proj(None)) == ID96 and encode96(hc, proj(None, junk=(7, 9))) == ID96


def test_decode96_refusals_and_the_curve_check(hc):
    """from_uncompressed_unchecked (g1.rs:273-322): canonical coordinates and flags only -- the curve equation is
    g1_affine_on_curve's, the subgroup nobody's here"""
    rnd = random.Random(85)
    pt = M.ec_mul(4242)
    good = M.enc96(pt)
    assert decode96(hc, good) == (True, proj(pt))

    def with_xy(x, y):
        return x.to_bytes(48, "big") + y.to_bytes(48, "big")

    refused = [with_xy(P, pt[1]), with_xy(pt[0], P), with_xy(P, P), with_xy((1 << 381) - 1, pt[1]), with_xy(pt[0], (1 << 384) - 1)]
    refused += [bytes([good[0] | bit]) + good[1:] for bit in (0x80, 0x40, 0x20)]             # each flag alone, on a real point
    refused += [bytes([bit]) + bytes(95) for bit in (0x80, 0x20, 0xC0, 0x60, 0xE0)]
    refused += [bytes([0x40]) + bytes(46) + bytes([1]) + bytes(48), bytes([0x40]) + bytes(94) + bytes([1]),   # infinity, x or y != 0
                bytes([0x40]) + good[1:]]
    for rec in refused:
        ok, out = decode96(hc, rec)
        assert not ok and out == POISON * 144, rec.hex()                                      # refused, and `out` left alone
    assert decode96(hc, ID96) == (True, proj(None))
    # y bytes carry no flags: a set top bit there is just y >= p
    assert not decode96(hc, good[:48] + bytes([good[48] | 0x80]) + good[49:])[0]
    # canonical but off the curve: decode96 takes it, the curve check refuses it
    off = (pt[0], (pt[1] + 1) % P)
    assert decode96(hc, M.enc96(off)) == (True, proj(off))
    assert not hc.hc_on_curve(affine(off)) and hc.hc_on_curve(affine(pt))
    # where decode96 meets the (0, 0)-as-identity convention of device buffers: zero coordinates WITHOUT the infinity flag decode as
    # the non-identity (0 : 0 : 1), and the curve check refuses them (0 != 4), as the reference's is_on_curve does with infinity = false.
    # Only the flagged record is the identity (z = 0), and the equation alone says nothing of it: (0, 0) is not on the curve.
    assert decode96(hc, bytes(96)) == (True, fp_mont(0) + fp_mont(0) + fp_mont(1))
    assert not hc.hc_on_curve(affine(None)) and not hc.hc_on_curve(bytes(96))
    assert decode96(hc, ID96)[1][96:] == fp_mont(0)
    assert not hc.hc_on_curve(affine((0, 0))[:48] + fp_mont(1))                               # (0, 1): x = 0 alone is not the identity
    # on the curve, outside the subgroup: passes (the subgroup test is g1_is_torsion_free's)
    for _ in range(4):
        q = random_curve_point(rnd)
        assert ec_mul_unreduced(Q, q) is not None
        assert decode96(hc, M.enc96(q)) == (True, proj(q)) and hc.hc_on_curve(affine(q))


def fr_from_bytes(hc, b, fmt):
    out = C.create_string_buffer(32)
    return bool(hc.hc_fr_from_bytes(out, b, fmt)), out.raw


def fr_to_bytes(hc, mont, fmt):
    out = C.create_string_buffer(32)
    hc.hc_fr_to_bytes(out, mont, fmt)
    return out.raw


def test_fr_bytes_both_formats(hc):
    """Scalar::from_bytes / to_bytes (scalar.rs:264-304): canonical little-endian values only; Montgomery limbs pass untouched"""
    rnd = random.Random(86)
    for v in (0, 1, Q - 1):
        b = v.to_bytes(32, "little")
        assert hc.hc_fr_is_canonical(b)
        assert fr_from_bytes(hc, b, FR_BYTES_LE) == (True, fr_mont(v)), v
    for v in (Q, Q + 1, (1 << 256) - 1):
        b = v.to_bytes(32, "little")
        assert not hc.hc_fr_is_canonical(b)
        assert fr_from_bytes(hc, b, FR_BYTES_LE) == (False, POISON * 32), v                   # refused, and `out` left alone
        assert fr_from_bytes(hc, b, FR_MONT) == (True, b), v                                  # any 32 bytes pass through
        assert fr_to_bytes(hc, b, FR_MONT) == b, v
    for _ in range(64):
        v = rnd.randrange(Q)
        le, mont = v.to_bytes(32, "little"), fr_mont(v)
        assert fr_from_bytes(hc, le, FR_BYTES_LE) == (True, mont)
        assert fr_to_bytes(hc, mont, FR_BYTES_LE) == le
        assert fr_from_bytes(hc, mont, FR_MONT) == (True, mont) and fr_to_bytes(hc, mont, FR_MONT) == mont


def test_fr_from_u64_and_pow(hc):
    rnd = random.Random(87)
    out = C.create_string_buffer(32)
    for v in (0, 1, 2, 7, (1 << 32) - 1, 1 << 32, (1 << 64) - 1):
        hc.hc_fr_from_u64(out, v)
        assert out.raw == fr_mont(v), v
    for a, e in [(0, 0), (0, 5), (1, (1 << 64) - 1), (7, 0), (7, 1), (Q - 1, 3), (Q - 1, (1 << 64) - 2)] + \
                [(rnd.randrange(Q), rnd.randrange(1 << 64)) for _ in range(12)] + [(rnd.randrange(Q), 1 << s) for s in (31, 32, 63)]:
        hc.hc_fr_pow_u64(out, fr_mont(a), e)
        assert fr_unmont(out.raw) == pow(a, e, Q), (a, e)


def test_host_root_of_unity(hc):
    """utils.rs:39-43: ROOT_OF_UNITY^(2^32 / order) with the integer division as written; order 0 (a division by zero in the
    reference) is refused and writes nothing"""
    out = C.create_string_buffer(32)
    for order in (1, 2, 3, 1 << 10, 1 << 28, 1 << 32, (1 << 32) + 1, 1 << 40, (1 << 64) - 1):
        assert hc.hc_root_of_unity(out, order) == 1
        want = pow(M.ROOT_OF_UNITY, (1 << 32) // order, Q)
        assert fr_unmont(out.raw) == want, order
        if order > 1 << 32:
            assert want == 1
    assert pow(M.ROOT_OF_UNITY, 1 << 32, Q) == 1 and pow(M.ROOT_OF_UNITY, 1 << 31, Q) == Q - 1      # the constant has order 2^32
    assert hc.hc_root_of_unity(out, 0) == 0 and out.raw == POISON * 32

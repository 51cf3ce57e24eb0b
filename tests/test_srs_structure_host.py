"""CPU checks of the host pieces of the SRS structure calls: the prefix search of bp_srs_check_powers / bp_srs_adopt_lagrange
(csrc/srs_check_host.hpp), the G2 multiplication behind bp_g2_mul (csrc/pairing_host.hpp), and the new names of the C ABI; no GPU:
the headers are compiled for the host alone (tests/cpp/srs_check_host_host.hip)."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

from tests import bigint_model as M

Q = M.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_MAX = (1 << 64) - 1
NEW_NAMES = ["bp_srs_powers_reduce", "bp_srs_check_powers", "bp_srs_check_last_stats", "bp_srs_adopt_lagrange", "bp_srs_scale", "bp_g2_mul"]
BAD_POINT, BAD_SCALAR = -3, -4


@pytest.fixture(scope="module")
def sc(tmp_path_factory):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    so = str(tmp_path_factory.mktemp("srs_check_host") / "libsrscheckhost.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O1", "-fPIC", "-shared",
                           os.path.join(ROOT, "tests", "cpp", "srs_check_host_host.hip"), "-o", so])
    lib = C.CDLL(so)
    buf = C.c_char_p
    for name, res, args in (("sc_lowest_failing_prefix", C.c_uint64, [C.c_uint64, buf, C.POINTER(C.c_uint32)]), ("sc_ceil_log2", C.c_uint32, [C.c_uint64]),
                            ("sc_g2_mul", C.c_int, [buf, buf, buf]), ("sc_g2_mul_generator", C.c_int, [buf, buf])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def search(sc, n, bad_positions):
    flags = bytearray(max(n, 1))
    for p in bad_positions:
        flags[p] = 1
    calls = C.c_uint32(99)
    return sc.sc_lowest_failing_prefix(n, bytes(flags), C.byref(calls)), calls.value


def ceil_log2(n):
    return (n - 1).bit_length() if n > 1 else 0


def test_ceil_log2(sc):
    for n in list(range(0, 70)) + [2**20 - 1, 2**20, 2**20 + 1, 2**24 + 1]:
        assert sc.sc_ceil_log2(n) == ceil_log2(n), n


def test_lowest_failing_prefix_finds_the_lowest_break_within_its_bound(sc):
    """every n in 0 .. 70, every position of one break and every pair of positions of two: the answer is the length of the shortest
    failing prefix, lowest break + 1, after at most 1 + ceil(log2 n) questions; a clean input costs one question (none for n = 0)"""
    for n in range(0, 71):
        bound = 1 + ceil_log2(n)
        assert search(sc, n, []) == (SIZE_MAX, 1 if n else 0)
        for p in range(n):
            got, calls = search(sc, n, [p])
            assert got == p + 1 and 1 <= calls <= bound, (n, p, got, calls)
            for p2 in range(p + 1, n):
                got, calls = search(sc, n, [p, p2])
                assert got == p + 1 and 1 <= calls <= bound, (n, p, p2, got, calls)


def le32(v):
    return int(v).to_bytes(32, "little")


def g2_gen(sc, k):
    out = C.create_string_buffer(192)
    assert sc.sc_g2_mul_generator(le32(k), out) == 0
    return out.raw


def g2_mul(sc, q192, k, expect=0):
    out = C.create_string_buffer(b"\xaa" * 192, 192)
    assert sc.sc_g2_mul(q192, le32(k), out) == expect
    return out.raw


ID192 = bytes([0x40]) + bytes(191)


def test_g2_mul_is_the_group_action(sc):
    rnd = random.Random(0x62)
    values = [1, 2, Q - 1, rnd.randrange(Q)]
    gens = {a: g2_gen(sc, a) for a in values}
    for a in values:
        for b in values:
            assert g2_mul(sc, gens[a], b) == g2_gen(sc, a * b % Q), (a, b)
    assert g2_mul(sc, gens[1], 1) == gens[1] and gens[1] != gens[2]


def test_g2_mul_identities_and_refusals(sc):
    g = g2_gen(sc, 7)
    assert g2_mul(sc, g, 0) == ID192                                      # k = 0
    assert g2_mul(sc, ID192, 12345) == ID192                              # the identity stays the identity
    assert g2_gen(sc, 0) == ID192
    untouched = b"\xaa" * 192
    assert g2_mul(sc, g, Q, BAD_SCALAR) == untouched                      # k >= q
    assert g2_mul(sc, g, 2**256 - 1, BAD_SCALAR) == untouched
    off = bytearray(g)
    off[191] ^= 1                                                         # y.c0 changed: not on the curve
    assert g2_mul(sc, bytes(off), 3, BAD_POINT) == untouched
    for flag in (0x80, 0x20, 0x40):                                       # compression / sort flag; infinity flag over non-zero coordinates
        bad = bytearray(g)
        bad[0] |= flag
        assert g2_mul(sc, bytes(bad), 3, BAD_POINT) == untouched
    big = bytearray(g)
    big[0:48] = (M.P).to_bytes(48, "big")                                 # x.c1 = p: not canonical
    assert g2_mul(sc, bytes(big), 3, BAD_POINT) == untouched


def test_the_abi_holds_the_new_names():
    """the header, the Rust bindings and the library's dynamic symbol table all hold the entry points of the SRS structure calls"""
    import baby_plonk_rust_amd as bp
    from baby_plonk_rust_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bp_msm_ntt.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "include", "bp_msm_ntt.rs")).read()
    listing = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in listing.splitlines() if line.strip()}
    lib = bp.load()
    for name in NEW_NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert re.search(r"\bfn %s\s*\(" % name, rust), name
        assert name in exported and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert "#define BP_SRS_CHECK_GENERATOR 2u" in header


def test_bp_g2_mul_through_the_library(sc):
    """the exported bp_g2_mul is the host code checked above: same bytes, same codes, and the Python mirror raises them"""
    import baby_plonk_rust_amd as bp
    a, b = 0x1234567, random.Random(5).randrange(Q)
    assert bp.g2_mul(bp.g2_mul_generator(a), b) == g2_gen(sc, a * b % Q) == bp.g2_mul_generator(a * b % Q)
    assert bp.g2_mul(bp.g2_mul_generator(a), 0) == ID192
    with pytest.raises(bp.BpError) as e:
        bp.g2_mul(bp.g2_mul_generator(a), Q)
    assert e.value.code == BAD_SCALAR
    off = bytearray(bp.g2_mul_generator(a))
    off[191] ^= 1
    with pytest.raises(bp.BpError) as e:
        bp.g2_mul(bytes(off), 3)
    assert e.value.code == BAD_POINT

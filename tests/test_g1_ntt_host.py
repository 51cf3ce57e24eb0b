"""CPU checks of csrc/g1_ntt.hpp, the inverse transform over G1 behind bp_srs_lagrange: its schedule (which butterfly of which pass
touches which two points with which power of omega), its scalar multiplication, and the host loop over its butterfly -- the lines the
kernel g1_ntt_pass runs, compiled for the host alone (tests/cpp/g1_ntt_host.hip); no GPU.
Expected points come from the literal double sum L_i = sum_j M_ij P_j with M read off O.i_ntt_381 of the unit vectors and the sum built
from O.g1_mul / O.g1_add; expected exponents from the decimation-in-time identity restated below; none from the header under test."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import bigint_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = M.Q
U64x3 = C.c_uint64 * 3


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    so = str(tmp_path_factory.mktemp("g1_ntt") / "libg1ntt.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O2", "-fPIC", "-shared",
                           os.path.join(ROOT, "tests", "cpp", "g1_ntt_host.hip"), "-o", so])
    lib = C.CDLL(so)
    u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
    for name, res, args in (("gn_step", None, [u32, u32, u64, C.POINTER(C.c_uint64)]), ("gn_bitrev", u64, [u64, u32]), ("gn_max_log", u32, []),
                            ("gn_mul", C.c_int, [vp, vp, vp]), ("gn_transform", C.c_int, [vp, u32, vp])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def step(lib, log_n, s, b):
    out = U64x3()
    lib.gn_step(log_n, s, b, out)
    return tuple(out)


# ---- the schedule --------------------------------------------------------------------------------------------------------------------
def demanded_exponent(log_n, s, i0):
    """Decimation in time of x_i = n^-1 sum_j omega^(-ij) X_j over bit-reversed input: after pass s every block of 2^(s+1) slots holds
    the inverse DFT of its inputs, and the butterfly on slots i0, i0 + 2^s of a block (bit s of i0 clear) multiplies the upper one by
    omega_(2^(s+1))^-(i0 mod 2^s) = omega_n^(-(i0 mod 2^s) n / 2^(s+1)): the exponent of omega_n, taken mod n."""
    n = 1 << log_n
    return (-(i0 & ((1 << s) - 1)) * (n >> (s + 1))) % n


def check_step(lib, log_n, s, b):
    i0, i1, e = step(lib, log_n, s, b)
    assert i1 == i0 + (1 << s) and not (i0 >> s) & 1 and i1 < (1 << log_n), (log_n, s, b)
    assert e == demanded_exponent(log_n, s, i0), (log_n, s, b)
    return i0


def test_limits(lib):
    assert lib.gn_max_log() == 24


@pytest.mark.parametrize("log_n", range(1, 11))
def test_schedule_exhaustive(lib, log_n):
    """every butterfly of every pass: the demanded exponent, and the n / 2 butterflies of a pass cover every slot exactly once"""
    half = 1 << (log_n - 1)
    for s in range(log_n):
        lows = [check_step(lib, log_n, s, b) for b in range(half)]
        assert sorted(lows + [i + (1 << s) for i in lows]) == list(range(1 << log_n))


@pytest.mark.parametrize("log_n", range(11, 25))
def test_schedule_sampled(lib, log_n):
    rnd = random.Random(log_n)
    half = 1 << (log_n - 1)
    for s in range(log_n):
        seen = {check_step(lib, log_n, s, b) for b in [0, 1, half - 2, half - 1] + [rnd.randrange(half) for _ in range(60)]}
        assert len(seen) >= 60                                   # distinct butterflies, distinct slots


@pytest.mark.parametrize("log_n", range(1, 7))
def test_schedule_computes_i_ntt_in_the_field(lib, log_n):
    """the same schedule run over Fr with Python integers (bit-reversed input, n^-1 on the inputs, (u, v) -> (u + w v, u - w v)) is
    O.i_ntt_381: the demanded exponents above are the right demand, and the bit reversal is the right reordering"""
    n = 1 << log_n
    x = [random.Random(7 * log_n + i).randrange(Q) for i in range(n)]
    w, n_inv = M.omega(n), pow(n, Q - 2, Q)
    buf = [x[lib.gn_bitrev(i, log_n)] * n_inv % Q for i in range(n)]
    assert sorted(lib.gn_bitrev(i, log_n) for i in range(n)) == list(range(n))
    assert all(lib.gn_bitrev(i, log_n) == int(format(i, "0%db" % log_n)[::-1], 2) for i in range(n))
    for s in range(log_n):
        nxt = list(buf)
        for b in range(n // 2):
            i0, i1, e = step(lib, log_n, s, b)
            t = buf[i1] * pow(w, e, Q) % Q
            nxt[i0], nxt[i1] = (buf[i0] + t) % Q, (buf[i0] - t) % Q
        buf = nxt
    assert buf == O.fr_array_to_ints(O.i_ntt_381(O.fr_array_from_ints(x)))


# ---- the scalar multiplication ---------------------------------------------------------------------------------------------------------
def test_scalar_multiplication(lib):
    rnd = random.Random(11)
    base = M.enc96(M.ec_mul(5))
    for k in [0, 1, 2, 3, Q - 1, Q - 2, 1 << 254, (1 << 254) - 1, 0x55555555 << 200] + [rnd.randrange(Q) for _ in range(4)]:
        k %= Q
        out = np.zeros(96, dtype=np.uint8)
        src, kb = np.frombuffer(base, dtype=np.uint8).copy(), np.frombuffer(k.to_bytes(32, "little"), dtype=np.uint8).copy()
        assert lib.gn_mul(src.ctypes.data, kb.ctypes.data, out.ctypes.data) == 0
        assert bytes(out) == M.enc96(M.ec_mul(5 * k % Q) if 5 * k % Q else None), k
    ident = np.frombuffer(M.enc96(None), dtype=np.uint8).copy()
    kb = np.frombuffer((Q - 1).to_bytes(32, "little"), dtype=np.uint8).copy()
    out = np.zeros(96, dtype=np.uint8)
    assert lib.gn_mul(ident.ctypes.data, kb.ctypes.data, out.ctypes.data) == 0 and bytes(out) == M.enc96(None)


# ---- the transform -------------------------------------------------------------------------------------------------------------------
_MATRIX = {}


def matrix(n):
    """M_ij of i_ntt_381 at size n, read off the oracle's transform of the unit vectors (computed once per size)"""
    if n not in _MATRIX:
        cols = [O.i_ntt_381(O.fr_array_from_ints([int(j == k) for k in range(n)])) for j in range(n)]
        _MATRIX[n] = [[cols[j][i] for j in range(n)] for i in range(n)]
    return _MATRIX[n]


def double_sum(points):
    """L_i = sum_j M_ij P_j, literally, as 96-byte records"""
    n, m = len(points), matrix(len(points))
    out = []
    for i in range(n):
        acc = O.g1_identity()
        for j in range(n):
            acc = O.g1_add(acc, O.g1_mul(points[j], m[i][j]))
        out.append(O.g1_bytes96(acc))
    return b"".join(out)


def transform(lib, points):
    n = len(points)
    src = np.frombuffer(b"".join(O.g1_bytes96(p) for p in points), dtype=np.uint8).copy()
    out = np.zeros(96 * n, dtype=np.uint8)
    assert lib.gn_transform(src.ctypes.data, n.bit_length() - 1, out.ctypes.data) == 0
    return bytes(out)


def mult(k):
    return O.g1_mul(O.g1_generator(), O.fr_from_int(k % Q))


SIZES = (1, 2, 4, 8, 16)


@pytest.mark.parametrize("n", SIZES)
def test_random_multiples(lib, n):
    rnd = random.Random(n)
    ks = [rnd.randrange(1, Q) for _ in range(n)]
    pts = [mult(k) for k in ks]
    got = transform(lib, pts)
    assert got == double_sum(pts)
    coeffs = O.fr_array_to_ints(O.i_ntt_381(O.fr_array_from_ints(ks)))           # the first statement of the definition: L_i = (i_ntt(k))_i G
    assert got == b"".join(M.enc96(M.ec_mul(c) if c else None) for c in coeffs)


@pytest.mark.parametrize("n", SIZES)
def test_all_points_equal(lib, n):
    """pass 0 adds every point to itself (u == w v: the addition formula must double) and subtracts it from itself (the identity comes
    out of u - w v); from pass 1 on every butterfly has the identity as one or both operands.  L = [P, O, O, ...]"""
    pts = [mult(0xABCDEF)] * n
    got = transform(lib, pts)
    assert got == double_sum(pts) == O.g1_bytes96(pts[0]) + M.enc96(None) * (n - 1)


@pytest.mark.parametrize("n", SIZES)
def test_identity_inputs(lib, n):
    """[G, O, O, ...]: the identity is scaled by n^-1 in pass 0 and multiplied by every twiddle after it; L_i = n^-1 G for every i"""
    pts = [O.g1_generator()] + [O.g1_identity()] * (n - 1)
    got = transform(lib, pts)
    assert got == double_sum(pts) == M.enc96(M.ec_mul(pow(n, Q - 2, Q))) * n


@pytest.mark.parametrize("n", (4, 8, 16))
def test_one_hot_output(lib, n):
    """P_j = omega^(3j) G: L_3 = G and every other L_i is the identity -- the last pass's butterflies meet u == -w v (and u == w v at
    slot 3), the passes before it cancel block by block"""
    w = M.omega(n)
    pts = [mult(pow(w, 3 * j, Q)) for j in range(n)]
    got = transform(lib, pts)
    assert got == double_sum(pts) == b"".join(M.enc96(M.ec_mul(1) if i == 3 else None) for i in range(n))

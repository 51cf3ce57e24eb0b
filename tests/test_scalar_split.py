"""CPU checks of csrc/scalar_split.hpp, the lines that write a scalar as k = k1 x^2 + k0 for the endomorphism form of the
variable-base multiplication (verify_segments_kernels.hpp); no GPU: the header is compiled for the host alone
(tests/cpp/scalar_split_host.hip).  Expectations are Python integers; the endomorphism itself -- (beta x, -y) = [x^2] P with the
beta of g1_check.hpp -- is checked on the fixture's points with tests/bigint_model.py."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

from tests import bigint_model as M
from tests import verify_model as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q, P = M.Q, M.P
BLS_X = 0xD201000000010000                                    # |x|; q = x^4 - x^2 + 1
X2 = BLS_X * BLS_X


@pytest.fixture(scope="module")
def ss(tmp_path_factory):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    so = str(tmp_path_factory.mktemp("scalar_split") / "libscalarsplit.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O1", "-fPIC", "-shared",
                           os.path.join(ROOT, "tests", "cpp", "scalar_split_host.hip"), "-o", so])
    lib = C.CDLL(so)
    lib.ss_split.restype, lib.ss_split.argtypes = None, [C.c_void_p, C.c_size_t, C.c_void_p]
    lib.ss_x2.restype, lib.ss_x2.argtypes = None, [C.c_void_p]
    lib.ss_bits.restype, lib.ss_bits.argtypes = C.c_int, []
    return lib


def split(lib, scalars):
    buf = np.frombuffer(b"".join(k.to_bytes(32, "little") for k in scalars), dtype=np.uint32).copy()
    out = np.zeros(8 * len(scalars), dtype=np.uint32)
    lib.ss_split(buf.ctypes.data, len(scalars), out.ctypes.data)
    raw = out.tobytes()
    return [(int.from_bytes(raw[32 * i: 32 * i + 16], "little"), int.from_bytes(raw[32 * i + 16: 32 * i + 32], "little")) for i in range(len(scalars))]


def edge_scalars():
    edges = [0, 1, X2 - 1, X2, X2 + 1, Q - 1, 2**255 - 1]      # 2^255 - 1: not canonical, still inside what the lines accept
    for bits in (32, 64, 96, 128, 160, 192, 224):               # every multiple of x^2 next to a limb boundary, and its neighbours
        for t in (((1 << bits) // X2) * X2, ((1 << bits) // X2 + 1) * X2):
            edges += [v for v in (t - 1, t, t + 1) if 0 <= v < 2**255]
        edges += [(1 << bits) - 1, 1 << bits]
    for bits in (32, 64, 96):                                   # quotients next to a limb boundary of k1
        edges += [((1 << bits) - 1) * X2 + X2 - 1, (1 << bits) * X2, (1 << bits) * X2 - 1]
    edges += [((2**255 - 1) // X2) * X2, ((Q - 1) // X2) * X2 - 1]
    return sorted(set(edges))


def test_the_constant_is_x_squared_and_q_is_built_from_it(ss):
    out = np.zeros(4, dtype=np.uint32)
    ss.ss_x2(out.ctypes.data)
    assert int.from_bytes(out.tobytes(), "little") == X2
    assert Q == X2 * X2 - X2 + 1 and X2.bit_length() == 128 and ss.ss_bits() == 128


def test_split_is_exact_and_both_halves_fit_the_loop_count(ss):
    rnd = random.Random(0x5C41A4)
    scalars = edge_scalars() + [rnd.randrange(Q) for _ in range(10000)] + [rnd.getrandbits(255) for _ in range(200)]
    bits = ss.ss_bits()
    for k, (k0, k1) in zip(scalars, split(ss, scalars)):
        assert k0 + k1 * X2 == k, hex(k)
        assert k0 < X2 and k0 < (1 << bits) and k1 < (1 << bits), hex(k)
        assert (k0, k1) == (k % X2, k // X2)


def header_beta():
    text = open(os.path.join(ROOT, "baby_plonk_rust_amd", "csrc", "g1_check.hpp")).read()
    limbs = re.search(r"BP_TABLE\(fp_beta_canonical,([^)]*)\)", text).group(1)
    return sum(int(w.strip().rstrip("u"), 16) << (32 * i) for i, w in enumerate(limbs.split(",")))


def test_the_endomorphism_of_the_header_is_x_squared_on_the_fixture():
    """(beta x, -y) = [x^2] P: beta from Python's own arithmetic, the header's constant equal to it, lambda = x^2 a root of
    l^2 + l + 1 up to sign conventions (-x^2 is the eigenvalue of phi)"""
    beta = header_beta()
    assert beta not in (0, 1) and pow(beta, 3, P) == 1
    own = pow(2, (P - 1) // 3, P)                               # 2 is not a cube: a primitive cube root of unity
    assert own != 1 and beta in (own, own * own % P)
    lam = (-X2) % Q
    assert (lam * lam + lam + 1) % Q == 0                       # phi^2 + phi + 1 = 0
    fx = V.fixture_points()
    for i in (1, 2, 3, 7, 500, 999):
        x, y = M.dec48(fx[i])
        assert (beta * x % P, (-y) % P) == M.ec_mul(X2 % Q, (x, y)), i
    rnd = random.Random(3)
    for _ in range(3):                                          # and the identity the kernel relies on: k P = k0 P + k1 (beta x, -y)
        k = rnd.randrange(Q)
        x, y = M.dec48(fx[rnd.randrange(1, 1000)])
        assert M.ec_add(M.ec_mul(k % X2, (x, y)), M.ec_mul(k // X2, (beta * x % P, (-y) % P))) == M.ec_mul(k, (x, y))

"""CPU checks of csrc/kzg_host.hpp, the host arithmetic of the KZG calls: is the opening point on the domain (and where), the
barycentric scale, and the scalars of bp_kzg_verify_reduce; no GPU: the header is compiled for the host alone
(tests/cpp/kzg_host_host.hip).  Every expectation comes from tests/kzg_model.py."""
import ctypes as C
import os
import random
import subprocess

import pytest

from tests import bigint_model as M
from tests import kzg_model as K

Q = M.Q
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kh(tmp_path_factory):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    so = str(tmp_path_factory.mktemp("kzg_host") / "libkzghost.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O1", "-fPIC", "-shared",
                           os.path.join(ROOT, "tests", "cpp", "kzg_host_host.hip"), "-o", so])
    lib = C.CDLL(so)
    buf = C.c_char_p
    for name, res, args in (("kh_domain_index", C.c_longlong, [buf, C.c_uint32]), ("kh_barycentric_scale", None, [buf, C.c_uint32, buf]),
                            ("kh_reduce_scalars", None, [C.c_size_t, C.c_size_t, buf, buf, buf, buf, buf])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def enc(values):
    assert all(0 <= v < Q for v in values)
    return b"".join(v.to_bytes(32, "little") for v in values)


def dec(raw):
    return [int.from_bytes(raw[i: i + 32], "little") for i in range(0, len(raw), 32)]


@pytest.mark.parametrize("k", [0, 1, 3, 10, 24, 28])
def test_domain_index_and_scale(kh, k):
    n, rng = 1 << k, random.Random(k)
    w = M.omega(n)
    inside = sorted({0, 1 % n, n // 2, n - 1, rng.randrange(n), rng.randrange(n)})
    for m in inside:
        assert kh.kh_domain_index(enc([pow(w, m, Q)]), k) == m
    for z in (0, rng.randrange(Q), M.omega(2 * n), 7):                    # w_2n: z^n = -1
        assert kh.kh_domain_index(enc([z]), k) == -1
        out = C.create_string_buffer(32)
        kh.kh_barycentric_scale(enc([z]), k, out)
        assert dec(out.raw) == [(pow(z, n, Q) - 1) * pow(n, -1, Q) % Q]


REDUCE_CASES = [(m, count, special) for m in (1, 2, 5) for count in (1, 3) for special in ("random", "nu = 0", "z = 0", "no weights", "no nu")
                if special != "no nu" or count == 1]                      # nu may be absent for one polynomial only


@pytest.mark.parametrize("m, count, special", REDUCE_CASES)
def test_reduce_scalars(kh, m, count, special):
    rng = random.Random(31 * m + count)
    claims = [(rng.randrange(Q), [rng.randrange(Q) for _ in range(count)], rng.randrange(Q), rng.randrange(Q)) for _ in range(m)]
    if special == "nu = 0":
        claims[-1] = claims[-1][:2] + (0,) + claims[-1][3:]
    if special == "z = 0":
        claims[0] = (0,) + claims[0][1:]
    if special == "no weights":
        claims = [c[:3] + (1,) for c in claims]
    if special == "no nu":
        claims = [c[:2] + (1,) + c[3:] for c in claims]                   # count = 1: nu^0 only
    out = C.create_string_buffer(32 * (m * count + 2 * m + 1))
    kh.kh_reduce_scalars(m, count, enc([c[0] for c in claims]), enc([y for c in claims for y in c[1]]),
                         None if special == "no nu" else enc([c[2] for c in claims]),
                         None if special == "no weights" else enc([c[3] for c in claims]), out)
    got = dec(out.raw)
    c, w, g, a = K.reduce_scalars(claims)
    assert got == [x for row in c for x in row] + w + a + [g]

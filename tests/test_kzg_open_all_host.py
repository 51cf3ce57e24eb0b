"""CPU checks of csrc/kzg_open_all.hpp, the map behind bp_kzg_open_all (all n proofs of a polynomial on its domain): the index
functions of S^, c^ and the forward-by-reversal rule, and the host loop over pass 0 of the three transforms, the butterfly and the
scalar multiplication of csrc/g1_ntt.hpp -- the lines the kernels run, compiled for the host alone (tests/cpp/kzg_open_all_host.hip);
no GPU.  Expected indices come from the definitions restated below, expected proofs from [horner(quotient_coeffs(f, w^i), tau)] G of
tests/kzg_model.py over the oracle's G1 (no division by tau - w^i, so tau on the domain is covered); none from the header under test."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from tests import bigint_model as M
from tests import kzg_model as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = M.Q


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    so = str(tmp_path_factory.mktemp("kzg_open_all") / "libkzgopenall.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O2", "-fPIC", "-shared",
                           os.path.join(ROOT, "tests", "cpp", "kzg_open_all_host.hip"), "-o", so])
    lib = C.CDLL(so)
    u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
    for name, res, args in (("oa_shat", u64, [u32, u64]), ("oa_chat", u64, [u32, u64]), ("oa_reversed", u64, [u32, u64]),
                            ("oa_forward_source", u64, [u32, u64]), ("oa_none", u64, []), ("oa_proofs", C.c_int, [vp, vp, u64, u32, vp])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


# ---- the index maps ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", range(1, 7))
def test_index_functions_are_the_definitions(lib, log_n):
    """S^_j = P_{n-2-j} for j <= n - 2, the identity for n - 1 <= j < N; c^_t = f_{(t+n-1) mod N} where that index is < n, else 0;
    the reversed sequence has x_{(len - j) mod len} at place j -- for every index"""
    n, none = 1 << log_n, lib.oa_none()
    N = 2 * n
    for j in range(N):
        assert lib.oa_shat(log_n, j) == (n - 2 - j if j <= n - 2 else none), j
        k = (j + n - 1) % N
        assert lib.oa_chat(log_n, j) == (k if k < n else none), j
        assert lib.oa_reversed(log_n + 1, j) == (N - j) % N
        rev = int(format(j, "0%db" % (log_n + 1))[::-1], 2)
        assert lib.oa_forward_source(log_n + 1, j) == (N - rev) % N
    for j in range(n):
        assert lib.oa_reversed(log_n, j) == (n - j) % n
    assert sorted(lib.oa_forward_source(log_n, s) for s in range(n)) == list(range(n))


@pytest.mark.parametrize("log_n", range(1, 5))
def test_map_in_integers(lib, log_n):
    """the map of the header over Python integers in place of points (P_k = tau^k): the cyclic convolution of S^ and c^ through the
    index functions gives h_m = sum_k f_{m+1+k} tau^k for m < n (h_{n-1} = 0, entries n.. not zero in general), and the DFT of h the
    quotient values (f(tau) - f(w^i)) / (tau - w^i)"""
    n, none = 1 << log_n, lib.oa_none()
    N, rnd = 2 * n, random.Random(log_n)
    tau, f = rnd.randrange(2, Q), [rnd.randrange(Q) for _ in range(n)]
    s = [0 if lib.oa_shat(log_n, j) == none else pow(tau, lib.oa_shat(log_n, j), Q) for j in range(N)]
    c = [0 if lib.oa_chat(log_n, t) == none else f[lib.oa_chat(log_n, t)] for t in range(N)]
    conv = [sum(s[j] * c[(m - j) % N] for j in range(N)) % Q for m in range(N)]
    h = [sum(f[m + 1 + k] * pow(tau, k, Q) for k in range(n - 1 - m)) % Q for m in range(n)]
    assert conv[:n] == h and h[n - 1] == 0
    w = M.omega(n)
    for i in range(n):
        z = pow(w, i, Q)
        assert sum(pow(z, m, Q) * h[m] for m in range(n)) % Q == K.proof_scalar(K.horner(f, tau), K.horner(f, z), tau, z)


# ---- the host loop over the real butterfly and multiplication ---------------------------------------------------------------------------
def proofs(lib, tau, f, n):
    log_n = n.bit_length() - 1
    srs = np.frombuffer(b"".join(K.point96(pow(tau, k, Q)) for k in range(n - 1)) + bytes(96), dtype=np.uint8).copy()
    co = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in f) + bytes(32), dtype=np.uint8).copy()
    out = np.zeros(96 * n, dtype=np.uint8)
    assert lib.oa_proofs(srs.ctypes.data, co.ctypes.data, len(f), log_n, out.ctypes.data) == 0
    return bytes(out)


def expected(tau, f, n):
    w = M.omega(n)
    f = list(f) + [0] * (n - len(f))
    return b"".join(K.point96(K.horner(K.quotient_coeffs(f, pow(w, i, Q)), tau)) for i in range(n))


def polynomials(n, rnd):
    return {"random": [rnd.randrange(Q) for _ in range(n)], "zero": [0] * n, "constant": [rnd.randrange(1, Q)],
            "top": [0] * (n - 1) + [1], "shorter": [rnd.randrange(Q) for _ in range(n - 1)]}


@pytest.mark.parametrize("n", (2, 4, 8))
@pytest.mark.parametrize("kind", ("random", "zero", "constant", "top", "shorter"))
def test_host_loop_against_the_closed_form(lib, n, kind):
    rnd = random.Random(100 * n + len(kind))
    tau, f = rnd.randrange(2, Q), polynomials(n, rnd)[kind]
    got = proofs(lib, tau, f, n)
    assert got == expected(tau, f, n)
    if kind in ("zero", "constant"):
        assert got == M.enc96(None) * n                          # the quotient of a constant is zero: every proof is the identity record


@pytest.mark.parametrize("n", (4, 8))
@pytest.mark.parametrize("tau_kind", ("one", "on_domain"))
def test_host_loop_degenerate_points(lib, n, tau_kind):
    """tau = 1: every point is G, so additions meet doublings and cancellations; tau = w_n: tau on the domain (the closed form here
    divides by nothing)"""
    rnd = random.Random(n)
    tau = 1 if tau_kind == "one" else M.omega(n)
    f = [rnd.randrange(Q) for _ in range(n)]
    assert proofs(lib, tau, f, n) == expected(tau, f, n)

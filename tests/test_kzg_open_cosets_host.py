"""CPU checks of csrc/kzg_open_cosets.hpp, the map behind bp_kzg_open_cosets (the n / l cell proofs of a polynomial): the index
functions of S^(j), c^(j) and the cell layout, and the host loops over the per-lane bodies of the table, multiplication, halving and
butterfly passes -- the lines the kernels run, compiled for the host alone (tests/cpp/kzg_open_cosets_host.hip); no GPU.  Expected
indices come from the definitions restated below, expected proofs from [q_k(tau)] G with q_k = f div (x^l - a_k) by the schoolbook
recurrence of tests/kzg_cells_model.py over the oracle's G1; none from the header under test."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from tests import bigint_model as M
from tests import kzg_cells_model as CM
from tests import kzg_model as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = M.Q
PAIRS = [(log_n, log_l) for log_n in range(1, 7) for log_l in range(log_n)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    so = str(tmp_path_factory.mktemp("kzg_open_cosets") / "libkzgopencosets.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O2", "-fPIC", "-shared",
                           os.path.join(ROOT, "tests", "cpp", "kzg_open_cosets_host.hip"), "-o", so])
    lib = C.CDLL(so)
    u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
    for name, res, args in (("oc_shat", u64, [u32, u32, u64, u64]), ("oc_chat", u64, [u32, u32, u64, u64]), ("oc_value_source", u64, [u32, u32, u64]),
                            ("oc_all_shat", u64, [u32, u64]), ("oc_all_chat", u64, [u32, u64]), ("oc_none", u64, []),
                            ("oc_proofs", C.c_int, [vp, vp, u64, u32, u32, vp])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


# ---- the index maps ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", range(1, 7))
def test_index_functions_are_the_definitions(lib, log_n):
    """S^(j)_i = P_{(r-2-i) l + j} for i <= r - 2, the identity for r - 1 <= i < R; c^(j)_t = f_{((t+r-1) mod R) l + j} where that
    strided index is < r, else 0; place k l + j of the values is f(w^(k + r j)) -- for every index and every log_l <= log_n (log_l =
    log_n: r = 1, nothing is read); the highest SRS index read is n - l - 1; at log_l = 0 they are open_all_shat / open_all_chat"""
    n, none = 1 << log_n, lib.oc_none()
    for log_l in range(log_n + 1):
        l, r = 1 << log_l, n >> log_l
        R, read = 2 * r, []
        for j in range(l):
            for i in range(R):
                got = lib.oc_shat(log_n, log_l, j, i)
                assert got == ((r - 2 - i) * l + j if i <= r - 2 else none), (log_l, j, i)
                read += [got] if got != none else []
                k = (i + r - 1) % R
                assert lib.oc_chat(log_n, log_l, j, i) == (k * l + j if k < r else none), (log_l, j, i)
                if log_l == 0:
                    assert got == lib.oc_all_shat(log_n, i) and lib.oc_chat(log_n, 0, 0, i) == lib.oc_all_chat(log_n, i)
        assert sorted(read) == list(range(n - l)) and (not read or max(read) == n - l - 1)      # P_0 .. P_{n-l-1}, each once
        coeffs = [lib.oc_chat(log_n, log_l, j, t) for j in range(l) for t in range(R)]
        assert sorted(c for c in coeffs if c != none) == list(range(n))                        # every coefficient once
        src = [lib.oc_value_source(log_n, log_l, c) for c in range(n)]
        assert src == [k + r * j for k in range(r) for j in range(l)] and sorted(src) == list(range(n))


@pytest.mark.parametrize("log_n,log_l", [(1, 0), (1, 1), (2, 1), (3, 1), (3, 2), (4, 2), (4, 4), (5, 3)])
def test_map_in_integers(lib, log_n, log_l):
    """the map of the header over Python integers in place of points (P_k = tau^k): the l cyclic convolutions of S^(j) and c^(j)
    through the index functions, summed, give h_m = the double sum for m < r (h_{r-1} = 0), and the DFT of h with root w^l the
    quotient values q_k(tau)"""
    n, l, none = 1 << log_n, 1 << log_l, lib.oc_none()
    r, rnd = n >> log_l, random.Random(16 * log_n + log_l)
    R = 2 * r
    tau, f = rnd.randrange(2, Q), [rnd.randrange(Q) for _ in range(n)]
    conv = [0] * R
    for j in range(l):
        idx_s, idx_c = [lib.oc_shat(log_n, log_l, j, i) for i in range(R)], [lib.oc_chat(log_n, log_l, j, t) for t in range(R)]
        s = [0 if k == none else pow(tau, k, Q) for k in idx_s]
        c = [0 if k == none else f[k] for k in idx_c]
        for m in range(R):
            conv[m] = (conv[m] + sum(s[i] * c[(m - i) % R] for i in range(R))) % Q
    h = CM.h_double_sum(f, n, l, [pow(tau, k, Q) for k in range(n)])
    assert conv[:r] == h and h[r - 1] == 0
    assert CM.proofs_from_h(h, n, l) == [CM.proof_scalar(f, n, l, k, tau) for k in range(r)]
    for k in range(r):                                             # the division itself: f = q (x^l - a_k) + I, I the interpolant
        values, _ = CM.cell(f, n, l, k, tau)
        q, rem = CM.div_binomial(f, l, CM.cell_a(n, l, k))
        for z, v in zip(CM.cell_points(n, l, k), values):
            assert pow(z, l, Q) == CM.cell_a(n, l, k) and K.horner(rem, z) == v
        x = rnd.randrange(Q)
        assert (K.horner(q, x) * (pow(x, l, Q) - CM.cell_a(n, l, k)) + K.horner(rem, x)) % Q == K.horner(f, x)


# ---- the host loop over the real butterfly and multiplication ---------------------------------------------------------------------------
def proofs(lib, tau, f, log_n, log_l):
    n, l = 1 << log_n, 1 << log_l
    used = n - l if log_l else n - 1
    srs = np.frombuffer(b"".join(K.point96(pow(tau, k, Q)) for k in range(used)) + bytes(96), dtype=np.uint8).copy()
    co = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in f) + bytes(32), dtype=np.uint8).copy()
    out = np.zeros(96 * (n // l), dtype=np.uint8)
    assert lib.oc_proofs(srs.ctypes.data, co.ctypes.data, len(f), log_n, log_l, out.ctypes.data) == 0
    return bytes(out)


def expected(tau, f, log_n, log_l):
    n, l = 1 << log_n, 1 << log_l
    return b"".join(K.point96(CM.cell(f, n, l, k, tau)[1]) for k in range(n // l))


def polynomials(n, l, rnd):
    return {"random": [rnd.randrange(Q) for _ in range(n)], "zero": [0] * n, "constant": [rnd.randrange(1, Q)],
            "top": [0] * (n - 1) + [1], "short": [rnd.randrange(1, Q) for _ in range(l - 1)]}


@pytest.mark.parametrize("log_n,log_l", [(2, 1), (3, 1), (4, 2), (4, 3)])
@pytest.mark.parametrize("kind", ("random", "zero", "constant", "top", "short"))
def test_host_loop_against_the_closed_form(lib, log_n, log_l, kind):
    """(2,1): the smallest real convolution, r = 2, R = 4; (4,3): r = 2 with l = 8, the halving passes dominate"""
    n, l = 1 << log_n, 1 << log_l
    rnd = random.Random(100 * n + 10 * l + len(kind))
    tau, f = rnd.randrange(2, Q), polynomials(n, l, rnd)[kind]
    got = proofs(lib, tau, f, log_n, log_l)
    assert got == expected(tau, f, log_n, log_l)
    if kind in ("zero", "constant", "short"):
        assert got == M.enc96(None) * (n // l)                      # fewer than l + 1 coefficients: every quotient is zero


@pytest.mark.parametrize("log_n", (2, 3))
def test_host_loop_at_cell_size_one_is_open_all(lib, log_n):
    n, rnd = 1 << log_n, random.Random(log_n)
    tau, f = rnd.randrange(2, Q), [rnd.randrange(Q) for _ in range(n)]
    want = b"".join(K.point96(K.horner(K.quotient_coeffs(f, z), tau)) for z in K.domain(n))
    assert proofs(lib, tau, f, log_n, 0) == want == expected(tau, f, log_n, 0)


@pytest.mark.parametrize("tau_kind", ("one", "on_domain"))
def test_host_loop_degenerate_points(lib, tau_kind):
    """tau = 1: every point is G, so additions meet doublings and cancellations; tau = w_8: tau on the domain"""
    rnd = random.Random(8)
    tau = 1 if tau_kind == "one" else M.omega(8)
    f = [rnd.randrange(Q) for _ in range(8)]
    assert proofs(lib, tau, f, 3, 1) == expected(tau, f, 3, 1)

"""CPU checks of csrc/prover_host.hpp, the host arithmetic of the native prover: the constants of the quotient coset, the choice of
path under the BP_PROVE_* knobs, and the scalars rounds 3 and 5 hand to their kernels; no GPU: the header is compiled for the host
alone (tests/cpp/prover_host_host.hip).  Every expectation is a Python-integer closed form written out below; none comes from the
header under test."""
import ctypes as C
import itertools
import os
import random
import subprocess

import pytest

from tests import prover_rounds as PR
from tests.bigint_model import Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ph(tmp_path_factory):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    so = str(tmp_path_factory.mktemp("prover_host") / "libproverhost.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O1", "-fPIC", "-shared",
                           os.path.join(ROOT, "tests", "cpp", "prover_host_host.hip"), "-o", so])
    lib = C.CDLL(so)
    i32, u32, u64, buf = C.c_int, C.c_uint32, C.c_uint64, C.c_char_p
    for name, res, args in (("ph_coset_consts", None, [u32, buf, buf]), ("ph_knob_tristate", i32, [buf]),
                            ("ph_prove_paths", i32, [u32] + [i32] * 7), ("ph_quotient_args", None, [buf, buf, buf]),
                            ("ph_round5_scalars", None, [u64, buf, buf])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def enc(values):
    assert all(0 <= v < Q for v in values)
    return b"".join(v.to_bytes(32, "little") for v in values)


def dec(raw):
    return [int.from_bytes(raw[i: i + 32], "little") for i in range(0, len(raw), 32)]


@pytest.mark.parametrize("log_n", [3, 10, 24])
def test_coset_consts(ph, log_n):
    """the quotient coset g <w_4n>, g = 7, as the four cosets s_j <w_n>: s_j = g w_4n^j, X^n = s_j^n = g^n i4^j on coset j"""
    n = 1 << log_n
    consts, recombine = C.create_string_buffer(27 * 32), C.create_string_buffer(5 * 32)
    ph.ph_coset_consts(log_n, consts, recombine)
    v = dec(consts.raw)
    g, ginv, w4n, gn, i4, iinv, n_inv = v[:7]
    s, s_inv, sn, zh_inv, scale = (v[7 + 4 * k: 11 + 4 * k] for k in range(5))
    assert g == 7 and ginv * 7 % Q == 1 and n_inv * n % Q == 1
    assert pow(w4n, 4 * n, Q) == 1 and pow(w4n, 2 * n, Q) == Q - 1
    assert w4n == PR.root_of_unity(4 * n)
    assert i4 == pow(w4n, n, Q) and i4 * i4 % Q == Q - 1 and iinv * i4 % Q == 1
    assert gn == pow(7, n, Q)
    for j in range(4):
        assert s[j] == 7 * pow(w4n, j, Q) % Q and s_inv[j] * s[j] % Q == 1
        assert sn[j] == pow(s[j], n, Q) == gn * pow(i4, j, Q) % Q
        assert zh_inv[j] * (sn[j] - 1) % Q == 1
        assert scale[j] * 4 * pow(gn, j, Q) % Q == 1
    assert dec(recombine.raw) == scale + [iinv]                # RecombineArgs: scale[4], iinv


def round5_closed_form(n, alpha, beta, gamma, zeta, nu, a, b, c, s1, s2, zw, pi):
    """prover.rs:543-634 as one linear combination over  qm ql qr qo qc | z | s3 | t_lo t_mid t_hi | a b c s1 s2"""
    zn = pow(zeta, n, Q)
    Z = (zn - 1) % Q
    L = 1 if zeta == 1 else Z * pow(n * (zeta - 1), -1, Q) % Q
    f = (a + beta * zeta + gamma) * (b + 2 * beta * zeta + gamma) * (c + 3 * beta * zeta + gamma) % Q
    g = (a + beta * s1 + gamma) * (b + beta * s2 + gamma) % Q
    coef = [a * b, a, b, c, 1, alpha * f + alpha * alpha * L, -alpha * beta * g * zw, -Z, -zn * Z, -zn * zn * Z,
            nu, nu**2, nu**3, nu**4, nu**5]
    const = pi - alpha * g * zw * (c + gamma) - alpha * alpha * L - (nu * a + nu**2 * b + nu**3 * c + nu**4 * s1 + nu**5 * s2)
    return [x % Q for x in coef], const % Q


def round5_cases():
    rng = random.Random(5)
    rnd = lambda: [rng.randrange(Q) for _ in range(12)]       # alpha beta gamma zeta nu a b c s1 s2 zw pi
    for n in (8, 1 << 24):
        yield "random", n, rnd()
        yield "all q - 1", n, [Q - 1] * 12
        for name, at, value in (("zeta = 1", 3, 1), ("zeta an n-th root of unity", 3, pow(PR.root_of_unity(n), 3, Q)), ("nu = 1", 4, 1),
                                ("PI(zeta) = 0", 11, 0)):
            case = rnd()
            case[at] = value
            yield name, n, case


@pytest.mark.parametrize("name,n,case", [pytest.param(*c, id="%s, n = %d" % c[:2]) for c in round5_cases()])
def test_round5_scalars(ph, name, n, case):
    if name == "zeta an n-th root of unity":
        assert case[3] != 1 and pow(case[3], n, Q) == 1           # Z = 0 and L = 0
    out = C.create_string_buffer(16 * 32)
    ph.ph_round5_scalars(n, enc(case), out)
    got = dec(out.raw)
    coef, const = round5_closed_form(n, *case)
    assert got[:15] == coef
    assert got[15] == const


KNOB = (-1, 0, 1)                                                 # unset, "0", "1"


def test_knob_tristate(ph):
    """only a first character 0 or 1 sets a knob; everything else counts as unset"""
    for value, want in ((None, -1), (b"", -1), (b"0", 0), (b"1", 1), (b"2", -1), (b"x", -1), (b"-1", -1), (b" 1", -1), (b"01", 0), (b"10", 1),
                        (b"1x", 1), (b"yes", -1)):
        assert ph.ph_knob_tristate(value) == want, value


def test_prove_paths_full_table(ph):
    """a knob overrides the size threshold, never the feasibility"""
    cases = 0
    for log_n, host, group, has_split in itertools.product((3, 17, 18, 19, 20, 24), (0, 1), (0, 1), (0, 1)):
        for k_staged, k_split, k_side, k_early in itertools.product(KNOB, repeat=4):
            staged = bool(host) and not group and (k_staged == 1 if k_staged != -1 else log_n >= 18)
            split = bool(has_split) and k_split != 0
            side = not split and (k_side == 1 if k_side != -1 else log_n < 20)
            early = split and k_early != 0
            got = ph.ph_prove_paths(log_n, host, group, has_split, k_staged, k_split, k_side, k_early)
            assert got == staged | split << 1 | side << 2 | early << 3, (log_n, host, group, has_split, k_staged, k_split, k_side, k_early)
            cases += 1
    assert cases == 6 * 8 * 81


def test_quotient_args(ph):
    rng = random.Random(3)
    for abg in ([rng.randrange(Q) for _ in range(3)], [Q - 1] * 3, [0, 0, 0], [1, 1, 1]):
        zh = [rng.randrange(Q) for _ in range(4)]
        out = C.create_string_buffer(11 * 32)
        ph.ph_quotient_args(enc(abg), enc(zh), out)
        alpha, beta, gamma = abg
        assert dec(out.raw) == [alpha, alpha * alpha % Q, beta, gamma, 2 * beta % Q, 3 * beta % Q, 1] + zh

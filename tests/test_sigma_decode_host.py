"""CPU checks of csrc/sigma_decode.hpp: a value of S1, S2, S3 back to the cell whose label (col + 1) w^row it is (utils.rs:28-37,
program.rs:126-137), by the n-th power for the column and a bit-by-bit discrete logarithm for the row.  No GPU: the header is compiled
for the host alone (tests/cpp/sigma_decode_host.hip) with the device's multiplier.  Every expectation is a Python integer."""
import ctypes as C
import os
import random
import subprocess

import pytest

from tests import general_circuits as G
from tests.bigint_model import Q, ROOT_OF_UNITY, omega

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = pow(2, 256, Q)
NO_CELL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def sd(tmp_path_factory):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    so = str(tmp_path_factory.mktemp("sigma_decode") / "libsigmadecode.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O1", "-fPIC", "-shared",
                           os.path.join(ROOT, "tests", "cpp", "sigma_decode_host.hip"), "-o", so])
    lib = C.CDLL(so)
    lib.sd_decode_cells.restype, lib.sd_decode_cells.argtypes = None, [C.c_uint32, C.c_char_p, C.c_size_t, C.c_void_p]
    lib.sd_decode_columns.restype, lib.sd_decode_columns.argtypes = C.c_size_t, [C.c_uint32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p]
    lib.sd_consts.restype, lib.sd_consts.argtypes = None, [C.c_uint32, C.c_void_p]
    return lib


def mont(values):
    assert all(0 <= v < Q for v in values)
    return b"".join((v * R % Q).to_bytes(32, "little") for v in values)


def decode(sd, log_n, values):
    out = (C.c_uint32 * len(values))()
    sd.sd_decode_cells(log_n, mont(values), len(values), out)
    return list(out)


def label(n, col, row):
    return (col + 1) * pow(omega(n), row, Q) % Q


@pytest.mark.parametrize("log_n", [3, 10, 24])
def test_constants(sd, log_n):
    n = 1 << log_n
    raw = C.create_string_buffer(30 * 32)
    sd.sd_consts(log_n, raw)
    v = [int.from_bytes(raw.raw[32 * i: 32 * i + 32], "little") * pow(R, -1, Q) % Q for i in range(30)]
    assert v[:3] == [1, pow(2, n, Q), pow(3, n, Q)] and len(set(v[:3])) == 3
    assert [v[3 + k] * (k + 1) % Q for k in range(3)] == [1, 1, 1]
    w = omega(n)
    assert w == pow(ROOT_OF_UNITY, (1 << 32) // n, Q)
    for j in range(24):
        assert v[6 + j] == (pow(w, -(1 << j), Q) if j < log_n else 1), j


@pytest.mark.parametrize("n", [8, 16])
def test_every_label_decodes_to_its_cell(sd, n):
    cells = [(col, row) for row in range(n) for col in range(3)]
    got = decode(sd, n.bit_length() - 1, [label(n, col, row) for col, row in cells])
    assert got == [3 * row + col for col, row in cells]


@pytest.mark.parametrize("log_n", [3, 10, 24])
def test_rows_at_the_edges(sd, log_n):
    n = 1 << log_n
    for row in (0, 1, n // 2, n - 1, n - 2):
        assert decode(sd, log_n, [label(n, col, row) for col in range(3)]) == [3 * row + col for col in range(3)], row
    assert decode(sd, log_n, [1, Q - 1]) == [0, 3 * (n // 2)]            # 1 -> (0, 0), q - 1 = w^(n/2) -> (0, n/2)


@pytest.mark.parametrize("log_n", [3, 4, 10, 24])
def test_values_that_are_no_label(sd, log_n):
    n = 1 << log_n
    w, w2n = omega(n), omega(2 * n)
    assert pow(w2n, n, Q) == Q - 1
    bad = [0] + [4 * pow(w, r, Q) % Q for r in (0, 1, n - 1)]
    bad += [k * w2n % Q for k in (1, 2, 3)]                              # n-th power -k^n
    bad += [k * pow(w2n, r, Q) % Q for k in (1, 2, 3) for r in (1, 3, 2 * n - 1)]      # labels of a circuit twice the size, odd rows
    assert decode(sd, log_n, bad) == [NO_CELL] * len(bad)


def test_random_elements_are_no_label(sd):
    rnd = random.Random(1)
    vals = [rnd.randrange(Q) for _ in range(1000)]
    labels = {label(16, col, row) for col in range(3) for row in range(16)}
    assert not labels & set(vals)
    assert decode(sd, 4, vals) == [NO_CELL] * 1000


def test_limbs_not_below_q_are_no_label(sd):
    out = (C.c_uint32 * 2)()
    sd.sd_decode_cells(4, Q.to_bytes(32, "little") + b"\xff" * 32, 2, out)
    assert list(out) == [NO_CELL, NO_CELL]


@pytest.mark.parametrize("shape", G.SHAPES[:2] + (G.NO_PUBLIC,), ids=["n16", "n128", "n128_no_public"])
def test_host_loop_reproduces_the_copy_cycles(sd, shape):
    """the decoded columns are a bijection of the 3n cells whose cycles are general_circuits.copy_cycles"""
    n = shape[0]
    pk = G.general_circuit(*shape)[1]
    target = (C.c_uint32 * (3 * n))()
    assert sd.sd_decode_columns(n.bit_length() - 1, mont(pk["s1"]), mont(pk["s2"]), mont(pk["s3"]), target) == 0
    t = list(target)
    assert sorted(t) == list(range(3 * n))
    cycles = G.copy_cycles(pk)
    assert sum(len(c) for c in cycles) == 3 * n
    for cyc in cycles:
        for k, (col, row) in enumerate(cyc):                             # copy_cycles walks cur -> the cell its S value names
            ncol, nrow = cyc[(k + 1) % len(cyc)]
            assert t[3 * row + col] == 3 * nrow + ncol
    s1 = list(pk["s1"])
    s1[5] = 4 * omega(n) % Q
    assert sd.sd_decode_columns(n.bit_length() - 1, mont(s1), mont(pk["s2"]), mont(pk["s3"]), target) == 1
    assert target[3 * 5] == NO_CELL

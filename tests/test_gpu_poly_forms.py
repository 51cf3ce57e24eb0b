"""-m gpu: every Polynomial operator of the C ABI in its host form and its device form, on one table of the smallest operands that
reach each rule of csrc/poly_rules.hpp (polynomial.rs:14-380).  Each case goes through the host entry point in both scalar formats
and through the *_device entry point; return code, n_out and values are compared with Python integers mod q, and the forms with
each other.  Every case runs in all three columns; there is no fourth, because the *_device entry points take Montgomery limbs only
(no canonical-bytes input exists on the device)."""
import ctypes as C

import numpy as np
import pytest

import baby_plonk_rust_amd as bp
from tests.gpu_common import Q

pytestmark = pytest.mark.gpu
MONO, LAG = bp.BASIS_MONOMIAL, bp.BASIS_LAGRANGE
POISON = 0xEEEEEEEE                        # n_out before a call: a refusal leaves it alone


@pytest.fixture(scope="module")
def ctx():
    return bp.default_context()


class HostForm:
    suffix = ""

    def __init__(self, fmt):
        self.fmt, self.fmt_args = fmt, (fmt,)
        self.name = "host/mont" if fmt == bp.FR_MONT else "host/bytes"

    def encode(self, vals):
        if self.fmt == bp.FR_MONT:
            return np.ascontiguousarray(bp.scalars_from_ints(list(vals)), dtype=np.uint64).reshape(-1, 4).copy()
        return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()

    def decode(self, arr):
        if self.fmt == bp.FR_MONT:
            return [int(v) for v in bp.scalars_to_ints(np.ascontiguousarray(arr))]
        return [int.from_bytes(row.tobytes(), "little") for row in arr]

    def vec(self, vals):                   # at least one element of room: an empty operand still has a pointer
        return self.encode(list(vals) or [0])

    def out(self, n):
        return np.full((max(n, 1), 4), 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)

    def ptr(self, buf):
        return buf.ctypes.data

    def read(self, buf, n):
        return self.decode(buf[:n])


class DeviceForm(HostForm):
    suffix, name = "_device", "device/mont"

    def __init__(self, device):
        self.fmt, self.fmt_args, self.device = bp.FR_MONT, (), device

    def vec(self, vals):
        import torch
        t = torch.from_numpy(self.encode(list(vals) or [0]).view(np.int64)).to(torch.device("cuda", self.device))
        torch.cuda.current_stream().synchronize()
        return t

    def out(self, n):
        import torch
        t = torch.full((max(n, 1), 4), -0x1111111111111112, dtype=torch.int64, device=torch.device("cuda", self.device))
        torch.cuda.current_stream().synchronize()
        return t

    def ptr(self, buf):
        return buf.data_ptr()

    def read(self, buf, n):
        return self.decode(buf[:n].cpu().numpy().view(np.uint64))


def forms(ctx):
    return [HostForm(bp.FR_MONT), HostForm(bp.FR_BYTES_LE), DeviceForm(ctx.device)]


# ---------------------------------------------------------------------------------------------- the table
# (id, op, basis, a, b or scalar, return code, values or None)
def m(vals):
    return [v % Q for v in vals]


def addsub_case(op, basis, a, b):
    """polynomial.rs:57-174: Lagrange operands of one length (-6 otherwise), Monomial ones padded with zeros to the longer"""
    sign = 1 if op == "add" else -1
    if basis == LAG and len(a) != len(b):
        return -6, None
    n = max(len(a), len(b))
    pad = lambda v: list(v) + [0] * (n - len(v))
    return 0, [(x + sign * y) % Q for x, y in zip(pad(a), pad(b))]


def scalar_case(op, basis, a, s):
    """Mul<Scalar> scales every value; Lagrange Add AND Sub add s to every value (polynomial.rs:126-128); Monomial Add / Sub change
    values[0] alone and panic on the empty polynomial (:62, :123)"""
    if op == 2:
        return 0, [v * s % Q for v in a]
    if basis == LAG:
        return 0, [(v + s) % Q for v in a]
    if not a:
        return -1, None
    return 0, [(a[0] + (s if op == 0 else -s)) % Q] + list(a[1:])


def mul_case(basis, a, b):
    """polynomial.rs:176-312: todo!() for Lagrange, len - 1 underflows on an empty operand, else the na + nb - 1 product coefficients"""
    if basis != MONO:
        return -5, None
    if not a or not b:
        return -1, None
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % Q
    return 0, out


def evaluate_case(basis, a, x):
    return (0, [sum(c * pow(x, i, Q) for i, c in enumerate(a)) % Q]) if basis == MONO else (-5, None)


A3, B3, B2, A2 = [7, Q - 1, 3], [Q - 5, 11, Q - 2], [Q - 4, 9], [5, Q - 6]
S = Q - 3
CASES = []
for op in ("add", "sub"):
    for a, b in (([], []), ([], B3), (A3, []), (A3, B2), (A2, B3)):
        CASES.append(("%s mono (%d,%d)" % (op, len(a), len(b)), op, MONO, a, b) + addsub_case(op, MONO, a, b))
    CASES.append(("%s lag (3,3)" % op, op, LAG, A3, B3) + addsub_case(op, LAG, A3, B3))
    CASES.append(("%s lag (3,2) -> -6" % op, op, LAG, A3, B2) + addsub_case(op, LAG, A3, B2))
    CASES.append(("%s lag (0,0)" % op, op, LAG, [], []) + addsub_case(op, LAG, [], []))
for op in (0, 1, 2):
    for basis in (MONO, LAG):
        for a in ([], [Q - 2], A3):
            CASES.append(("scalar op %d %s n=%d" % (op, "mono" if basis == MONO else "lag", len(a)), "scalar%d" % op, basis, a, S)
                         + scalar_case(op, basis, a, S))
CASES += [("mul (1,1)", "mul", MONO, [Q - 2], [Q - 3]) + mul_case(MONO, [Q - 2], [Q - 3]),
          ("mul (3,2)", "mul", MONO, A3, B2) + mul_case(MONO, A3, B2),
          ("mul (2,2): 2^k + 1 coefficients", "mul", MONO, A2, B2) + mul_case(MONO, A2, B2),
          ("mul (0,2) -> -1", "mul", MONO, [], B2) + mul_case(MONO, [], B2),
          ("mul (3,0) -> -1", "mul", MONO, A3, []) + mul_case(MONO, A3, []),
          ("mul lag -> -5", "mul", LAG, A3, B3) + mul_case(LAG, A3, B3),
          # the literals of test_div_literals_quirk_and_random (polynomial.rs:453-521)
          ("div exact", "div", MONO, m([-1, -1, -1, 3]), m([-1, 1]), 0, [1, 2, 3]),
          ("div trailing zeros on both", "div", MONO, m([-1, -1, -1, 3, 0, 0]), m([-1, 1, 0]), 0, [1, 2, 3]),
          ("div with a remainder", "div", MONO, [1, 0, 1], [1, 1], 0, [Q - 1, 1]),
          ("div squeezes a zero coefficient", "div", MONO, m([-1, 0, 0, 0, 1]), m([-1, 0, 1]), 0, [1, 1]),
          ("div general divisor", "div", MONO, [2, 7, 13, 11, 3], [1, 2, 3], 0, [2, 3, 1]),      # (1 + 2x + 3x^2)(2 + 3x + x^2)
          ("div na < nb -> empty", "div", MONO, [5], [1, 1], 0, []),
          ("div zero dividend -> empty", "div", MONO, [0, 0], [1, 1], 0, []),
          ("div empty dividend -> empty", "div", MONO, [], [1, 1], 0, []),
          ("div zero divisor -> -7", "div", MONO, [1, 2], [0, 0], -7, None),
          ("div empty divisor -> -7", "div", MONO, [1, 2], [], -7, None),
          ("div lag -> -5", "div", LAG, [1, 2], [1, 1], -5, None)]
for a in ([], [Q - 2], A3):
    CASES.append(("evaluate n=%d" % len(a), "evaluate", MONO, a, S) + evaluate_case(MONO, a, S))
CASES += [("evaluate lag -> -5", "evaluate", LAG, A3, S) + evaluate_case(LAG, A3, S),
          ("grand product n=0", "grand_product", LAG, [], None, 0, [])]


def run(ctx, form, op, basis, a, b):
    """-> (return code, n_out, values): values None after a refusal, n_out POISON where a refusal left it alone"""
    lib, h = ctx._lib, ctx._h
    va = form.vec(a)
    if op in ("add", "sub", "mul", "div"):
        vb, out, n = form.vec(b), form.out(len(a) + len(b) + 1), C.c_size_t(POISON)
        rc = getattr(lib, "bp_poly_%s%s" % (op, form.suffix))(h, form.ptr(va), len(a), form.ptr(vb), len(b), basis, *form.fmt_args, form.ptr(out),
                                                              C.byref(n))
        return rc, n.value, form.read(out, n.value) if rc == 0 else None
    if op.startswith("scalar"):
        s, out = form.encode([b]), form.out(len(a))
        rc = getattr(lib, "bp_poly_scalar_op" + form.suffix)(h, form.ptr(va), len(a), basis, s.ctypes.data, int(op[-1]), *form.fmt_args, form.ptr(out))
        return rc, len(a) if rc == 0 else POISON, form.read(out, len(a)) if rc == 0 else None
    if op == "evaluate":
        x, r = form.encode([b]), np.zeros((1, 4), dtype=np.uint64)
        rc = getattr(lib, "bp_poly_evaluate" + form.suffix)(h, form.ptr(va), len(a), basis, x.ctypes.data, *form.fmt_args, r.ctypes.data)
        return rc, 1 if rc == 0 else POISON, form.decode(r) if rc == 0 else None
    assert op == "grand_product" and not a
    scal = [form.encode([v]) for v in (5, 6, 2, 3)]
    rc = getattr(lib, "bp_grand_product" + form.suffix)(h, *[None] * 6, 0, *[s.ctypes.data for s in scal], *form.fmt_args, None)
    return rc, 0, []


def test_table_reaches_every_rule():
    """every case has a name of its own, and between them the cases meet every code the rules return"""
    ids = [c[0] for c in CASES]
    assert len(set(ids)) == len(ids)
    assert {c[5] for c in CASES} == {0, -1, -5, -6, -7}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_and_device_forms(ctx, case):
    name, op, basis, a, b, want_rc, want = case
    got = {}
    for form in forms(ctx):
        rc, n_out, vals = run(ctx, form, op, basis, a, b)
        assert rc == want_rc, (name, form.name, rc)
        if rc == 0:
            assert n_out == len(want) and vals == want, (name, form.name, n_out, vals, want)
        else:
            assert n_out == POISON, (name, form.name, n_out)
        got[form.name] = (rc, n_out, vals)
    assert got["host/mont"] == got["host/bytes"] == got["device/mont"], got

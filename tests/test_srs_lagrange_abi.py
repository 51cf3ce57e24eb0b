"""The entry points of the Lagrange-basis SRS without a GPU: they are exported, bound with the header's signatures, declared in the
Rust bindings, and refuse a missing context or output with BP_ERR_INVALID_ARG instead of crashing; and the commit rule they bring
(rule_commit_srs of csrc/poly_rules.hpp), compiled for the host alone."""
import ctypes as C
import os
import subprocess

import pytest

import baby_plonk_rust_amd as bp
from baby_plonk_rust_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lagrange_entry_points_reject_bad_arguments_without_a_gpu():
    lib = bp.load()
    h, basis, log_n = C.c_uint64(7), C.c_int(-1), C.c_uint32(99)
    assert lib.bp_srs_lagrange(None, 1, 3, C.byref(h)) == -1 and h.value == 7
    assert lib.bp_srs_lagrange(None, 1, 3, None) == -1
    assert lib.bp_srs_lagrange(None, 1, 25, C.byref(h)) == -1              # no context: nothing else is looked at
    assert lib.bp_srs_basis(None, 1, C.byref(basis), C.byref(log_n)) == -1 and (basis.value, log_n.value) == (-1, 99)
    assert lib.bp_srs_basis(None, 1, None, None) == -1


def test_lagrange_entry_points_are_declared_everywhere():
    header = open(os.path.join(ROOT, "include", "bp_msm_ntt.h")).read()
    rust = open(os.path.join(ROOT, "include", "bp_msm_ntt.rs")).read()
    for name, nargs in (("bp_srs_lagrange", 4), ("bp_srs_basis", 4)):
        assert "int  %s(bp_ctx* ctx, uint64_t srs_handle," % name in header
        assert "pub fn %s(" % name in rust
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs
    assert hasattr(bp.Context, "srs_lagrange") and hasattr(bp.Context, "srs_basis") and hasattr(bp.Setup, "lagrange")
    assert isinstance(bp.Setup.basis, property)


def test_commit_rule_of_an_srs_that_knows_its_basis(tmp_path):
    """rule_commit_srs (csrc/poly_rules.hpp), compiled for the host alone: the polynomial's basis must be the SRS's.  A Monomial SRS
    keeps rule_commit at every length; a Lagrange SRS takes Lagrange polynomials of exactly its length; every refusal has its text"""
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    so = str(tmp_path / "libcommitrule.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-host-only", "-O1", "-fPIC", "-shared",
                           os.path.join(ROOT, "tests", "cpp", "commit_rule_host.hip"), "-o", so])
    fn = C.CDLL(so).cr_commit_srs
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_size_t, C.c_int, C.c_size_t, C.POINTER(C.c_int)]
    LAG, MONO, OK, BASIS, LENGTH = _lib.BASIS_LAGRANGE, _lib.BASIS_MONOMIAL, 0, -5, -6

    def rule(basis, n, srs_basis, srs_len):
        text = C.c_int(-1)
        code = fn(basis, n, srs_basis, srs_len, C.byref(text))
        assert text.value == (code != OK)
        return code

    for n in (0, 1, 511, 512, 513, 1024, 1 << 40):
        assert rule(MONO, n, MONO, 512) == OK and rule(LAG, n, MONO, 512) == BASIS            # as rule_commit: any length, Monomial only
        assert rule(MONO, n, LAG, 512) == BASIS                                             # the basis is looked at before the length
        assert rule(LAG, n, LAG, 512) == (OK if n == 512 else LENGTH)
    assert rule(LAG, 1, LAG, 1) == OK and rule(LAG, 0, LAG, 1) == LENGTH and rule(LAG, 1 << 24, LAG, 1 << 24) == OK

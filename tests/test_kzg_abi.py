"""The KZG entry points of include/bp_msm_ntt.h without a GPU: they are exported, bound in the ctypes table, and answer a null
context or null pointers with BP_ERR_INVALID_ARG (-1) -- never a crash.  (Header, table and Rust bindings in step: tests/test_abi.py.)"""
import ctypes as C

import numpy as np

import baby_plonk_rust_amd as bp
from baby_plonk_rust_amd import _lib

KZG = ("bp_kzg_open_device", "bp_kzg_open", "bp_kzg_verify_reduce", "bp_kzg_last_stats")


def test_kzg_entry_points_are_exported_and_bound():
    lib = bp.load()
    for name in KZG:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name


def test_kzg_entry_points_refuse_null_arguments_without_a_gpu():
    lib = bp.load()
    buf = np.zeros(192, dtype=np.uint8)
    p = buf.ctypes.data
    ptrs, lens = (C.c_void_p * 1)(p), (C.c_size_t * 1)(1)
    bad = C.c_size_t()
    for fn in (lib.bp_kzg_open_device, lib.bp_kzg_open):
        assert fn(None, 1, ptrs, lens, 1, bp.BASIS_MONOMIAL, p, None, bp.FR_MONT, p, p) == -1          # no context
        assert fn(None, 1, None, None, 1, bp.BASIS_MONOMIAL, None, None, bp.FR_MONT, None, None) == -1
    assert lib.bp_kzg_verify_reduce(None, p, 1, 1, p, p, None, p, None, bp.FR_MONT, 0, p, C.byref(bad)) == -1
    assert lib.bp_kzg_verify_reduce(None, None, 1, 1, None, None, None, None, None, bp.FR_MONT, 0, None, None) == -1
    assert lib.bp_kzg_last_stats(None, (C.c_float * 3)()) == -1
    assert lib.bp_kzg_last_stats(None, None) == -1


def test_opening_record_is_public():
    o = bp.Opening(commitments=b"", z=None, ys=None, nu=None, proof=b"")
    assert o._fields == ("commitments", "z", "ys", "nu", "proof")
    for name in ("open", "opening_pairing_inputs", "verify_openings"):
        assert callable(getattr(bp.Setup, name))
    assert callable(bp.Context.kzg_stats)

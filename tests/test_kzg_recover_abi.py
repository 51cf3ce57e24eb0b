"""The cell-recovery entry points of the C ABI without a GPU: the four names are exported and bound, they refuse a null context, null
pointers and a bad format with BP_ERR_INVALID_ARG before anything is touched, and the Python names are public."""
import ctypes as C
import inspect

import numpy as np

import baby_plonk_rust_amd as bp
from baby_plonk_rust_amd import _lib

NAMES = ("bp_kzg_recover", "bp_kzg_recover_device", "bp_kzg_recover_cells", "bp_kzg_recover_last_stats")


def test_names_are_exported_and_bound():
    lib = bp.load()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.KZG_RECOVER_WALK == 256


def test_null_context_pointers_and_format_are_refused_and_nothing_is_written():
    lib = bp.load()
    idx = np.array([0, 1], dtype=np.uint32)
    vals = np.zeros((2, 2, 4), dtype=np.uint64)
    out, proofs, ms = np.full(32 * 8, 0xA5, dtype=np.uint8), np.full(96 * 4, 0xA5, dtype=np.uint8), (C.c_float * 4)(7, 7, 7, 7)
    bad = C.c_size_t(12345)
    i, v, o, p = idx.ctypes.data, vals.ctypes.data, out.ctypes.data, proofs.ctypes.data
    # no context: every argument pattern, good or bad, is BP_ERR_INVALID_ARG
    for fmt in (_lib.FR_MONT, _lib.FR_BYTES_LE, 7):
        assert lib.bp_kzg_recover(None, 3, 1, i, v, 2, 4, fmt, o, C.byref(bad)) == -1
        assert lib.bp_kzg_recover_cells(None, 1, 3, 1, i, v, 2, 4, fmt, o, p, C.byref(bad)) == -1
    assert lib.bp_kzg_recover(None, 3, 1, None, None, 2, 4, _lib.FR_MONT, None, None) == -1
    assert lib.bp_kzg_recover_device(None, 3, 1, i, v, 2, 4, o, C.byref(bad)) == -1
    assert lib.bp_kzg_recover_device(None, 3, 1, None, None, 2, 4, None, None) == -1
    assert lib.bp_kzg_recover_cells(None, 1, 3, 1, None, None, 2, 4, _lib.FR_MONT, None, None, None) == -1
    assert lib.bp_kzg_recover_last_stats(None, ms) == -1 and lib.bp_kzg_recover_last_stats(None, None) == -1
    assert (out == 0xA5).all() and (proofs == 0xA5).all() and list(ms) == [7, 7, 7, 7] and bad.value == 12345


def test_python_names_are_public():
    for name in ("recover_polynomial", "recover_polynomial_device"):
        assert callable(getattr(bp, name)), name
    assert callable(bp.Setup.recover_cells) and callable(bp.Context.kzg_recover_stats)
    assert inspect.signature(bp.recover_polynomial).parameters["n_coeffs"].default is None
    assert list(inspect.signature(bp.recover_polynomial).parameters) == ["indices", "cells", "group_order", "n_coeffs", "ctx", "fmt"]
    assert list(inspect.signature(bp.recover_polynomial_device).parameters) == ["indices", "d_cells", "cell_size", "group_order", "n_coeffs", "ctx"]
    assert list(inspect.signature(bp.Setup.recover_cells).parameters) == ["self", "indices", "cells", "group_order", "n_coeffs"]

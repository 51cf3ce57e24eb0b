"""The cell-proof entry points of include/bp_msm_ntt.h without a GPU: they are exported, bound in the ctypes table, and answer a
null context, null pointers and an out-of-range format or basis with BP_ERR_INVALID_ARG (-1) -- never a crash, and nothing is
written.  (Header, table and Rust bindings in step: tests/test_abi.py.)"""
import ctypes as C

import numpy as np

import baby_plonk_rust_amd as bp
from baby_plonk_rust_amd import _lib

CELLS = ("bp_srs_open_cosets_prepare", "bp_kzg_open_cosets", "bp_kzg_open_cosets_device", "bp_kzg_verify_cells_reduce")


def test_cell_entry_points_are_exported_and_bound():
    lib = bp.load()
    for name in CELLS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name


def test_cell_entry_points_refuse_null_and_out_of_range_arguments_without_a_gpu():
    lib = bp.load()
    buf = np.full(192, 0xA5, dtype=np.uint8)
    p = buf.ctypes.data
    idx = np.zeros(1, dtype=np.uint32)
    bad = C.c_size_t(7)
    assert lib.bp_srs_open_cosets_prepare(None, 1, 3, 1) == -1
    assert lib.bp_srs_open_cosets_prepare(None, 1, 3, 0) == -1                                                  # l = 1: the open_all call
    assert lib.bp_srs_open_cosets_prepare(None, 1, 1, 3) == -1                                                  # log_l > log_n
    for log_l in (0, 1, 3, 4):
        assert lib.bp_kzg_open_cosets(None, 1, p, 1, bp.BASIS_MONOMIAL, bp.FR_MONT, 3, log_l, p, p) == -1       # no context
        assert lib.bp_kzg_open_cosets(None, 1, p, 1, bp.BASIS_MONOMIAL, 7, 3, log_l, p, p) == -1                # and a bad format
        assert lib.bp_kzg_open_cosets(None, 1, p, 1, 9, bp.FR_MONT, 3, log_l, p, p) == -1                       # a bad basis
        assert lib.bp_kzg_open_cosets(None, 1, None, 1, bp.BASIS_MONOMIAL, bp.FR_MONT, 3, log_l, None, None) == -1
        assert lib.bp_kzg_open_cosets_device(None, 1, p, 1, bp.BASIS_MONOMIAL, 3, log_l, p, p) == -1
        assert lib.bp_kzg_open_cosets_device(None, 1, None, 1, 9, 3, log_l, None, None) == -1
    assert lib.bp_kzg_open_cosets(None, 1, p, 1, bp.BASIS_MONOMIAL, bp.FR_MONT, 24, 6, p, p) == -1
    assert lib.bp_kzg_verify_cells_reduce(None, 1, 3, 1, p, idx.ctypes.data, p, p, 1, None, bp.FR_MONT, 0, p, C.byref(bad)) == -1
    assert lib.bp_kzg_verify_cells_reduce(None, 1, 3, 1, None, None, None, None, 1, None, bp.FR_MONT, 0, None, None) == -1
    assert lib.bp_kzg_verify_cells_reduce(None, 1, 1, 3, p, idx.ctypes.data, p, p, 1, None, 7, 0, p, C.byref(bad)) == -1
    assert lib.bp_kzg_verify_cells_reduce(None, 1, 3, 1, p, idx.ctypes.data, p, p, 0, None, bp.FR_MONT, 0, p, None) == -1
    assert (buf == 0xA5).all() and bad.value == 7 and idx[0] == 0                                               # nothing was written


def test_cell_record_and_methods_are_public():
    o = bp.CellOpening(commitment=b"", index=0, values=None, proof=b"")
    assert o._fields == ("commitment", "index", "values", "proof")
    for name in ("prepare_open_cosets", "open_cosets", "cell_pairing_inputs", "verify_cells"):
        assert callable(getattr(bp.Setup, name))

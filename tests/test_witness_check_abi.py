"""bp_circuit_check_sigma, bp_circuit_check_witness and bp_circuit_check_last_stats without a context or a GPU: null pointers and bad
formats are BP_ERR_INVALID_ARG (-1), never a crash, and a rejected call leaves `report` untouched."""
import ctypes as C

import numpy as np

import baby_plonk_rust_amd as bp


def test_check_entry_points_reject_bad_arguments_without_a_gpu():
    lib = bp.load()
    mark = 0x1122334455667788
    rep4, rep5, ms = (C.c_uint64 * 4)(*[mark] * 4), (C.c_uint64 * 5)(*[mark] * 5), (C.c_float * 3)(7, 7, 7)
    col = np.zeros((8, 4), dtype=np.uint64)
    p = col.ctypes.data
    assert lib.bp_circuit_check_sigma(None, 1, rep4) == -1
    assert lib.bp_circuit_check_sigma(None, 1, None) == -1
    assert lib.bp_circuit_check_sigma(None, 0, rep4) == -1
    for fmt, dev in ((bp.FR_MONT, 0), (bp.FR_BYTES_LE, 0), (bp.FR_MONT, 1), (bp.FR_BYTES_LE, 1), (2, 0), (-1, 1)):
        assert lib.bp_circuit_check_witness(None, 1, p, p, p, p, fmt, dev, rep5) == -1, (fmt, dev)
        assert lib.bp_circuit_check_witness(None, 1, p, p, p, None, fmt, dev, rep5) == -1, (fmt, dev)
    assert lib.bp_circuit_check_witness(None, 1, None, None, None, None, bp.FR_MONT, 0, None) == -1
    assert lib.bp_circuit_check_last_stats(None, ms) == -1
    assert lib.bp_circuit_check_last_stats(None, None) == -1
    assert list(rep4) == [mark] * 4 and list(rep5) == [mark] * 5 and list(ms) == [7, 7, 7]


def test_python_reports_name_cells_by_column_and_row():
    from baby_plonk_rust_amd import api
    assert api._cell(0) == (0, 0) and api._cell(5) == (2, 1) and api._cell(3 * (1 << 24) - 1) == (2, (1 << 24) - 1)
    assert api._cell(0xFFFFFFFFFFFFFFFF) is None
    assert bp.SigmaReport(0, None, 0, None).ok and not bp.SigmaReport(1, (0, 0), 0, None).ok and not bp.SigmaReport(0, None, 2, (1, 3)).ok
    assert bp.WitnessReport(0, None, 0, None, None).ok and not bp.WitnessReport(1, 4, 0, None, None).ok
    assert not bp.WitnessReport(0, None, 2, (2, 0), (0, 1)).ok

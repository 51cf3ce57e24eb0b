"""The wire-id entry points of the C ABI without a GPU: bp_circuit_load_wires, bp_circuit_export_columns, bp_circuit_assign_device and
bp_prove_assignment (and the stage times of the first) are declared, bound, exported and refuse bad arguments with BP_ERR_INVALID_ARG
before they touch a device or an output.  The same refusals on a live context: tests/test_gpu_circuit_wires.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import baby_plonk_rust_amd as bp
from baby_plonk_rust_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bp_circuit_load_wires", "bp_circuit_load_wires_last_stats", "bp_circuit_export_columns", "bp_circuit_assign_device", "bp_prove_assignment"]
SENTINEL = 0xA5A5A5A5A5A5A5A5


def test_header_binding_table_rust_block_and_export_list_agree():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bp_msm_ntt.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "include", "bp_msm_ntt.rs")).read()
    listing = subprocess.run(["nm", "-D", "--defined-only", _lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in listing.splitlines() if line.strip()}
    lib = bp.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and "pub fn %s(" % name in rust and name in exported, name
        assert hasattr(lib, name)
    # the argument lists the issue states, as the binding table counts them
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [8, 2, 4, 10, 9]
    assert "selectors: *mut *const c_void, wire_ids: *const u32, n_public: usize" in rust
    assert open(os.path.join(ROOT, "baby_plonk_rust_amd", "csrc", "exports.map")).read().split() == "{ global: bp_*; bpx_*; local: *; };".split()


def test_bad_arguments_are_refused_without_a_context_and_outputs_stay_untouched():
    lib = bp.load()
    n = 8
    sel = [np.zeros((n, 4), dtype=np.uint64) for _ in range(5)]
    sel_ptrs = (C.c_void_p * 5)(*[s.ctypes.data for s in sel])
    ids = np.zeros((n, 3), dtype=np.uint32)
    handle = C.c_uint64(SENTINEL)
    load = lambda ctx, log_n, s, w, n_pub, fmt, h: lib.bp_circuit_load_wires(ctx, log_n, s, w, n_pub, fmt, 0, h)
    good = (None, 3, sel_ptrs, ids.ctypes.data, 0, bp.FR_MONT, C.byref(handle))
    for k, bad in ((0, None), (1, 2), (1, 25), (2, None), (3, None), (4, n + 1), (5, 7), (6, None)):
        args = list(good)
        args[k] = bad
        assert load(*args) == -1, k                                  # NULL context in every call: nothing else is ever reached
        assert handle.value == SENTINEL
    assert lib.bp_circuit_load_wires_last_stats(None, None) == -1
    cols = [np.full((n, 4), SENTINEL, dtype=np.uint64) for _ in range(8)]
    col_ptrs = (C.c_void_p * 8)(*[c.ctypes.data for c in cols])
    assert lib.bp_circuit_export_columns(None, 1, bp.FR_MONT, col_ptrs) == -1
    assert lib.bp_circuit_export_columns(None, 1, 7, col_ptrs) == -1 and lib.bp_circuit_export_columns(None, 1, bp.FR_MONT, None) == -1
    assert all((c == SENTINEL).all() for c in cols)
    values = np.zeros((4, 4), dtype=np.uint64)
    assert lib.bp_circuit_assign_device(None, 1, values.ctypes.data, 4, bp.FR_MONT, 0, None, None, None, None) == -1
    assert lib.bp_circuit_assign_device(None, 1, None, 4, bp.FR_MONT, 0, 8, 8, 8, None) == -1
    assert lib.bp_circuit_assign_device(None, 1, values.ctypes.data, 4, 7, 0, 8, 8, 8, None) == -1
    blinders = np.zeros(352, dtype=np.uint8)
    proof = np.full(624, 0xA5, dtype=np.uint8)
    for args in ((None, 1, 1, values.ctypes.data, 4, bp.FR_MONT, 0, blinders.ctypes.data, proof.ctypes.data),
                 (None, 1, 1, None, 4, bp.FR_MONT, 0, blinders.ctypes.data, proof.ctypes.data),
                 (None, 1, 1, values.ctypes.data, 4, 7, 0, blinders.ctypes.data, proof.ctypes.data),
                 (None, 1, 1, values.ctypes.data, 4, bp.FR_MONT, 0, None, proof.ctypes.data),
                 (None, 1, 1, values.ctypes.data, 4, bp.FR_MONT, 0, blinders.ctypes.data, None)):
        assert lib.bp_prove_assignment(*args) == -1
    assert (proof == 0xA5).all()

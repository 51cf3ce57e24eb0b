"""bp_verify_reduce_segments at the C boundary without a GPU: the symbol is exported, the Rust declarations carry it, and the argument
checks that need no device answer BP_ERR_INVALID_ARG (-1) instead of touching one."""
import ctypes as C
import os
import re

import numpy as np

import baby_plonk_rust_amd as bp
from baby_plonk_rust_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_and_declared_for_rust():
    lib = bp.load()
    rs = open(os.path.join(ROOT, "include", "bp_msm_ntt.rs")).read()
    header = open(os.path.join(ROOT, "include", "bp_msm_ntt.h")).read()
    for name in ("bp_verify_reduce_segments", "bp_verify_segments_last_stats"):
        assert getattr(lib, name) is not None and name in _lib.SIGNATURES
        assert re.search(r"\bint\s+%s\(" % name, header)
        assert re.search(r"pub fn %s\(" % name, rs), name
    decl = rs[rs.index("pub fn bp_verify_reduce_segments("):]
    decl = decl[:decl.index(";")]
    assert "segment: usize" in decl and "first_bad: *mut usize" in decl and decl.rstrip().endswith("-> c_int")
    # one more argument than bp_verify_reduce, in front of the output
    assert len(_lib.SIGNATURES["bp_verify_reduce_segments"][1]) == len(_lib.SIGNATURES["bp_verify_reduce"][1]) + 1


def test_null_context_and_null_arguments_are_invalid_without_a_device():
    lib = bp.load()
    vk, rec, out = np.zeros(768, dtype=np.uint8), np.zeros(624, dtype=np.uint8), np.full(192, 0xA5, dtype=np.uint8)
    bad = C.c_size_t(7)
    assert lib.bp_verify_reduce_segments(None, 3, vk.ctypes.data, rec.ctypes.data, 1, None, 0, None, None, 0, 1, out.ctypes.data, C.byref(bad)) == -1
    assert lib.bp_verify_reduce_segments(None, 3, None, None, 0, None, 0, None, None, 0, 1, None, None) == -1
    assert (out == 0xA5).all() and bad.value == 7
    ms = (C.c_float * 3)()
    assert lib.bp_verify_segments_last_stats(None, ms) == -1

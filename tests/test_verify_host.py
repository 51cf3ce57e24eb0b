"""CPU checks of the batch-verification boundary (bp_plonk_challenges, bp_verify_reduce, bp_verify_last_stats), no GPU: the
fixed-schedule transcript of csrc/verify_kernels.hpp -- the lines the device kernel runs, compiled for the host -- against the
Python twin of merlin (tests/merlin_transcript.py), on inputs that exercise the rejection sampling of transcript.rs:70-82, and
the argument checks of the three entry points."""
import ctypes as C
import json
import os
import random

import numpy as np

import baby_plonk_rust_amd as bp
from baby_plonk_rust_amd import FR_BYTES_LE, FR_MONT
from tests import verify_model as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = V.Q
SIZE_MAX = 2**64 - 1


def random_records(count=64, seed=0x7E51F1):
    """per record: nine times randbytes(48), then six times randrange(Q)"""
    rnd = random.Random(seed)
    recs = []
    for _ in range(count):
        pts = b"".join(rnd.randbytes(48) for _ in range(9))
        recs.append(pts + V.le32([rnd.randrange(Q) for _ in range(6)]))
    return recs


def toy_record():
    return bytes.fromhex(json.load(open(os.path.join(ROOT, "tests", "golden", "path_vectors.json")))["toy_proof"]["proof624"])


def test_challenges_equal_the_python_transcript_including_long_rejection_runs():
    recs = [toy_record()] + random_records()
    want, draws = [], []
    for r in recs:
        ch, d = V.challenges_of(r)
        want.append(ch)
        draws += d
    # the inputs must reach deep into the rejection loop, or that path would go untested without anyone noticing
    assert len(draws) == 6 * 65 and max(draws) >= 8 and sum(1 for d in draws[6:] if d >= 4) >= 20, (max(draws), sorted(draws)[-10:])
    got_le = bp.plonk_challenges(recs, fmt=FR_BYTES_LE)
    assert got_le.shape == (65, 6, 32)
    assert [[int.from_bytes(got_le[j, k].tobytes(), "little") for k in range(6)] for j in range(65)] == want
    got_mont = bp.plonk_challenges(b"".join(recs), fmt=FR_MONT)
    assert got_mont.shape == (65, 6, 4)
    assert [bp.scalars_to_ints(got_mont[j]) for j in range(65)] == want
    assert all(0 < v < Q for row in want for v in row)


def test_challenges_reject_bad_arguments_and_non_canonical_evaluations():
    lib = bp.load()
    recs = random_records(5, seed=7)
    buf = np.frombuffer(b"".join(recs), dtype=np.uint8).copy()
    out, bad = np.zeros((5, 6, 32), dtype=np.uint8), C.c_size_t(7)
    assert lib.bp_plonk_challenges(buf.ctypes.data, 5, FR_BYTES_LE, out.ctypes.data, C.byref(bad)) == 0 and bad.value == SIZE_MAX
    assert lib.bp_plonk_challenges(buf.ctypes.data, 5, FR_BYTES_LE, out.ctypes.data, None) == 0
    assert lib.bp_plonk_challenges(None, 5, FR_BYTES_LE, out.ctypes.data, C.byref(bad)) == -1
    assert lib.bp_plonk_challenges(buf.ctypes.data, 5, FR_BYTES_LE, None, C.byref(bad)) == -1
    assert lib.bp_plonk_challenges(buf.ctypes.data, 5, 2, out.ctypes.data, C.byref(bad)) == -1
    bad.value = 7
    assert lib.bp_plonk_challenges(None, 0, FR_MONT, None, C.byref(bad)) == 0 and bad.value == SIZE_MAX       # m = 0
    assert bp.plonk_challenges(b"").shape == (0, 6, 4)
    for rec, field, value in ((3, 0, Q), (1, 5, Q + 1), (4, 2, 2**256 - 1)):
        t = bytearray(buf.tobytes())
        t[624 * rec + 432 + 32 * field: 624 * rec + 464 + 32 * field] = value.to_bytes(32, "little")
        tb = np.frombuffer(bytes(t), dtype=np.uint8).copy()
        assert lib.bp_plonk_challenges(tb.ctypes.data, 5, FR_BYTES_LE, out.ctypes.data, C.byref(bad)) == -4 and bad.value == rec
        try:
            bp.plonk_challenges(bytes(t))
            raise AssertionError("accepted an evaluation >= q")
        except bp.BpError as e:
            assert e.code == -4 and e.index == rec
    # two bad records: the lower one is reported
    t = bytearray(buf.tobytes())
    for rec in (4, 2):
        t[624 * rec + 432: 624 * rec + 464] = Q.to_bytes(32, "little")
    tb = np.frombuffer(bytes(t), dtype=np.uint8).copy()
    assert lib.bp_plonk_challenges(tb.ctypes.data, 5, FR_MONT, out.ctypes.data, C.byref(bad)) == -4 and bad.value == 2


def test_verify_entry_points_need_a_context():
    lib = bp.load()
    vk, rec, out, bad = np.zeros(768, dtype=np.uint8), np.zeros(624, dtype=np.uint8), np.zeros(192, dtype=np.uint8), C.c_size_t(7)
    assert lib.bp_verify_reduce(None, 3, vk.ctypes.data, rec.ctypes.data, 1, None, 0, None, None, FR_MONT, out.ctypes.data, C.byref(bad)) == -1
    assert lib.bp_verify_reduce(None, 3, vk.ctypes.data, None, 0, None, 0, None, None, FR_MONT, out.ctypes.data, None) == -1
    assert not out.any()
    ms = (C.c_float * 5)()
    assert lib.bp_verify_last_stats(None, ms) == -1


def test_model_closed_form_and_definition_agree_on_and_off_the_roots():
    """the model the GPU tests compare against: L_1 and PI by the definition == the closed form / the indicator on a root"""
    rnd = random.Random(5)
    for n in (8, 64):
        om = V.M.omega(n)
        public = [rnd.randrange(Q) for _ in range(3)]
        for zeta in (1, pow(om, 2, Q), pow(om, 5, Q), rnd.randrange(Q)):
            l1, pi = V.l1_and_pi(n, zeta, public)
            if zeta == 1:
                assert (l1, pi) == (1, (-public[0]) % Q)
            elif zeta == pow(om, 2, Q):
                assert (l1, pi) == (0, (-public[2]) % Q)
            elif zeta == pow(om, 5, Q):
                assert (l1, pi) == (0, 0)

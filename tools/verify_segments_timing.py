#!/usr/bin/env python3
"""Per-segment batch verification (bp_verify_reduce_segments) on one MI355X, end to end from pageable host memory, on the 2^10-row
circuit of tools/verify_batch_timing.py (--distinct proofs by bp_prove, tiled to m records, a random 128-bit weight each).

  1. m = 2^12, segment = 1 against the only way the library had to obtain the same 2^12 pairs: 2^12 calls of bp_verify_reduce with
     one proof each, timed in the same run.  The pairs of both are compared byte for byte.  Fails below --min-ratio (10).
  2. m = 2^16: segment = 1, 2^8 and m next to bp_verify_reduce on the same batch, with the five stage times and the split of the
     last stage (multiplications | sums | normalisation and encoding).  segment = m may not exceed segment = 1 by more than 25 %:
     both do the same 11 m products and differ in the depth of the reduction only.
  3. with the experiment build (BABY_PLONK_LIBRARY=exp) and --ab, instead of 1 and 2: the multiplication kernel in its plain 255-step form against
     the endomorphism form, m = 2^14, segment = 1 (docs/EXPERIMENTS.md).

Every timed result is checked with the known tau before its number is printed (tau A == B is the pairing equation): the host sum
of all pairs of a call, and a sample of single pairs.  One JSON line per measurement; --out writes them as one document.

  python tools/verify_segments_timing.py [--loop-log 12] [--big-log 16] [--distinct 64] [--reps 3] [--ab] [--out profiles/verify_segments_timing.json]"""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import baby_plonk_rust_amd as bp  # noqa: E402
from baby_plonk_rust_amd import FR_BYTES_LE  # noqa: E402
from tests import bigint_model as M  # noqa: E402
from tests import prover_rounds as PR  # noqa: E402
from tests import verify_model as V  # noqa: E402

Q = M.Q
TAU = 0x1234567


def dec96(b):
    return None if b[0] & 0x40 else (int.from_bytes(b[:48], "big"), int.from_bytes(b[48:], "big"))


def accepted(a96, b96):
    A, B = dec96(a96), dec96(b96)
    return A is not None and M.ec_mul(TAU, A) == B


def check_pairs(raw, n_seg, rnd, what):
    """the sum of all pairs and a sample of single ones satisfy tau A == B"""
    part = [b"".join(bp.bytes96_to_partial(raw[192 * s + 96 * i: 192 * s + 96 * i + 96]) for s in range(n_seg)) for i in (0, 1)]
    assert accepted(bp.sum_partials(part[0]), bp.sum_partials(part[1])), "%s: the sum of the pairs was not accepted" % what
    for s in sorted({0, n_seg - 1} | {rnd.randrange(n_seg) for _ in range(6)}):
        assert accepted(raw[192 * s: 192 * s + 96], raw[192 * s + 96: 192 * s + 192]), "%s: pair %d was not accepted" % (what, s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop-log", type=int, default=12)
    ap.add_argument("--big-log", type=int, default=16)
    ap.add_argument("--ab-log", type=int, default=14)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--min-ratio", type=float, default=10.0)
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    n, log_n = 1024, 10
    ctx = bp.Context(0)
    lib = ctx._lib
    pk, witness = V.public_circuit(n, 1000)
    setup = bp.Setup.generate_srs(n + 6, TAU, ctx)
    circuit = bp.Circuit({k: PR.SV(v) for k, v in pk.items()}, ctx)
    prover, verifier, rnd = bp.Prover(setup, circuit), bp.Verifier(setup, circuit), random.Random(0x5E6715)
    proofs, publics = [], []
    for _ in range(args.distinct):
        cols, public, column = witness(rnd)
        proofs.append(prover.prove_with_blinding(PR.SV(cols[0]), PR.SV(cols[1]), PR.SV(cols[2]), PR.SV(column), [rnd.randrange(1, Q) for _ in range(11)]))
        publics.append(public)
    vk = np.frombuffer(verifier.vk, dtype=np.uint8).copy()
    doc = {"circuit": "2^10 rows: 3 public inputs + 1000 chained multiplications", "distinct_proofs": args.distinct, "reps": args.reps, "rows": []}

    def emit(row):
        doc["rows"].append(row)
        print(json.dumps(row), flush=True)

    def inputs(m):
        idx = [j % args.distinct for j in range(m)]
        rec = np.frombuffer(b"".join(proofs[j] for j in idx), dtype=np.uint8).copy()                   # pageable host memory
        pub = np.frombuffer(V.le32([x for j in idx for x in publics[j]]), dtype=np.uint8).copy()
        w = np.frombuffer(V.le32([rnd.getrandbits(128) for _ in range(m)]), dtype=np.uint8).copy()
        return rec, pub, w

    def segments(rec, pub, w, m, segment, what):
        n_seg = -(-m // segment)
        out, bad = np.zeros(192 * n_seg, dtype=np.uint8), C.c_size_t()

        def run():
            ctx.check(lib.bp_verify_reduce_segments(ctx._h, log_n, vk.ctypes.data, rec.ctypes.data, m, pub.ctypes.data, 3, w.ctypes.data, None, FR_BYTES_LE,
                                                    segment, out.ctypes.data, C.byref(bad)), "bp_verify_reduce_segments")
        run()                                                   # warm-up: the workspaces grow here
        best, stats = None, None
        for _ in range(args.reps):
            out[:] = 0
            t0 = time.perf_counter()
            run()
            dt = time.perf_counter() - t0
            if best is None or dt < best:
                best, stats = dt, (ctx.verify_stats(), ctx.verify_segments_stats())
        check_pairs(out.tobytes(), n_seg, rnd, what)            # checked before any number is printed
        return best, stats, out.tobytes()

    if not args.ab:
        # ---- 1. one call with segment = 1 against a loop of single-proof calls
        m = 1 << args.loop_log
        rec, pub, w = inputs(m)
        seg_s, (stages, split), seg_raw = segments(rec, pub, w, m, 1, "segment 1 at m = 2^%d" % args.loop_log)
        one, bad = np.zeros(192, dtype=np.uint8), C.c_size_t()
        loop_raw = bytearray()
        lib.bp_verify_reduce(ctx._h, log_n, vk.ctypes.data, rec.ctypes.data, 1, pub.ctypes.data, 3, w.ctypes.data, None, FR_BYTES_LE, one.ctypes.data, C.byref(bad))
        t0 = time.perf_counter()
        for j in range(m):
            ctx.check(lib.bp_verify_reduce(ctx._h, log_n, vk.ctypes.data, rec.ctypes.data + 624 * j, 1, pub.ctypes.data + 96 * j, 3, w.ctypes.data + 32 * j, None,
                                           FR_BYTES_LE, one.ctypes.data, C.byref(bad)), "bp_verify_reduce")
            loop_raw += one.tobytes()
        loop_s = time.perf_counter() - t0
        assert bytes(loop_raw) == seg_raw, "the loop of single-proof calls and the segments call differ"
        ratio = loop_s / seg_s
        emit({"what": "segment=1 against a loop of single-proof bp_verify_reduce calls", "m": m, "segments_call_ms": seg_s * 1e3, "loop_ms": loop_s * 1e3,
              "loop_ms_per_proof": loop_s * 1e3 / m, "ratio": ratio, "stages_ms": stages, "last_stage_split_ms": split, "pairs_equal_byte_for_byte": True})

        # ---- 2. the large batch: three segment lengths next to bp_verify_reduce
        m = 1 << args.big_log
        rec, pub, w = inputs(m)
        times = {}
        for segment in (1, 1 << (args.big_log // 2), m):
            dt, (stages, split), _ = segments(rec, pub, w, m, segment, "segment %d at m = 2^%d" % (segment, args.big_log))
            times[segment] = dt
            emit({"what": "bp_verify_reduce_segments", "m": m, "segment": segment, "wall_ms": dt * 1e3, "proofs_per_s": m / dt, "stages_ms": stages,
                  "last_stage_split_ms": split})
        out = np.zeros(192, dtype=np.uint8)

        def reduce_run():
            ctx.check(lib.bp_verify_reduce(ctx._h, log_n, vk.ctypes.data, rec.ctypes.data, m, pub.ctypes.data, 3, w.ctypes.data, None, FR_BYTES_LE,
                                           out.ctypes.data, C.byref(bad)), "bp_verify_reduce")
        reduce_run()
        best = None
        for _ in range(args.reps):
            t0 = time.perf_counter()
            reduce_run()
            dt = time.perf_counter() - t0
            best = dt if best is None or dt < best else best
        assert accepted(out[:96].tobytes(), out[96:].tobytes())
        emit({"what": "bp_verify_reduce", "m": m, "wall_ms": best * 1e3, "stages_ms": ctx.verify_stats(), "segment_1_over_reduce": times[1] / best,
              "segment_m_over_segment_1": times[m] / times[1]})

    # ---- 3. plain against split multiplication (experiment build only)
    if args.ab:
        assert bp._lib.EXPERIMENT, "--ab needs the experiment build: BABY_PLONK_LIBRARY=exp"
        m = 1 << args.ab_log
        rec, pub, w = inputs(m)
        ab = {}
        for name, value in (("split", "0"), ("plain", "1")):
            os.environ["BP_VERIFY_SEG_PLAIN"] = value
            dt, (stages, split), raw = segments(rec, pub, w, m, 1, "%s form at m = 2^%d" % (name, args.ab_log))
            ab[name] = {"wall_ms": dt * 1e3, "mul_ms": split["mul_ms"], "raw": raw}
        os.environ["BP_VERIFY_SEG_PLAIN"] = "0"
        assert ab["split"].pop("raw") == ab["plain"].pop("raw"), "the two forms of the multiplication differ"
        emit({"what": "multiplication kernel: 255-step double-and-add against the x^2 split", "m": m, "segment": 1, "terms": 20 * m, "split": ab["split"],
              "plain": ab["plain"], "plain_over_split_mul": ab["plain"]["mul_ms"] / ab["split"]["mul_ms"]})

    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    if args.ab:
        return
    assert ratio >= args.min_ratio, "segment = 1 is only %.1f x faster than the loop of single-proof calls" % ratio
    assert times[1 << args.big_log] <= 1.25 * times[1], "segment = m takes %.2f x segment = 1: a segment is being summed serially" % (times[1 << args.big_log] / times[1])


if __name__ == "__main__":
    main()

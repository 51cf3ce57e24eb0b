"""Wall time of getting an SRS into HBM from host bytes, per entry point, at 2^16, 2^20 and 2^24 points (one MI355X):
bp_srs_load (96-byte points), bp_srs_load_compressed48 unchecked and checked (48-byte records, pageable host memory),
bp_srs_check_subgroup alone, bp_srs_export_compressed48; plus the single-core CPU rate of the oracle's decoder.  Host clock around
calls that end in a synchronise, one warm-up call of each first, best of --reps.  Montgomery products per point are counted from the
exponent chain and the formulas (csrc/g1_check.hpp); rates over wall time here, over kernel time from a rocprofv3 run of this tool.
Last line: one JSON object.

  python tools/srs_load_timing.py [--sizes 16,20,24] [--reps 3] [--out profiles/r07_srs_load_timing.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import baby_plonk_rust_amd as bp  # noqa: E402
from baby_plonk_rust_amd import _lib  # noqa: E402
from oracle import oracle as O  # noqa: E402

# Montgomery products per point (csrc/g1_check.hpp)
PRODUCTS = {
    "decode48": 1 + 2 + 500 + 1,          # x to Montgomery, x^3, fp_sqrt (6 table + 378 squarings + 115 window products + 1 check), y out of Montgomery
    "subgroup": 2 * (63 * 8 + 5 * 12) + 4,  # two mul_by_x (63 doublings x 8 + 5 additions x 12), beta, beta x, two cross products
    "encode48": 2,                        # x, y out of Montgomery
}


def timed(fn, reps):
    fn()                                               # warm-up
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,20,24")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-sample", type=int, default=200)
    ap.add_argument("--out")
    args = ap.parse_args()
    ctx = bp.Context(0)
    lib = ctx._lib
    result = {"products_per_point": PRODUCTS, "sizes": {}}
    for lg in (int(s) for s in args.sizes.split(",")):
        n = 1 << lg
        hg = ctx.srs_generate_progression(n, 0x1F2E3D4C5B6A7988, 0x10203)
        p96, p48 = np.zeros(96 * n, dtype=np.uint8), np.zeros(48 * n, dtype=np.uint8)      # pageable host memory
        ctx.check(lib.bp_srs_export(ctx._h, hg, 0, n, p96.ctypes.data), "bp_srs_export")
        ctx.check(lib.bp_srs_export_compressed48(ctx._h, hg, 0, n, p48.ctypes.data), "bp_srs_export_compressed48")

        def load96():
            h = C.c_uint64()
            ctx.check(lib.bp_srs_load(ctx._h, p96.ctypes.data, n, C.byref(h)), "bp_srs_load")
            ctx.srs_free(h.value)

        def load48(checks):
            def run():
                h, bad = C.c_uint64(), C.c_size_t()
                ctx.check(lib.bp_srs_load_compressed48(ctx._h, p48.ctypes.data, n, checks, C.byref(h), C.byref(bad)), "bp_srs_load_compressed48")
                ctx.srs_free(h.value)
            return run

        def check():
            bad = C.c_size_t()
            ctx.check(lib.bp_srs_check_subgroup(ctx._h, hg, 0, n, C.byref(bad)), "bp_srs_check_subgroup")

        out48 = np.zeros(48 * n, dtype=np.uint8)

        def export48():
            ctx.check(lib.bp_srs_export_compressed48(ctx._h, hg, 0, n, out48.ctypes.data), "bp_srs_export_compressed48")

        row = {"load96_s": timed(load96, args.reps), "load48_unchecked_s": timed(load48(0), args.reps),
               "load48_checked_s": timed(load48(_lib.SRS_CHECK_SUBGROUP), args.reps), "check_subgroup_s": timed(check, args.reps),
               "export48_s": timed(export48, args.reps)}
        assert bytes(out48) == bytes(p48)
        row["subgroup_products_per_s_wall"] = PRODUCTS["subgroup"] * n / row["check_subgroup_s"]
        result["sizes"]["2^%d" % lg] = row
        print("2^%d: %s" % (lg, ", ".join("%s %.4f" % (k, v) if v < 1e6 else "%s %.3g" % (k, v) for k, v in row.items())), flush=True)
        ctx.srs_free(hg)
        del p96, p48, out48
    # the CPU decoder of the oracle (from_compressed_unchecked, no subgroup test), one core, ctypes overhead included
    rec = bytes(O.points_to_bytes96(O.points_progression(args.cpu_sample, 0x1F2E3D4C5B6A7988, 0x10203)))
    recs48 = []
    for i in range(args.cpu_sample):
        aff, ok = O.g1_from_uncompressed(rec[96 * i: 96 * i + 96])
        recs48.append(O.g1_to_compressed(aff))
    t0 = time.perf_counter()
    for r in recs48:
        assert O.g1_from_compressed(r)[1]
    dt = (time.perf_counter() - t0) / len(recs48)
    result["cpu_oracle_unchecked_decode_us_per_point"] = dt * 1e6
    result["cpu_oracle_unchecked_decode_2p24_s"] = dt * (1 << 24)
    print("CPU oracle g1_from_compressed (unchecked, 1 core): %.1f us/point -> %.0f s for 2^24 points" % (dt * 1e6, dt * (1 << 24)), flush=True)
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

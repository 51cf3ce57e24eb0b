"""Time of Setup.open_all (bp_kzg_open_all_device: all n proofs of one polynomial on its domain, csrc/kzg_open_all.hpp) at n = 2^12,
2^16 and 2^20 on one MI355X: the four stage times of a first call (which builds the table DFT_2n(S^)) and of a second call (the
table is there), the HIP-event time of every pass of the three transforms over G1, and -- for comparison -- the only route that
existed before: Setup.open, one MSM per point.  That route is timed at 64 sampled points of the same polynomial in the same
process; its median times n is an EXTRAPOLATION, labelled as one, and the ratio to it is the number this tool reports.

The polynomial is f_k = r^k + s^k (made on the device), so that every value and proof has a closed form of O(log n) Python-integer
operations for the known tau: f(x) = g(r x) + g(s x), g(y) = (y^n - 1) / (y - 1), proof_i = [(f(tau) - f(w^i)) / (tau - w^i)] G.
Before a time is recorded, 32 sampled proofs and values of that call's output are checked against it; the expected points come
from the CPU oracle (tests/kzg_model.py: point96), not from the library.
Which multiplication pass 0 of the Toeplitz transform used is recorded: g1_ntt_mul in the shipped library; with the experiment
library and BP_OPEN_ALL_MUL=split28 (BABY_PLONK_LIBRARY=exp) the g1_mul_split28 alternative, for the A/B of DESIGN.md 4.8.
Last line: one JSON object.

  python tools/kzg_open_all_timing.py [--sizes 12,16,20] [--points 64] [--out profiles/kzg_open_all_timing.json]"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import baby_plonk_rust_amd as bp  # noqa: E402
from baby_plonk_rust_amd import BASIS_MONOMIAL  # noqa: E402
from baby_plonk_rust_amd import _lib as _bp_lib  # noqa: E402
from tests import kzg_model as K  # noqa: E402  (point96: [k] G from the CPU oracle's G1, independent of the library)

Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
TAU = 0x1D0C5A3F9E8B7766554433221100FFEEDDCCBBAA99887766554433221100F1E2 % Q
R = 0x2F1E0D3C4B5A69788796A5B4C3D2E1F00112233445566778899AABBCCDDEEFF01 % Q
S = 0x0123456789ABCDEFFEDCBA98765432100F1E2D3C4B5A69788796A5B4C3D2E1F7 % Q


def omega(n):
    return pow(pow(7, (Q - 1) >> 32, Q), (1 << 32) // n, Q)


def f_at(x, n):
    """f(x) for f_k = r^k + s^k, k < n"""
    out = 0
    for base in (R, S):
        y = base * x % Q
        out += n if y == 1 else (pow(y, n, Q) - 1) * pow(y - 1, Q - 2, Q)
    return out % Q


def check_closed_form(ctx, ys, proofs, n):
    w, rnd, f_tau = omega(n), random.Random(n), f_at(TAU, n)
    for i in sorted({0, 1, 2, n // 2, n - 2, n - 1} | {rnd.randrange(n) for _ in range(26)}):
        z = pow(w, i, Q)
        y = f_at(z, n)
        assert bp.scalars_to_ints(ys[i:i + 1]) == [y], "value %d differs from the closed form" % i
        assert bytes(proofs[i]) == K.point96((f_tau - y) * pow((TAU - z) % Q, Q - 2, Q) % Q), "proof %d differs from the closed form" % i


def pass_times(ctx):
    """the pass times of the last call's transforms over G1, in the order they ran (ctx.hpp: g1_ntt_pass_ms)"""
    ms, k = (C.c_float * 96)(), C.c_uint32()
    fn = ctx._lib.bpx_srs_lagrange_pass_ms
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32)]
    ctx.check(fn(ctx._h, ms, 96, C.byref(k)), "bpx_srs_lagrange_pass_ms")
    return [float(ms[i]) for i in range(k.value)]


def one_call(ctx, setup, poly, n, lg, first):
    t0 = time.perf_counter()
    ys, proofs = setup.open_all(poly, n)
    wall = time.perf_counter() - t0
    stages, ms = ctx.kzg_open_all_stats(), pass_times(ctx)
    check_closed_form(ctx, ys, proofs, n)                                   # before anything is recorded
    assert len(ms) == (3 * lg + 2 if first else 2 * lg + 1), (len(ms), lg, first)
    assert (stages["table_ms"] > 0) == first
    if first:
        table, ms = ms[:lg + 1], ms[lg + 1:]
    row = {"wall_s": wall, "stage_ms": stages, "toeplitz_pass_ms": ms[:lg + 1], "final_pass_ms": ms[lg + 1:]}
    if first:
        row["table_pass_ms"] = table
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="12,16,20")
    ap.add_argument("--points", type=int, default=64)
    ap.add_argument("--out")
    args = ap.parse_args()
    ctx = bp.Context(0)
    result = {"tau": hex(TAU), "sizes": {}, "toeplitz_pass0_multiplication": "g1_mul_split28 (experiment build, BP_OPEN_ALL_MUL=split28)"
              if _bp_lib.EXPERIMENT and os.environ.get("BP_OPEN_ALL_MUL") == "split28" else "g1_ntt_mul",
              "reference": "no counterpart: the reference opens at zeta and zeta omega only", "parent_commit": "only the per-point route Setup.open"}
    for lg in (int(s) for s in args.sizes.split(",")):
        n = 1 << lg
        setup = bp.Setup.generate_srs(n, TAU, ctx)                           # with its fixed-base tables, as a user's Setup has them
        ones = bp.DevicePolynomial(np.tile(bp.scalar_from_int(1), (n, 1)), BASIS_MONOMIAL, ctx)
        poly = ones.scale_powers(bp.scalar_from_int(R)) + ones.scale_powers(bp.scalar_from_int(S))
        row = {"first_call": one_call(ctx, setup, poly, n, lg, True), "second_call": one_call(ctx, setup, poly, n, lg, False)}
        # the only earlier route: one Setup.open per point
        w, rnd, times = omega(n), random.Random(lg), []
        for i in [rnd.randrange(n) for _ in range(args.points)]:
            z = pow(w, i, Q)
            zs = bp.scalar_from_int(z)
            t0 = time.perf_counter()
            y, proof = setup.open(poly, zs)
            times.append(time.perf_counter() - t0)
            assert bp.scalars_to_ints(y) == [f_at(z, n)]
        med = statistics.median(times)
        row["per_point_route"] = {"points_timed": args.points, "median_open_s": med, "times_n_s_EXTRAPOLATED": med * n,
                                  "note": "n calls of Setup.open were not run: the median of %d calls times n" % args.points}
        row["ratio_extrapolated_per_point_route_to_second_call"] = med * n / row["second_call"]["wall_s"]
        row["ratio_extrapolated_per_point_route_to_first_call"] = med * n / row["first_call"]["wall_s"]
        result["sizes"]["2^%d" % lg] = row
        print("2^%d: first call %.3f s %s; second call %.3f s %s; Setup.open median %.3f ms x n = %.1f s (extrapolated): ratio %.1f" % (
            lg, row["first_call"]["wall_s"], {k: round(v, 2) for k, v in row["first_call"]["stage_ms"].items()}, row["second_call"]["wall_s"],
            {k: round(v, 2) for k, v in row["second_call"]["stage_ms"].items()}, med * 1e3, med * n,
            row["ratio_extrapolated_per_point_route_to_second_call"]), flush=True)
        ctx.srs_free(setup.handle)
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

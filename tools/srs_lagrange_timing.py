"""Time of bp_srs_lagrange (the inverse NTT over G1, csrc/g1_ntt.hpp) at 2^12, 2^16 and 2^20 points on one MI355X, with the HIP-event
time of every pass, and at 2^20 points the commitment of one evaluation-form column by both routes: i_ntt + commit on the powers-of-tau
SRS (the only route before bp_srs_lagrange existed) against commit on the Lagrange SRS, for a random column and for a 0/1 column.

Every Lagrange SRS is checked against the closed form for the known tau BEFORE its time is recorded: L_i = [L_i(tau)] G with
L_i(tau) = (tau^n - 1) omega^i / (n (tau - omega^i)) in Python integers -- a sample of exported points (first, last, random) point by
point, and the whole vector through one MSM with random scalars v against (sum_i v_i L_i(tau)) G.

Point operations per multiplication: 255 doublings + one addition per set bit of the scalar (the exact count for n^-1 in pass 0, 127.5
for a twiddle), + 2 additions per butterfly; the rate is those over the sum of the pass times.  --g1add runs tools/ubench_g1add (the
register-only rate of the MSM's 28-bit mixed addition on the same GPU) and records its additions/s beside them.
Last line: one JSON object.

  python tools/srs_lagrange_timing.py [--sizes 12,16,20] [--column-log 20] [--reps 3] [--g1add tools/ubench_g1add]
                                      [--out profiles/srs_lagrange_timing.json]"""
import argparse
import ctypes as C
import json
import os
import random
import re
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import baby_plonk_rust_amd as bp  # noqa: E402
from baby_plonk_rust_amd import BASIS_LAGRANGE  # noqa: E402

Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
TAU = 0x1D0C5A3F9E8B7766554433221100FFEEDDCCBBAA99887766554433221100F1E2 % Q


def omega(n):
    return pow(pow(7, (Q - 1) >> 32, Q), (1 << 32) // n, Q)


def lagrange_at_tau(n):
    """[L_i(tau)] for i < n, one batch inversion"""
    w, num = omega(n), (pow(TAU, n, Q) - 1) * pow(n, Q - 2, Q) % Q
    roots, den, prefix, acc = [], [], [], 1
    r = 1
    for _ in range(n):
        roots.append(r)
        d = (TAU - r) % Q
        den.append(d)
        acc = acc * d % Q
        prefix.append(acc)
        r = r * w % Q
    inv, out = pow(acc, Q - 2, Q), [0] * n
    for i in range(n - 1, -1, -1):
        d_inv = inv * (prefix[i - 1] if i else 1) % Q
        inv = inv * den[i] % Q
        out[i] = num * roots[i] % Q * d_inv % Q
    return out


def g_times(ctx, k):
    """k G as 96 bytes, through the library's own generator path (bp_srs_generate_progression with one point)"""
    h = ctx.srs_generate_progression(1, k % Q, 0)
    try:
        return ctx.srs_export(h)
    finally:
        ctx.srs_free(h)


def check_closed_form(ctx, lag, n):
    want = lagrange_at_tau(n)
    rnd = random.Random(n)
    for i in sorted({0, 1, 2, 3, n - 2, n - 1} | {rnd.randrange(n) for _ in range(26)}):
        if i < n:
            assert ctx.srs_export(lag, i, 1) == g_times(ctx, want[i]), "L_%d differs from the closed form" % i
    v = [rnd.randrange(Q) for _ in range(n)]
    got = ctx.msm(lag, np.frombuffer(b"".join(x.to_bytes(32, "little") for x in v), dtype=np.uint8).reshape(-1, 32), fmt=bp.FR_BYTES_LE)
    assert got == g_times(ctx, sum(a * b for a, b in zip(v, want)) % Q), "sum v_i L_i differs from the closed form"


def pass_times(ctx):
    ms, k = (C.c_float * 32)(), C.c_uint32()
    fn = ctx._lib.bpx_srs_lagrange_pass_ms
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32)]
    ctx.check(fn(ctx._h, ms, 32, C.byref(k)), "bpx_srs_lagrange_pass_ms")
    return [float(ms[i]) for i in range(k.value)]


def point_ops(log_n):
    n = 1 << log_n
    n_inv_bits = bin(pow(n, Q - 2, Q)).count("1")
    per_pass = [n * (255 + n_inv_bits) + n]                                  # pass 0: two scalings and two additions per butterfly
    for s in range(1, log_n):
        mults = n // 2 - (n >> (s + 1))                                      # the butterflies whose twiddle is not 1
        per_pass.append(mults * (255 + 127.5) + n)
    return per_pass


def timed(fn, reps):
    fn()
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="12,16,20")
    ap.add_argument("--column-log", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--g1add")
    ap.add_argument("--out")
    args = ap.parse_args()
    ctx = bp.Context(0)
    result = {"tau": hex(TAU), "sizes": {}, "parent_commit": "no counterpart: bp_srs_lagrange did not exist, so there is no earlier time to compare with"}
    if args.g1add:
        text = subprocess.run([args.g1add], capture_output=True, text=True, check=True, timeout=120).stdout
        rates = [float(x) for x in re.findall(r"g1_add_mixed28.*?([0-9.]+e[+-]?[0-9]+) additions/s", text)]
        result["ubench_g1add_mixed28_additions_per_s"] = max(rates)
        print("ubench_g1add: %.3e additions/s (register-only g1_add_mixed28, 28-bit limbs)" % max(rates), flush=True)
    for lg in (int(s) for s in args.sizes.split(",")):
        n = 1 << lg
        src = ctx.srs_generate(n, TAU)
        t0 = time.perf_counter()
        lag = ctx.srs_lagrange(src, lg)
        wall = time.perf_counter() - t0
        ms = pass_times(ctx)
        check_closed_form(ctx, lag, n)                                       # before anything is recorded
        ops = point_ops(lg)
        row = {"wall_s": wall, "pass_ms": ms, "passes_ms_total": sum(ms), "point_ops": sum(ops), "point_ops_per_s": sum(ops) / (sum(ms) * 1e-3),
               "point_ops_per_s_by_pass": [o / (t * 1e-3) for o, t in zip(ops, ms)]}
        if "ubench_g1add_mixed28_additions_per_s" in result:
            row["fraction_of_ubench_g1add"] = row["point_ops_per_s"] / result["ubench_g1add_mixed28_additions_per_s"]
        result["sizes"]["2^%d" % lg] = row
        print("2^%d: wall %.3f s, passes %.1f ms (%s), %.3e point ops/s" % (lg, wall, sum(ms), " ".join("%.1f" % t for t in ms), row["point_ops_per_s"]), flush=True)
        if lg == args.column_log:
            result["column_2^%d" % lg] = columns(ctx, src, lag, n, args.reps)
        ctx.srs_free(lag)
        ctx.srs_free(src)
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        open(args.out, "w").write(line + "\n")


def columns(ctx, src, lag, n, reps):
    """one device-resident evaluation-form column of n values: DevicePolynomial.i_ntt() (a copy and the transform) + commit on the
    powers of tau, against commit on the Lagrange SRS; both SRS with their automatic fixed-base tables, as a Setup builds them"""
    mono, lagr = bp.Setup(src, ctx, tables=True), bp.Setup(lag, ctx, tables=True)
    rnd = np.random.default_rng(20)
    out = {"tables": {"monomial": ctx.srs_table_info(src), "lagrange": ctx.srs_table_info(lag)}}
    for name, vals in (("random", [int.from_bytes(rnd.bytes(31), "little") for _ in range(n)]), ("bits", [int(b) for b in rnd.integers(0, 2, n)])):
        col = bp.DevicePolynomial(bp.scalars_from_ints(vals), BASIS_LAGRANGE, ctx)
        a, b = mono.commit_device(col.i_ntt()), lagr.commit_device(col)
        assert a == b, "the two routes disagree on the %s column" % name
        t_a = timed(lambda: mono.commit_device(col.i_ntt()), reps)
        t_b = timed(lambda: lagr.commit_device(col), reps)
        out[name] = {"i_ntt_then_commit_s": t_a, "commit_lagrange_s": t_b, "ratio": t_a / t_b}
        print("column %s at n = %d: i_ntt + commit %.3f ms, commit on the Lagrange SRS %.3f ms, ratio %.2f" % (name, n, t_a * 1e3, t_b * 1e3, t_a / t_b), flush=True)
    return out


if __name__ == "__main__":
    main()

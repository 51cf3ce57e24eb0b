"""Times of the SRS structure calls on one MI355X at 2^16 and 2^20 points (--sizes 16,20,24 where the sitting allows):
  - bp_srs_check_powers on a clean powers-of-tau SRS (one reduce, one host pairing check);
  - the same with ONE break in the middle (the price of the bisection: 1 + ceil(log2 (n - 1)) reduces and pairings);
  - bp_srs_adopt_lagrange of exported Lagrange points beside bp_srs_lagrange of the same size in the same run, and their ratio;
  - bp_srs_scale with s^i made on the device, split by HIP events into subgroup test | srs_scale kernel | normalisation, and the
    kernel's time per product beside verify_seg_mul's (the same multiplication; profiles/verify_segments_timing.json).
Method, as tools/srs_lagrange_timing.py: best of --reps (3) after one warm-up call, the host clock around the blocking call, stages by
HIP events.  The SRS carries the automatic fixed-base tables a Setup builds.  Every result is compared with its closed form for the
known tau BEFORE its time is recorded: the reduce against ((rho tau)^n - 1) / (rho tau - 1) G and tau times that, the verdicts against
the planted break, the adopted points against bp_srs_lagrange's and sampled L_i(tau) G, the scaled SRS against (tau s)^i G at
sampled indices and as a whole through check_powers with x_2 = tau s G2.  The checks have no counterpart in earlier commits:
absolute times only.  Last line: one JSON object.

  python tools/srs_structure_timing.py [--sizes 16,20] [--reps 3] [--out profiles/srs_structure_timing.json]"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import baby_plonk_rust_amd as bp  # noqa: E402

Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
TAU = 0x1D0C5A3F9E8B7766554433221100FFEEDDCCBBAA99887766554433221100F1E2 % Q
S = 0x2B992DDFA23249D6B5E5F7C1A3D4E6F8091A2B3C4D5E6F708192A3B4C5D6E7F8 % Q
RHO = (1 << 127) | 0x3C6EF372FE94F82BE54FF53A5F1D36F1


def omega(n):
    return pow(pow(7, (Q - 1) >> 32, Q), (1 << 32) // n, Q)


def g_times(ctx, k):
    """k G as 96 bytes, through the library's own generator path (bp_srs_generate_progression with one point)"""
    h = ctx.srs_generate_progression(1, k % Q, 0)
    try:
        return ctx.srs_export(h)
    finally:
        ctx.srs_free(h)


def timed(fn, reps):
    """best of reps after one warm-up; fn returns a closure's result, the last one is handed back with the time"""
    fn()
    best, last = None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        last = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, last


def sample(n, seed):
    rnd = random.Random(seed)
    return sorted({0, 1, n // 2, n - 1} | {rnd.randrange(n) for _ in range(12)})


def verify_seg_mul_ns():
    """ns per product of verify_seg_mul at scale, from the recorded profile: its largest batch reduced to one segment"""
    try:
        rows = json.load(open(os.path.join(ROOT, "profiles", "verify_segments_timing.json")))["rows"]
    except (OSError, ValueError, KeyError):
        return None
    rows = [r for r in rows if "last_stage_split_ms" in r and r.get("segment", 0) >= r["m"]]
    if not rows:
        return None
    r = max(rows, key=lambda r: r["m"])
    return r["last_stage_split_ms"]["mul_ms"] * 1e6 / (11 * r["m"] + 9)


def one_size(ctx, lg, reps):
    n = 1 << lg
    row = {}
    setup = bp.Setup.generate_srs(n, TAU, ctx, tables=True)
    src = setup.handle
    row["tables"] = ctx.srs_table_info(src)

    # ---- the reduce against its closed form, then the clean verdict
    rt = RHO * TAU % Q
    geo = (pow(rt, n - 1, Q) - 1) * pow(rt - 1, Q - 2, Q) % Q
    assert ctx.srs_powers_reduce(src, RHO) == (g_times(ctx, geo), g_times(ctx, geo * TAU)), "reduce differs from its closed form"
    t, verdict = timed(lambda: setup.check_powers(RHO), reps)
    assert verdict is None, "a clean SRS was refused at %r" % verdict
    st = ctx.srs_check_stats()
    assert (st["reduces"], st["pairings"]) == (1, 1)
    row["check_clean"] = {"wall_s": t, "reduces": 1, "pairings": 1}
    print("2^%d check_powers clean: %.2f ms" % (lg, t * 1e3), flush=True)

    # ---- one break in the middle: P_mid doubled (bp_srs_scale with every scalar 1 but one)
    mid = n // 2
    ks = np.tile(bp.scalar_from_int(1), (n, 1))
    ks[mid] = bp.scalar_from_int(2)
    broken = bp.Setup(ctx.srs_scale(src, ks), ctx, tables=True, x_2=setup.x_2)
    assert ctx.srs_export(broken.handle, mid, 1) == g_times(ctx, 2 * pow(TAU, mid, Q)) and ctx.srs_export(broken.handle, mid + 1, 1) == g_times(ctx, pow(TAU, mid + 1, Q))
    t, verdict = timed(lambda: broken.check_powers(RHO), reps)
    assert verdict == mid, "the break at %d was reported at %r" % (mid, verdict)
    st = ctx.srs_check_stats()
    assert st["reduces"] == st["pairings"] <= 2 + lg
    row["check_one_break"] = {"wall_s": t, "reduces": st["reduces"], "pairings": st["pairings"], "at": mid}
    print("2^%d check_powers, one break at %d: %.2f ms (%d reduces and pairings)" % (lg, mid, t * 1e3, st["reduces"]), flush=True)
    ctx.srs_free(broken.handle)

    # ---- adopt beside bp_srs_lagrange
    made = []
    t_lag, lag = timed(lambda: made.append(ctx.srs_lagrange(src, lg)) or made[-1], reps)
    for h in made[:-1]:
        ctx.srs_free(h)
    w, num = omega(n), (pow(TAU, n, Q) - 1) * pow(n, Q - 2, Q) % Q
    for i in sample(n, lg):
        wi = pow(w, i, Q)
        assert ctx.srs_export(lag, i, 1) == g_times(ctx, num * wi % Q * pow(TAU - wi, Q - 2, Q)), "L_%d differs from the closed form" % i
    points = ctx.srs_export(lag)
    loaded = ctx.srs_load(points)
    made = []
    t_adopt, adopted = timed(lambda: made.append(ctx.srs_adopt_lagrange(loaded, src, lg, RHO)) or made[-1], reps)
    for h in made[:-1]:
        ctx.srs_free(h)
    assert ctx.srs_basis(adopted) == (bp.BASIS_LAGRANGE, lg) and ctx.srs_export(adopted) == points, "the adopted SRS differs from bp_srs_lagrange's"
    row["lagrange"] = {"bp_srs_lagrange_wall_s": t_lag, "adopt_wall_s": t_adopt, "ratio": t_lag / t_adopt}
    print("2^%d bp_srs_lagrange %.2f ms, adopt_lagrange %.2f ms, ratio %.1f" % (lg, t_lag * 1e3, t_adopt * 1e3, t_lag / t_adopt), flush=True)
    for h in (lag, loaded, adopted):
        ctx.srs_free(h)

    # ---- a contribution: s^i on the device, bp_srs_scale
    import torch
    ones = bp.DevicePolynomial(np.tile(bp.scalar_from_int(1), (n, 1)), bp.BASIS_MONOMIAL, ctx)
    pows = ones.scale_powers(bp.scalar_from_int(S))
    torch.cuda.current_stream().synchronize()
    made, stages = [], []

    def scale_once():
        h = ctx.srs_scale(src, device_ptr=pows._ptr(), n=n)
        stages.append(ctx.srs_scale_stats())
        made.append(h)
        return h
    t_scale, scaled = timed(scale_once, reps)
    for h in made[:-1]:
        ctx.srs_free(h)
    ts = TAU * S % Q
    for i in sample(n, lg + 100):
        assert ctx.srs_export(scaled, i, 1) == g_times(ctx, pow(ts, i, Q)), "scaled point %d differs from (tau s)^i G" % i
    assert ctx.srs_check_powers(scaled, bp.g2_mul_generator(ts), RHO) is None, "the scaled SRS is not the powers of tau s"
    best = min(stages[1:], key=lambda s: s["scale_ms"])
    row["scale"] = {"wall_s": t_scale, "stages_ms": best, "ns_per_product": best["scale_ms"] * 1e6 / n}
    print("2^%d bp_srs_scale %.2f ms: subgroup %.2f, srs_scale %.2f (%.1f ns per product), normalise %.2f" %
          (lg, t_scale * 1e3, best["subgroup_ms"], best["scale_ms"], row["scale"]["ns_per_product"], best["normalise_ms"]), flush=True)
    ctx.srs_free(scaled)
    ctx.srs_free(src)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,20")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    ctx = bp.Context(0)
    result = {"tau": hex(TAU), "s": hex(S), "rho": hex(RHO), "reps": args.reps, "sizes": {},
              "method": "best of reps after one warm-up call; host clock around the blocking call; bp_srs_scale's stages by HIP events; "
                        "every result compared with its closed form before its time is recorded",
              "parent_commit": "no counterpart: these entry points did not exist, absolute times only",
              "verify_seg_mul_ns_per_product": verify_seg_mul_ns()}
    for lg in (int(s) for s in args.sizes.split(",")):
        result["sizes"]["2^%d" % lg] = one_size(ctx, lg, args.reps)
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

"""Time of a KZG opening (Setup.open: bp_kzg_open_device) on one MI355X, in both bases, for 1 and 7 polynomials at one point, with
the stage split of bp_kzg_last_stats -- and, in the same process, alternating with it after a warm-up, the composition of calls that
gave the same proof before Setup.open existed:
  Lagrange   i_ntt of every column + bp_poly_evaluate_device + the nu-combination + bp_poly_div_device by (x - z) + bp_commit_device
             on the powers-of-tau setup
  Monomial   the same without the transforms
Per configuration: the medians, the composition's spread against itself (max - min of its repetitions) and whether the new call's
median stays within composition median + spread.  The values-plus-quotient stage of the Lagrange form is reported beside
bp_ntt_fr_device(inverse) of ONE column of the same n.

Every timed result -- both routes -- is byte-compared with the closed form for the known tau (Python integers, one batched
inversion per point; [q(tau)] G through the library's generator path) BEFORE its time is printed.  Fails without a GPU.
Last line: one JSON object.

  python tools/kzg_open_timing.py [--sizes 16,20] [--counts 1,7] [--reps 5] [--out profiles/kzg_open_timing.json]
(2^24 is accepted by --sizes; its closed form costs minutes of Python integer work per configuration.)"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import baby_plonk_rust_amd as bp  # noqa: E402
from baby_plonk_rust_amd import BASIS_LAGRANGE, BASIS_MONOMIAL  # noqa: E402

Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
TAU = 0x1D0C5A3F9E8B7766554433221100FFEEDDCCBBAA99887766554433221100F1E2 % Q


def omega(n):
    return pow(pow(7, (Q - 1) >> 32, Q), (1 << 32) // n, Q)


def bary_weights(n, x):
    """c_i with f(x) = sum_i f_i c_i for evaluations over the n-th roots of unity (x off the domain): one batched inversion"""
    w, scale = omega(n), (pow(x, n, Q) - 1) * pow(n, Q - 2, Q) % Q
    roots, den, prefix, acc, r = [], [], [], 1, 1
    for _ in range(n):
        roots.append(r)
        d = (x - r) % Q
        den.append(d)
        acc = acc * d % Q
        prefix.append(acc)
        r = r * w % Q
    inv, out = pow(acc, Q - 2, Q), [0] * n
    for i in range(n - 1, -1, -1):
        out[i] = scale * roots[i] % Q * (inv * (prefix[i - 1] if i else 1) % Q) % Q
        inv = inv * den[i] % Q
    return out


def power_weights(n, x):
    out, p = [], 1
    for _ in range(n):
        out.append(p)
        p = p * x % Q
    return out


def dot(a, b):
    return sum(map(int.__mul__, a, b)) % Q


def g_times(ctx, k):
    """k G as 96 bytes, through the library's own generator path"""
    if k % Q == 0:
        return bytes([0x40]) + bytes(95)
    h = ctx.srs_generate_progression(1, k % Q, 0)
    try:
        return ctx.srs_export(h)
    finally:
        ctx.srs_free(h)


def closed_form(ctx, cols, basis, z, nu):
    """(ys, W96) of the columns opened at z: weights of the basis at z and at tau, then O(n) dot products"""
    n = len(cols[0])
    weights = bary_weights if basis == BASIS_LAGRANGE else power_weights
    at_z, at_tau = weights(n, z), weights(n, TAU)
    ys = [dot(c, at_z) for c in cols]
    y_g = sum(pow(nu, j, Q) * y for j, y in enumerate(ys)) % Q
    g_tau = sum(pow(nu, j, Q) * dot(c, at_tau) for j, c in enumerate(cols)) % Q
    return ys, g_times(ctx, (g_tau - y_g) * pow((TAU - z) % Q, Q - 2, Q) % Q)


def random_column(raw, n):
    """n random 248-bit values: as Python integers, and as Montgomery limbs through the host converter (bp_fr_convert)"""
    le = np.frombuffer(raw.bytes(32 * n), dtype=np.uint8).reshape(n, 32).copy()
    le[:, 31] = 0
    flat = le.tobytes()
    ints = [int.from_bytes(flat[32 * i: 32 * i + 32], "little") for i in range(n)]
    mont = np.zeros((n, 4), dtype=np.uint64)
    rc = bp.load().bp_fr_convert(le.ctypes.data, n, bp.FR_BYTES_LE, bp.FR_MONT, mont.ctypes.data)
    assert rc == 0, rc
    return ints, mont


def composition(mono, polys, z, nu):
    """what a caller wrote before Setup.open: coefficient forms, one evaluation each, the combination, the division, the commit"""
    ctx = mono.ctx
    coeffs = [p.i_ntt() if p.basis == BASIS_LAGRANGE else p for p in polys]
    ys = [c.coeffs_evaluate(z) for c in coeffs]
    g, p = coeffs[0], nu
    for c in coeffs[1:]:
        g = g + c * p
        p = bp.scalar_from_int(bp.scalar_to_int(p) * bp.scalar_to_int(nu))
    divisor = bp.DevicePolynomial(np.stack([bp.scalar_from_int(-bp.scalar_to_int(z)), bp.scalar_from_int(1)]), BASIS_MONOMIAL, ctx)
    return np.stack(ys), mono.commit_device(g / divisor)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,20")
    ap.add_argument("--counts", default="1,7")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    ctx = bp.Context(0)                                   # raises without a GPU
    import torch
    rng = random.Random(2024)
    result = {"tau": hex(TAU), "reps": args.reps, "sizes": {}}
    ok = True
    for lg in (int(s) for s in args.sizes.split(",")):
        n = 1 << lg
        mono = bp.Setup.generate_srs(n, TAU, ctx)
        lag = mono.lagrange(n)
        raw = np.random.default_rng(lg)
        scratch = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        ctx.ntt_device(scratch.data_ptr(), lg, inverse=True)
        ntt_ms = []
        for _ in range(args.reps):
            ctx.ntt_device(scratch.data_ptr(), lg, inverse=True)
            ntt_ms.append(ctx.ntt_stats()["device_ms"])
        row = {"ntt_inverse_device_ms": statistics.median(ntt_ms)}
        for count in (int(s) for s in args.counts.split(",")):
            pairs = [random_column(raw, n) for _ in range(count)]
            cols = [ints for ints, _ in pairs]
            z, nu = rng.randrange(Q), rng.randrange(Q)
            zl, nul = bp.scalar_from_int(z), bp.scalar_from_int(nu)
            for basis, setup, name in ((BASIS_LAGRANGE, lag, "lagrange"), (BASIS_MONOMIAL, mono, "monomial")):
                polys = [bp.DevicePolynomial(mont, basis, ctx) for _, mont in pairs]
                want_ys, want_w = closed_form(ctx, cols, basis, z, nu)
                new_s, comp_s, stages = [], [], []
                for rep in range(args.reps + 1):          # rep 0 is the warm-up of both routes
                    t0 = time.perf_counter()
                    ys, w = setup.open(polys, zl, nul)
                    t1 = time.perf_counter()
                    st = ctx.kzg_stats()
                    t2 = time.perf_counter()
                    cys, cw = composition(mono, polys, zl, nul)
                    t3 = time.perf_counter()
                    assert bp.scalars_to_ints(ys) == want_ys and w == want_w, "Setup.open differs from the closed form (%s, 2^%d, %d)" % (name, lg, count)
                    assert bp.scalars_to_ints(cys) == want_ys and cw == want_w, "the composition differs from the closed form (%s, 2^%d, %d)" % (name, lg, count)
                    if rep:
                        new_s.append(t1 - t0)
                        comp_s.append(t3 - t2)
                        stages.append(st)
                spread = max(comp_s) - min(comp_s)
                cell = {"open_median_ms": statistics.median(new_s) * 1e3, "composition_median_ms": statistics.median(comp_s) * 1e3,
                        "composition_spread_ms": spread * 1e3, "open_ms": [t * 1e3 for t in new_s], "composition_ms": [t * 1e3 for t in comp_s],
                        "values_quotient_ms": statistics.median(s["values_quotient_ms"] for s in stages),
                        "commit_ms": statistics.median(s["commit_ms"] for s in stages)}
                cell["within_spread"] = cell["open_median_ms"] <= cell["composition_median_ms"] + cell["composition_spread_ms"]
                ok = ok and cell["within_spread"]
                row["%s_x%d" % (name, count)] = cell
                print("2^%d %s x%d: open %.3f ms (values + quotient %.3f, commit %.3f), composition %.3f ms (spread %.3f)%s; inverse NTT of one column %.3f ms"
                      % (lg, name, count, cell["open_median_ms"], cell["values_quotient_ms"], cell["commit_ms"], cell["composition_median_ms"],
                         cell["composition_spread_ms"], "" if cell["within_spread"] else "  ABOVE THE COMPOSITION", row["ntt_inverse_device_ms"]), flush=True)
                del polys
        result["sizes"]["2^%d" % lg] = row
        ctx.srs_free(lag.handle)
        ctx.srs_free(mono.handle)
    result["every_open_within_spread"] = ok
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        open(args.out, "w").write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

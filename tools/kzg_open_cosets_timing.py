"""Time of Setup.open_cosets (bp_kzg_open_cosets_device: the n / l cell proofs of one polynomial, csrc/kzg_open_cosets.hpp) on one
MI355X at (log_n, log_l) = (12,6), (13,6), (16,6), (20,6): the four stage times of a first call (which builds the table) and of a later
call (the table is there) and the HIP-event time of every pass over G1, and -- in the same process -- the two routes to compare with:
  * Setup.open_all at the same n (a later call): the same 2n scalar multiplications, more butterfly passes;
  * the parent commit's only route per cell: divide by x^l - a_k on the host and commit once per cell.  Timed as the median of 64
    Setup.commit calls of n - l coefficients; that median times r = n / l is an EXTRAPOLATION, labelled as one.
Then Setup.verify_cells for m = 128 claims at (13,6): the reduce (bp_kzg_verify_cells_reduce) and the pairing check on the GPU.

The polynomial is f_i = R^i + S^i (made on the device), so that every value and proof has a closed form of O(log n) Python-integer
operations for the known tau: f(x) = g(R x, n) + g(S x, n) with g(y, k) = (y^k - 1) / (y - 1); the remainder of f by x^l - a is
I(x) = sum_base g(base^l a, r) g(base x, l), and proof k = [(f(tau) - I_k(tau)) / (tau^l - a_k)] G.  Before a time is recorded, 32
sampled cells of that call's output (every value, the proof) are checked against it; the expected points come from the CPU oracle
(tests/kzg_model.py: point96), not from the library.  Last line: one JSON object.

  python tools/kzg_open_cosets_timing.py [--sizes 12:6,13:6,16:6,20:6] [--commits 64] [--claims 128] [--out profiles/kzg_open_cosets_timing.json]"""
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
from tests import kzg_model as K  # noqa: E402  (point96: [k] G from the CPU oracle's G1, independent of the library)

Q = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
TAU = 0x1D0C5A3F9E8B7766554433221100FFEEDDCCBBAA99887766554433221100F1E2 % Q
R = 0x2F1E0D3C4B5A69788796A5B4C3D2E1F00112233445566778899AABBCCDDEEFF01 % Q
S = 0x0123456789ABCDEFFEDCBA98765432100F1E2D3C4B5A69788796A5B4C3D2E1F7 % Q


def omega(n):
    return pow(pow(7, (Q - 1) >> 32, Q), (1 << 32) // n, Q)


def geom(y, k):
    """1 + y + .. + y^(k-1)"""
    y %= Q
    return k % Q if y == 1 else (pow(y, k, Q) - 1) * pow(y - 1, Q - 2, Q) % Q


def f_at(x, n):
    return (geom(R * x, n) + geom(S * x, n)) % Q


def proof_scalar(n, l, k):
    """q_k(tau) for q_k = f div (x^l - a_k): (f(tau) - I_k(tau)) / (tau^l - a_k)"""
    a, r = pow(omega(n), k * l, Q), n // l
    rem = sum(geom(pow(base, l, Q) * a, r) * geom(base * TAU, l) for base in (R, S)) % Q
    return (f_at(TAU, n) - rem) * pow((pow(TAU, l, Q) - a) % Q, Q - 2, Q) % Q


def sampled_cells(n, l):
    r, rnd = n // l, random.Random(n + l)
    return sorted({0, 1, r // 2, r - 2, r - 1} | {rnd.randrange(r) for _ in range(27)})


def check_closed_form(cells, proofs, n, l):
    w, r = omega(n), n // l
    for k in sampled_cells(n, l):
        want = [f_at(pow(w, k + r * j, Q), n) for j in range(l)]
        assert bp.scalars_to_ints(cells[k]) == want, "the values of cell %d differ from the closed form" % k
        assert bytes(proofs[k]) == K.point96(proof_scalar(n, l, k)), "the proof of cell %d differs from the closed form" % k


def pass_times(ctx):
    """the pass times of the last call's passes over G1, in the order they ran (ctx.hpp: g1_ntt_pass_ms)"""
    ms, k = (C.c_float * 128)(), C.c_uint32()
    fn = ctx._lib.bpx_srs_lagrange_pass_ms
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32)]
    ctx.check(fn(ctx._h, ms, 128, C.byref(k)), "bpx_srs_lagrange_pass_ms")
    return [float(ms[i]) for i in range(k.value)]


def one_call(ctx, setup, poly, n, l, first):
    lg, ll = n.bit_length() - 1, l.bit_length() - 1
    lr = lg - ll
    t0 = time.perf_counter()
    cells, proofs = setup.open_cosets(poly, l, n)
    wall = time.perf_counter() - t0
    stages, ms = ctx.kzg_open_all_stats(), pass_times(ctx)
    check_closed_form(cells, proofs, n, l)                                   # before anything is recorded
    assert len(ms) == (lr + 1 if first else 0) + ll + (lr + 1) + lr, (len(ms), lg, ll, first)
    assert (stages["table_ms"] > 0) == first
    row = {"wall_s": wall, "stage_ms": stages}
    if first:
        row["table_pass_ms"], ms = ms[:lr + 1], ms[lr + 1:]
    row.update({"multiply_pass_ms": ms[0], "halve_pass_ms": ms[1:ll], "inverse_pass_ms": ms[ll:ll + lr + 1], "final_pass_ms": ms[ll + lr + 1:]})
    return row


def time_verify(ctx, setup, cells, proofs, n, l, m):
    com = K.point96(f_at(TAU, n))
    rnd = random.Random(m)
    claims = [bp.CellOpening(com, k, cells[k], bytes(proofs[k])) for k in (rnd.randrange(n // l) for _ in range(m))]
    weights = bp.scalars_from_ints([rnd.getrandbits(128) | 1 << 127 for _ in claims])
    tau_l_g2 = bp.g2_mul_generator(pow(TAU, l, Q))
    rows = []
    for _ in range(3):
        t0 = time.perf_counter()
        pair = setup.cell_pairing_inputs(claims, n, weights)
        t1 = time.perf_counter()
        ok = bp.pairing_check([pair], tau_l_g2, ctx=ctx)[0]
        t2 = time.perf_counter()
        assert ok is True
        rows.append({"reduce_wall_s": t1 - t0, "reduce_device_ms": ctx.kzg_stats()["reduce_ms"], "pairing_check_wall_s": t2 - t1})
    bad = list(claims)
    bad[5] = claims[5]._replace(index=(claims[5].index + 1) % (n // l))
    assert setup.verify_cells(bad, n, tau_l_g2, weights, host=False) is False
    return {"log_n": n.bit_length() - 1, "log_l": l.bit_length() - 1, "claims": m, "first_call": rows[0], "later_calls": rows[1:]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="12:6,13:6,16:6,20:6")
    ap.add_argument("--commits", type=int, default=64)
    ap.add_argument("--claims", type=int, default=128)
    ap.add_argument("--out")
    args = ap.parse_args()
    ctx = bp.Context(0)
    result = {"tau": hex(TAU), "sizes": {}, "reference": "no counterpart: the reference opens at zeta and zeta omega only",
              "parent_commit": "per cell: divide by x^l - a_k on the host, then one Setup.commit of n - l coefficients"}
    for lg, ll in (tuple(int(v) for v in s.split(":")) for s in args.sizes.split(",")):
        n, l = 1 << lg, 1 << ll
        r = n // l
        setup = bp.Setup.generate_srs(n, TAU, ctx)                           # with its fixed-base tables, as a user's Setup has them
        ones = bp.DevicePolynomial(np.tile(bp.scalar_from_int(1), (n, 1)), BASIS_MONOMIAL, ctx)
        poly = ones.scale_powers(bp.scalar_from_int(R)) + ones.scale_powers(bp.scalar_from_int(S))
        row = {"first_call": one_call(ctx, setup, poly, n, l, True), "later_calls": [one_call(ctx, setup, poly, n, l, False) for _ in range(2)]}
        later = min(c["wall_s"] for c in row["later_calls"])
        # open_all at the same n: the first call builds its table (and replaces the cells' one), the later one is the comparison
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            setup.open_all(poly, n)
            walls.append(time.perf_counter() - t0)
            stages = ctx.kzg_open_all_stats()
        row["open_all_same_n"] = {"first_call_wall_s": walls[0], "later_call_wall_s": min(walls[1:]), "later_call_stage_ms": stages}
        row["ratio_open_all_later_to_open_cosets_later"] = min(walls[1:]) / later
        # the parent commit's route per cell: one commit of n - l coefficients (the host division is not even counted)
        block = bp.scalars_from_ints([pow(R, i + 1, Q) for i in range(min(n - l, 4096))])       # full-width coefficients, tiled
        q = bp.Polynomial(np.ascontiguousarray(np.tile(block, ((n - l + 4095) // 4096, 1))[:n - l]), BASIS_MONOMIAL, ctx)
        times = []
        for _ in range(args.commits):
            t0 = time.perf_counter()
            setup.commit(q)
            times.append(time.perf_counter() - t0)
        med = statistics.median(times)
        row["per_cell_commit_route"] = {"commits_timed": args.commits, "median_commit_s": med, "times_r_s_EXTRAPOLATED": med * r,
                                        "note": "r commits were not run: the median of %d Setup.commit calls of n - l coefficients times r" % args.commits}
        row["ratio_extrapolated_commit_route_to_later_call"] = med * r / later
        if (lg, ll) == (13, 6):
            setup.open_cosets(poly, l, n)
            cells, proofs = setup.open_cosets(poly, l, n)
            result["verify_cells"] = time_verify(ctx, setup, cells, proofs, n, l, args.claims)
        result["sizes"]["2^%d / 2^%d" % (lg, ll)] = row
        print("n 2^%d l 2^%d: first %.3f s %s; later %.3f s %s; open_all later %.3f s; commit median %.3f ms x r = %.2f s (extrapolated)" % (
            lg, ll, row["first_call"]["wall_s"], {k: round(v, 2) for k, v in row["first_call"]["stage_ms"].items()}, later,
            {k: round(v, 2) for k, v in row["later_calls"][-1]["stage_ms"].items()}, min(walls[1:]), med * 1e3, med * r), flush=True)
        ctx.srs_free(setup.handle)
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

"""Time of a cell recovery (bp_kzg_recover_device, bp_kzg_recover_cells: csrc/kzg_recover.hpp) on one MI355X at l = 64 with half the
cells missing, n = 2^12, 2^13, 2^16, 2^20, n_coeffs = n / 2:
  * recover_polynomial_device alone: host wall time around the blocking call and its four HIP-event stage times
    (vanishing evaluations | spread + first inverse transform | coset division | check + output), a first call and later calls;
  * Setup.recover_cells end to end (host cells in, all cells and proofs out), a first call (builds the table of the cell proofs) and
    later calls;
  * in the same process, a later call of Setup.open_cosets at the same shape: what the second half of a recovery costs alone.
The ratio recovery / open_cosets is computed from the later calls' minima.

The polynomial is f_i = R^i + S^i, i < n / 2 (made on the device), so that every coefficient, value and proof has a closed form of
O(log n) Python-integer operations for the known tau (tools/kzg_open_cosets_timing.py has the formulas; here with n / 2 terms).  The
cells handed over are checked against the closed form at sampled places first; then, before a time is recorded, sampled coefficients
of every recover call (and sampled cells and proofs of every recover_cells and open_cosets call) are checked against it.  The expected
points come from the CPU oracle (tests/kzg_model.py: point96), not from the library.  Last line: one JSON object.

  python tools/kzg_recover_timing.py [--sizes 12:6,13:6,16:6,20:6] [--later 3] [--out profiles/kzg_recover_timing.json]"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import baby_plonk_rust_amd as bp  # noqa: E402
from baby_plonk_rust_amd import BASIS_MONOMIAL, _lib  # noqa: E402
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


def f_at(x, d):
    return (geom(R * x, d) + geom(S * x, d)) % Q


def proof_scalar(n, l, d, k):
    """q_k(tau) for q_k = f div (x^l - a_k), f of d coefficients (l divides d): (f(tau) - I_k(tau)) / (tau^l - a_k)"""
    a = pow(omega(n), k * l, Q)
    rem = sum(geom(pow(base, l, Q) * a, d // l) * geom(base * TAU, l) for base in (R, S)) % Q
    return (f_at(TAU, d) - rem) * pow((pow(TAU, l, Q) - a) % Q, Q - 2, Q) % Q


def sampled(count, seed, k=24):
    rnd = random.Random(seed)
    return sorted({0, 1, count // 2, count - 2, count - 1} | {rnd.randrange(count) for _ in range(k)})


def check_coefficients(values, d):
    """values: [d, 4] uint64 Montgomery limbs of the recovered polynomial"""
    assert len(values) == d
    for i in sampled(d, d):
        assert bp.scalar_to_int(values[i]) == (pow(R, i, Q) + pow(S, i, Q)) % Q, "coefficient %d differs from the known polynomial" % i


def check_cells(cells, proofs, n, l, d, which):
    w, r = omega(n), n // l
    for k in which:
        want = [f_at(pow(w, k + r * j, Q), d) for j in range(l)]
        assert bp.scalars_to_ints(cells[k]) == want, "the values of cell %d differ from the closed form" % k
        if proofs is not None:
            assert bytes(proofs[k]) == K.point96(proof_scalar(n, l, d, k)), "the proof of cell %d differs from the closed form" % k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="12:6,13:6,16:6,20:6")
    ap.add_argument("--later", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    ctx = bp.Context(0)
    dev = torch.device("cuda", ctx.device)
    result = {"tau": hex(TAU), "walk": _lib.KZG_RECOVER_WALK, "sizes": {},
              "reference": "no counterpart: the reference has no cells", "missing": "half the cells, drawn at random; indices shuffled"}
    for lg, ll in (tuple(int(v) for v in s.split(":")) for s in args.sizes.split(",")):
        n, l = 1 << lg, 1 << ll
        r, d = n // l, n // 2
        setup = bp.Setup.generate_srs(n, TAU, ctx, tables=False)             # no MSM runs here: the fixed-base tables would not be read
        ones = bp.DevicePolynomial(np.tile(bp.scalar_from_int(1), (d, 1)), BASIS_MONOMIAL, ctx)
        poly = ones.scale_powers(bp.scalar_from_int(R)) + ones.scale_powers(bp.scalar_from_int(S))
        # all cells, by one forward transform of the zero-padded coefficients; place k l + j holds natural index k + r j
        padded = torch.zeros((n, 4), dtype=torch.int64, device=dev)
        padded[:d] = poly.t
        torch.cuda.current_stream().synchronize()
        ctx.ntt_device(padded.data_ptr(), lg)
        all_cells = padded.view(l, r, 4).permute(1, 0, 2).contiguous()
        rnd = random.Random(lg)
        present = rnd.sample(range(r), r // 2)
        d_cells = all_cells[torch.tensor(present, device=dev)].contiguous()
        torch.cuda.current_stream().synchronize()
        h_cells = d_cells.cpu().numpy().view(np.uint64)
        check_cells(dict(zip(present, h_cells)), None, n, l, d, [present[i] for i in sampled(len(present), lg, 8)])      # the input itself
        row = {"n_coeffs": d, "cells_present": len(present), "cells_missing": r - len(present)}
        calls = []
        for _ in range(1 + args.later):
            t0 = time.perf_counter()
            got = bp.recover_polynomial_device(present, d_cells, l, n, d, ctx)
            wall = time.perf_counter() - t0
            stats = ctx.kzg_recover_stats()
            check_coefficients(got.values, d)                                # before anything is recorded
            calls.append({"wall_s": wall, "stage_ms": stats})
        row["recover_device"] = {"first_call": calls[0], "later_calls": calls[1:]}
        recover_later = min(c["wall_s"] for c in calls[1:])
        calls = []
        which = sampled(r, n, 8)
        for _ in range(1 + args.later):
            t0 = time.perf_counter()
            cells, proofs = setup.recover_cells(present, h_cells, n, d)
            wall = time.perf_counter() - t0
            check_cells(cells, proofs, n, l, d, which)
            calls.append({"wall_s": wall, "recover_stage_ms": ctx.kzg_recover_stats(), "proof_stage_ms": ctx.kzg_open_all_stats()})
        row["recover_cells"] = {"first_call": calls[0], "later_calls": calls[1:]}
        calls = []
        for _ in range(1 + args.later):                                      # the table is there: every one of these is a later call
            t0 = time.perf_counter()
            cells, proofs = setup.open_cosets(poly, l, n)
            wall = time.perf_counter() - t0
            check_cells(cells, proofs, n, l, d, which)
            calls.append({"wall_s": wall, "stage_ms": ctx.kzg_open_all_stats()})
        row["open_cosets_later_calls"] = calls
        cosets_later = min(c["wall_s"] for c in calls)
        row["ratio_recover_device_later_to_open_cosets_later"] = recover_later / cosets_later
        result["sizes"]["2^%d / 2^%d" % (lg, ll)] = row
        print("n 2^%d l 2^%d: recover_device later %.3f ms %s; recover_cells later %.3f ms; open_cosets later %.3f ms; ratio %.3f" % (
            lg, ll, recover_later * 1e3, {k: round(v, 3) for k, v in row["recover_device"]["later_calls"][-1]["stage_ms"].items()},
            min(c["wall_s"] for c in row["recover_cells"]["later_calls"]) * 1e3, cosets_later * 1e3,
            row["ratio_recover_device_later_to_open_cosets_later"]), flush=True)
        ctx.srs_free(setup.handle)
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

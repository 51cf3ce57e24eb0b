#!/usr/bin/env python3
"""Batch verification end to end (bp_verify_reduce) on one MI355X: proofs per second from pageable host memory and the five stage
times of bp_verify_last_stats, per batch size m, for a 2^10-row synthetic circuit with three public inputs (tests/verify_model.py
public_circuit: 1000 chained multiplications).  --distinct proofs are made by bp_prove (distinct witnesses and blinders) and
tiled to m records; every record gets its own random 128-bit weight.  A multiset of valid proofs is a valid batch, and the work
per record does not depend on its bytes (except the transcript's rejection draws, which the distinct proofs sample).
Every timed result is checked before its number is printed: with the known tau the pairing equation is tau A == B.
For comparison: the single-core CPU cost of the same reduction done proof by proof with the CPU oracle's point decoder and
scalar multiplications (20 per proof: 2 for A_j, 18 for B_j) at m = 2^6, checked against the GPU's bytes for those 64 proofs.
One JSON line per batch size; --out writes them all as one JSON document.

  python tools/verify_batch_timing.py [--sizes 0,10,14,16] [--distinct 256] [--reps 3] [--out profiles/verify_batch_timing.json]"""
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
STAGES = ("upload_ms", "transcript_ms", "scalars_ms", "decode_check_ms", "msm_ms")
# what the same kernels reach where they are used today (README: the 2^20-point MSM without tables)
DECODE_CHECK_S_PER_POINT = 0.495 / (1 << 24)
MSM_TABLE_FREE_S_PER_POINT = 3.34e-3 / (1 << 20)


def dec96(b):
    return None if b[0] & 0x40 else (int.from_bytes(b[:48], "big"), int.from_bytes(b[48:], "big"))


def accepted(out192):
    A, B = dec96(out192[:96]), dec96(out192[96:])
    return A is not None and M.ec_mul(TAU, A) == B


def cpu_reduce(vk, proofs, publics, weights):
    """Verifier::verify's group operations proof by proof on one core (the scalars come from tests/verify_model.py and are not timed)"""
    from oracle import oracle as O
    shared = [O.g1_from_affine(O.g1_from_uncompressed(vk[96 * k: 96 * k + 96])[0]) for k in range(8)] + [O.g1_generator()]
    coeff = []
    for proof, public, rho in zip(proofs, publics, weights):
        ev = [int.from_bytes(proof[432 + 32 * k: 464 + 32 * k], "little") for k in range(6)]
        p9, a2, s9 = V.coefficients(1024, ev, V.challenges_of(proof)[0], public, by_definition=False)
        coeff.append(([O.fr_from_int(c * rho % Q) for c in p9], [O.fr_from_int(c * rho % Q) for c in a2], [O.fr_from_int(c * rho % Q) for c in s9]))
    t0 = time.perf_counter()
    A, B = O.g1_identity(), O.g1_identity()
    for proof, (p9, a2, s9) in zip(proofs, coeff):
        pts = [O.g1_from_affine(O.g1_from_compressed(proof[48 * k: 48 * k + 48])[0]) for k in range(9)]
        for k in range(9):
            B = O.g1_add(B, O.g1_mul(pts[k], p9[k]))
            B = O.g1_add(B, O.g1_mul(shared[k], s9[k]))
        A = O.g1_add(A, O.g1_add(O.g1_mul(pts[7], a2[0]), O.g1_mul(pts[8], a2[1])))
    dt = time.perf_counter() - t0
    return dt, O.g1_bytes96(A) + O.g1_bytes96(B)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="0,10,14,16", help="log2 of the batch sizes")
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    n, log_n = 1024, 10
    ctx = bp.Context(0)
    lib = ctx._lib
    pk, witness = V.public_circuit(n, 1000)
    setup = bp.Setup.generate_srs(n + 6, TAU, ctx)
    circuit = bp.Circuit({k: PR.SV(v) for k, v in pk.items()}, ctx)
    prover, verifier, rnd = bp.Prover(setup, circuit), bp.Verifier(setup, circuit), random.Random(0x7E51F1)
    proofs, publics = [], []
    t0 = time.perf_counter()
    for _ in range(args.distinct):
        cols, public, column = witness(rnd)
        proofs.append(prover.prove_with_blinding(PR.SV(cols[0]), PR.SV(cols[1]), PR.SV(cols[2]), PR.SV(column), [rnd.randrange(1, Q) for _ in range(11)]))
        publics.append(public)
    prove_s = (time.perf_counter() - t0) / args.distinct
    vk = np.frombuffer(verifier.vk, dtype=np.uint8).copy()
    rows = []
    for lg in (int(s) for s in args.sizes.split(",")):
        m = 1 << lg
        idx = [j % args.distinct for j in range(m)]
        rec = np.frombuffer(b"".join(proofs[j] for j in idx), dtype=np.uint8).copy()                 # pageable host memory
        pub = np.frombuffer(V.le32([x for j in idx for x in publics[j]]), dtype=np.uint8).copy()
        w = np.frombuffer(V.le32([rnd.getrandbits(128) for _ in range(m)]), dtype=np.uint8).copy()
        out, bad = np.zeros(192, dtype=np.uint8), C.c_size_t()

        def run():
            ctx.check(lib.bp_verify_reduce(ctx._h, log_n, vk.ctypes.data, rec.ctypes.data, m, pub.ctypes.data, 3, w.ctypes.data, None, FR_BYTES_LE,
                                           out.ctypes.data, C.byref(bad)), "bp_verify_reduce")
        run()                                                   # warm-up: the workspaces grow here
        best, stats = None, None
        for _ in range(args.reps):
            out[:] = 0
            t0 = time.perf_counter()
            run()
            dt = time.perf_counter() - t0
            assert accepted(out.tobytes()), "the batch of m = 2^%d was not accepted" % lg            # checked before any number is printed
            if best is None or dt < best:
                best, stats = dt, ctx.verify_stats()
        row = {"m": m, "wall_ms": best * 1e3, "proofs_per_s": m / best, "stages_ms": stats, "points": 9 * m + 9,
               "decode_check_ms_at_the_srs_loaders_rate": DECODE_CHECK_S_PER_POINT * 9 * m * 1e3,
               "msm_ms_at_the_table_free_2p20_rate": MSM_TABLE_FREE_S_PER_POINT * (11 * m + 9) * 1e3,
               "dominant_stage": max(STAGES, key=lambda k: stats[k])}
        # a tampered batch of the same size must not be accepted (the check above is not vacuous)
        keep = rec[432]
        rec[432] ^= 1
        run()
        assert not accepted(out.tobytes()), "a tampered batch was accepted"
        rec[432] = keep
        rows.append(row)
        print(json.dumps(row), flush=True)
    m = 64
    weights = [rnd.getrandbits(128) for _ in range(m)]
    cpu_s, cpu_bytes = cpu_reduce(verifier.vk, proofs[:m], publics[:m], weights)
    pub64 = np.frombuffer(V.le32([x for j in range(m) for x in publics[j]]), dtype=np.uint8).reshape(m, 3, 32)
    gpu_sides = verifier.pairing_inputs(proofs[:m], pub64, np.frombuffer(V.le32(weights), dtype=np.uint8).reshape(m, 32), fmt=FR_BYTES_LE)
    assert gpu_sides[0] + gpu_sides[1] == cpu_bytes and accepted(cpu_bytes), "CPU and GPU reductions differ"
    cpu = {"cpu_single_core": {"m": m, "group_ops_s": cpu_s, "proofs_per_s": m / cpu_s, "what": "oracle g1_from_compressed + 20 g1_mul + 20 g1_add per proof, "
                                "scalars excluded, same bytes as the GPU for these 64 proofs"}}
    print(json.dumps(cpu), flush=True)
    doc = {"circuit": "2^10 rows: 3 public inputs + 1000 chained multiplications", "distinct_proofs": args.distinct, "bp_prove_s_per_proof": prove_s,
           "reps": args.reps, "rows": rows}
    doc.update(cpu)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

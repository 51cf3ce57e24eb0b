#!/usr/bin/env python3
"""Pairing checks on one MI355X against the host path of the same tree -> profiles/pairing_timing.json.

  1. For n in --sizes (1, 64, 2^10, 2^12, 2^14): the wall time and the three stage times of bp_pairing_check (a warm-up call first,
     then the best of --reps), beside bp_pairing_check_host on one core for the SAME n pairs (timed whole, once; sizes above
     --host-max are device only).  The pairs are the known-secret mix of tests/pairing_cases.py (tau = 7, fixture points) tiled to
     n; both results are compared with the known verdicts before a number is printed.
  2. For m = 2^12 proofs of the 2^10-row circuit of tools/verify_segments_timing.py (--distinct proofs by bp_prove, tiled to m, a
     random 128-bit weight each): Verifier.verify_each (segment = 1, then one check per GPU lane) against
     Verifier.locate_invalid(decide=None) (bisection over host pairings) for k bad proofs, k in --bad (0, 1, 2, 3, 4, 8, m/2).  A bad
     proof has one bit of an evaluation flipped.  Both answers must name exactly the tampered proofs, and the pairs of a sample of
     proofs are checked against the known tau (tau A == B iff the proof was left alone) before a number is printed.  The crossover
     is the smallest measured k at which the bisection takes longer than verify_each.

  python tools/pairing_timing.py [--sizes ...] [--host-max 16384] [--m-log 12] [--out profiles/pairing_timing.json]"""
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
from baby_plonk_rust_amd import FR_BYTES_LE  # noqa: E402
from tests import bigint_model as M  # noqa: E402
from tests import pairing_cases as PC  # noqa: E402
from tests import prover_rounds as PR  # noqa: E402
from tests import tower_model as T  # noqa: E402
from tests import verify_model as V  # noqa: E402

Q = M.Q
TAU = 0x1234567


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def dec96(b):
    return None if b[0] & 0x40 else (int.from_bytes(b[:48], "big"), int.from_bytes(b[48:], "big"))


def accepted(a96, b96):
    A, B = dec96(a96), dec96(b96)
    return A is not None and M.ec_mul(TAU, A) == B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,1024,4096,16384,32768,65536")
    ap.add_argument("--host-max", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--m-log", type=int, default=12)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--bad", default="0,1,2,3,4,8,half")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairing_timing.json"))
    a = ap.parse_args()
    doc = {"tool": "tools/pairing_timing.py", "host_cpu": cpu_model(), "host_threads": 1, "reps": a.reps, "check_sizes": [], "locate": []}
    ctx = bp.Context(0)

    # ---- 1. n pairs: device against host
    x2 = T.g2_enc192(T.g2_mul(PC.G2, PC.TAU))
    base, base_truth = PC.mixed_pairs(130, 1)
    for n in [int(v) for v in a.sizes.split(",")]:
        tiles = -(-n // 130)
        pairs, truth = (base * tiles)[:192 * n], (base_truth * tiles)[:n]
        assert ctx.pairing_check(pairs, x2) == truth              # warm-up: workspaces grow here; checked
        best, stats = None, None
        for _ in range(a.reps):
            t = time.perf_counter()
            got = ctx.pairing_check(pairs, x2)
            dt = (time.perf_counter() - t) * 1e3
            assert got == truth, "device verdicts differ from the known ones at n = %d" % n
            if best is None or dt < best:
                best, stats = dt, ctx.pairing_stats()
        row = {"n": n, "device_wall_ms": best, **stats, "host_wall_ms": None, "host_ms_per_pair": None}
        if n <= a.host_max:
            bp.pairing_check(pairs[:192], x2, host=True)          # the generator's lines are prepared once per process: not timed
            t = time.perf_counter()
            got = bp.pairing_check(pairs, x2, host=True)
            host_ms = (time.perf_counter() - t) * 1e3
            assert got == truth, "host verdicts differ from the known ones at n = %d" % n
            row.update(host_wall_ms=host_ms, host_ms_per_pair=host_ms / n, host_over_device=host_ms / best)
        doc["check_sizes"].append(row)
        print(json.dumps(row), flush=True)

    # ---- 2. m proofs: verify_each against bisection over host pairings
    n_rows, m = 1024, 1 << a.m_log
    pk, witness = V.public_circuit(n_rows, 1000)
    setup = bp.Setup.generate_srs(n_rows + 6, TAU, ctx)
    circuit = bp.Circuit({k: PR.SV(v) for k, v in pk.items()}, ctx)
    prover, verifier, rnd = bp.Prover(setup, circuit), bp.Verifier(setup, circuit), random.Random(0x5E6715)
    proofs, publics = [], []
    for _ in range(a.distinct):
        cols, public, column = witness(rnd)
        proofs.append(prover.prove_with_blinding(PR.SV(cols[0]), PR.SV(cols[1]), PR.SV(cols[2]), PR.SV(column), [rnd.randrange(1, Q) for _ in range(11)]))
        publics.append(public)
    idx = [j % a.distinct for j in range(m)]
    pub = np.frombuffer(V.le32([x for j in idx for x in publics[j]]), dtype=np.uint8).reshape(m, 3, 32).copy()
    weights = np.frombuffer(V.le32([rnd.getrandbits(128) for _ in range(m)]), dtype=np.uint8).reshape(m, 32).copy()
    crossover = None
    for spec in a.bad.split(","):
        k = m // 2 if spec == "half" else int(spec)
        bad = sorted(rnd.sample(range(m), k)) if k < m // 2 else list(range(1, m, 2))
        batch = [proofs[j] for j in idx]
        for j in bad:
            t = bytearray(batch[j])
            t[432 + 32 * (j % 6)] ^= 1
            batch[j] = bytes(t)
        want = [j not in set(bad) for j in range(m)]
        assert verifier.verify_each(batch, pub, fmt=FR_BYTES_LE) == want      # warm-up; checked
        each_ms = None
        for _ in range(a.reps):
            t = time.perf_counter()
            got = verifier.verify_each(batch, pub, fmt=FR_BYTES_LE)
            dt = (time.perf_counter() - t) * 1e3
            assert got == want, "verify_each does not name the tampered proofs (k = %d)" % k
            each_ms = dt if each_ms is None or dt < each_ms else each_ms
        stats = ctx.pairing_stats()
        leaves = verifier.pairing_inputs_segments(batch, pub, None, None, FR_BYTES_LE, 1)
        for j in sorted({0, m - 1} | set(bad[:3]) | {rnd.randrange(m) for _ in range(3)}):
            assert accepted(*leaves[j]) == want[j], "pair %d against the known tau" % j
        calls = []

        def decide(a96, b96):
            calls.append(1)
            return bp.pairing_check([(a96, b96)], setup.x_2, host=True)[0]
        t = time.perf_counter()
        located = verifier.locate_invalid(batch, pub, weights, decide, FR_BYTES_LE)
        locate_ms = (time.perf_counter() - t) * 1e3
        assert located == bad, "locate_invalid does not name the tampered proofs (k = %d)" % k
        row = {"m": m, "bad": k, "verify_each_ms": each_ms, "verify_each_pairing_stages_ms": stats, "locate_invalid_host_ms": locate_ms,
               "host_pairing_checks": len(calls), "locate_over_each": locate_ms / each_ms}
        if crossover is None and locate_ms > each_ms:
            crossover = k
        doc["locate"].append(row)
        print(json.dumps(row), flush=True)
    doc["crossover_bad_proofs"] = crossover
    print(json.dumps({"crossover_bad_proofs": crossover}), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

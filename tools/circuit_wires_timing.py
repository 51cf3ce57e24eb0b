#!/usr/bin/env python3
"""Two routes from a circuit's wire ids to a handle that can prove and check, on one MI355X -> profiles/circuit_wires_timing.json.

For the chained multiplications of synthetic.chained_multiplications (row i = (x_i, y_i, z_i), x_{i+1} = z_i: ids 1 .. 2n + 1, every
copy cycle of length 1 or 2) at --sizes rows (2^16, 2^20, 2^24), host clock around each blocking call, best of --reps after a warm-up:
  columns route   bp_make_s_polynomials on the host (one core), bp_circuit_load of eight 32-byte columns, the first
                  bp_circuit_check_sigma (the Pohlig-Hellman decode; its HIP-event time aside)
  wires route     bp_circuit_load_wires of five selector columns and 12 bytes of ids per row, with its HIP-event time per stage
                  (upload, largest id, sort, roots + link, derived forms), and the first bp_circuit_check_sigma (no decode)
The sigma columns of the two handles are compared byte for byte before a time is recorded.
At --prove-sizes (2^16, 2^20): bp_prove from three pageable host columns against bp_prove_assignment from one pageable value array
on the same handle, same bytes asserted, with the host-to-device bytes of each per proof.

  python tools/circuit_wires_timing.py [--sizes 16,20,24] [--prove-sizes 16,20] [--reps 3] [--out profiles/circuit_wires_timing.json]"""
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
from baby_plonk_rust_amd import synthetic  # noqa: E402

Q = bp.api.Q
TAU = 0x1234567


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def chain_ids(n):
    """the wire ids of synthetic.chained_multiplications"""
    ids = np.zeros((n, 3), dtype=np.uint32)
    ids[:, 0] = np.arange(1, n + 1, dtype=np.uint32)
    ids[:, 1] = np.arange(n + 2, 2 * n + 2, dtype=np.uint32)
    ids[:, 2] = np.arange(2, n + 2, dtype=np.uint32)
    return ids


def chain_selectors(n):
    zero = np.zeros((n, 4), dtype=np.uint64)
    return [zero, zero, np.tile(bp.scalar_from_int(Q - 1), (n, 1)), np.tile(bp.scalar_from_int(1), (n, 1)), zero]


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,20,24")
    ap.add_argument("--prove-sizes", default="16,20")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "circuit_wires_timing.json"))
    a = ap.parse_args()
    ctx = bp.Context(0)
    prove_sizes = [int(v) for v in a.prove_sizes.split(",") if v]
    doc = {"tool": "tools/circuit_wires_timing.py", "reps": a.reps, "device": torch.cuda.get_device_name(0), "sizes": []}
    clean = bp.SigmaReport(0, None, 0, None)
    for log_n in [int(v) for v in a.sizes.split(",")]:
        n = 1 << log_n
        ids, sel = chain_ids(n), chain_selectors(n)
        print(json.dumps({"log_n": log_n, "stage": "inputs ready"}), flush=True)

        def columns_route():
            make_ms, sig = timed(lambda: bp.make_s_polynomials(ids))
            load_ms, circuit = timed(lambda: bp.Circuit(sel + list(sig), ctx))
            check_ms, rep = timed(circuit.check_sigma)
            decode_ms = circuit.check_stats()["decode_ms"]
            assert rep == clean and decode_ms > 0
            return {"make_s_polynomials_ms": make_ms, "circuit_load_ms": load_ms, "first_check_sigma_ms": check_ms, "decode_ms": decode_ms,
                    "total_ms": make_ms + load_ms + check_ms}, circuit, sig

        def wires_route():
            load_ms, circuit = timed(lambda: bp.Circuit.from_wires(sel, ids, 0, ctx))
            stages = circuit.load_stats()
            check_ms, rep = timed(circuit.check_sigma)
            assert rep == clean and circuit.check_stats()["decode_ms"] == 0
            return {"circuit_load_wires_ms": load_ms, "stages_ms": stages, "first_check_sigma_ms": check_ms, "total_ms": load_ms + check_ms}, circuit

        _, c0, sig = columns_route()                                # warm-up of both routes; the columns compared
        _, c1 = wires_route()
        got = c1.columns(names=("s1", "s2", "s3"))
        assert all(got[k].tobytes() == sig[j].tobytes() for j, k in enumerate(("s1", "s2", "s3")))
        c0.free()
        c1.free()
        del got, sig
        best = [None, None]
        for _ in range(a.reps):
            r, c0, _ = columns_route()
            c0.free()
            if best[0] is None or r["total_ms"] < best[0]["total_ms"]:
                best[0] = r
            r, c1 = wires_route()
            c1.free()
            if best[1] is None or r["total_ms"] < best[1]["total_ms"]:
                best[1] = r
        row = {"log_n": log_n, "columns_route": best[0], "wires_route": best[1], "columns_over_wires": best[0]["total_ms"] / best[1]["total_ms"],
               "load_host_to_device_bytes": {"columns_route": 8 * 32 * n, "wires_route": (5 * 32 + 12) * n}}
        print(json.dumps(row), flush=True)

        if log_n in prove_sizes:
            wit, _ = synthetic.chained_multiplications(n, 7)
            # values[id]: x_i has id i + 1, z_(n-1) id n + 1, y_i id n + 2 + i; slot 0 is never read
            values = np.concatenate([np.zeros((1, 4), dtype=np.uint64), wit[0], wit[2][-1:], wit[1]])
            assert len(values) == 2 * n + 2
            circuit = bp.Circuit.from_wires(sel, ids, 0, ctx)
            setup = bp.Setup.generate_srs(n + 6, TAU, ctx)
            prover = bp.Prover(setup, circuit)
            blinders = [random.Random(1).randrange(1, Q) for _ in range(11)]
            want = prover.prove_with_blinding(*wit, None, blinders)      # warm-up of both; the same bytes
            assert prover.prove_assignment(values, blinders) == want
            prove_ms = min(timed(lambda: prover.prove_with_blinding(*wit, None, blinders))[0] for _ in range(a.reps))
            assign_ms = min(timed(lambda: prover.prove_assignment(values, blinders))[0] for _ in range(a.reps))
            gather_ms = min(timed(lambda: circuit.assign(values))[0] for _ in range(a.reps))
            circuit.free()
            ctx.srs_free(setup.handle)
            row["prove"] = {"bp_prove_host_columns_ms": prove_ms, "bp_prove_assignment_host_values_ms": assign_ms, "bp_circuit_assign_device_ms": gather_ms,
                            "host_to_device_bytes_per_proof": {"bp_prove": 3 * 32 * n, "bp_prove_assignment": 32 * len(values)}}
            print(json.dumps(row["prove"]), flush=True)
        doc["sizes"].append(row)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""bp_circuit_check_witness on one MI355X against the only route there was before it, bp_prove's refusal
-> profiles/witness_check_timing.json.

For the chained multiplications of synthetic.chained_multiplications at --sizes rows (2^16, 2^20, 2^22), with one product c_i, i = n / 2,
changed (row i fails its gate; both edges of the cycle (2, i) <-> (0, i + 1) fail their copy):
  first_check_ms    the first check of a freshly loaded circuit (sigma decode + in-degree passes + upload + check), host clock around the
                    blocking call, best of --reps fresh loads after a warm-up; with the HIP-event stage times of that call
  cached_check_ms   a repeated check of the same circuit, host witness (upload + check) and HBM-resident witness (the kernel alone)
  prove_refusal_ms  bp_prove on the same broken witness until it answers BP_ERR_ASSERT (-11); this pull request does not touch bp_prove
  for the cached kernel the bytes it moves (9 column reads, 3 target reads and 3 gathers per row) and their share of 8 TB/s; for the
  decode the Fr products per second (per cell: log_n squarings for the column, one product by 1 / k, log_n (log_n - 1) / 2 squarings
  and one product per set bit of the row for the logarithm).
Every timed report is compared with the closed form before its time is recorded.

  python tools/witness_check_timing.py [--sizes 16,20,22] [--reps 3] [--out profiles/witness_check_timing.json]"""
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
HBM_BYTES_PER_S = 8e12


def best_of(reps, fn):
    best = None
    for _ in range(reps):
        t = time.perf_counter()
        extra = fn()
        dt = (time.perf_counter() - t) * 1e3
        if best is None or dt < best[0]:
            best = (dt, extra)
    return best


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,20,22")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "witness_check_timing.json"))
    a = ap.parse_args()
    ctx = bp.Context(0)
    doc = {"tool": "tools/witness_check_timing.py", "reps": a.reps, "device": torch.cuda.get_device_name(0), "sizes": []}
    for log_n in [int(v) for v in a.sizes.split(",")]:
        n = 1 << log_n
        wit, pk = synthetic.chained_multiplications(n, 7)
        i = n // 2
        bad = [w.copy() for w in wit]
        bad[2][i] = bp.scalar_from_int((bp.scalar_to_int(bad[2][i]) + 1) % Q)
        want = bp.WitnessReport(1, i, 2, (2, i), (0, i + 1))
        clear = bp.WitnessReport(0, None, 0, None, None)
        print(json.dumps({"log_n": log_n, "stage": "inputs ready"}), flush=True)

        def first_check():
            circuit = bp.Circuit(pk, ctx)
            try:
                t = time.perf_counter()
                got = circuit.check_witness(*bad)
                dt = (time.perf_counter() - t) * 1e3
                stats = circuit.check_stats()
                assert got == want and stats["decode_ms"] > 0, (got, stats)
                return dt, stats
            finally:
                circuit.free()

        first_check()                                               # warm-up: the workspaces grow here; checked
        first_ms, first_stats = min((first_check() for _ in range(a.reps)), key=lambda r: r[0])
        print(json.dumps({"log_n": log_n, "first_check_ms": first_ms, **first_stats}), flush=True)

        circuit = bp.Circuit(pk, ctx)
        assert circuit.check_sigma() == bp.SigmaReport(0, None, 0, None)
        assert circuit.check_witness(*wit) == clear and circuit.check_witness(*bad) == want      # warm-up; checked

        def cached_host():
            got = circuit.check_witness(*bad)
            assert got == want and circuit.check_stats()["decode_ms"] == 0
            return circuit.check_stats()
        cached_ms, cached_stats = best_of(a.reps, cached_host)

        zero = np.zeros((n, 4), dtype=np.uint64)
        dev = [torch.from_numpy(w.view(np.int64)).cuda() for w in bad + [zero]]
        torch.cuda.synchronize()
        ptrs = [t.data_ptr() for t in dev]
        assert circuit.check_witness_device(*ptrs) == want

        def cached_device():
            got = circuit.check_witness_device(*ptrs)
            assert got == want
            return circuit.check_stats()
        device_ms, device_stats = best_of(a.reps, cached_device)
        kernel_ms = device_stats["check_ms"]
        moved = n * (9 * 32 + 3 * 4 + 3 * 32)

        setup = bp.Setup.generate_srs(n + 6, TAU, ctx)
        prover = bp.Prover(setup, circuit)
        blinders = [random.Random(1).randrange(1, Q) for _ in range(11)]

        def refusal():
            try:
                prover.prove_with_blinding(*bad, None, blinders)
            except bp.BpError as e:
                assert e.code == -11, e
                return prover.last_stats()
            raise AssertionError("bp_prove accepted the broken witness")
        refusal()                                                   # warm-up
        refusal_ms, _ = best_of(a.reps, refusal)
        prove_ms, _ = best_of(a.reps, lambda: prover.prove_with_blinding(*wit, None, blinders))
        assert circuit.check_witness(*bad) == want                  # the proofs in between disturbed nothing
        circuit.free()
        ctx.srs_free(setup.handle)

        products = 3 * n * (log_n + 1 + log_n * (log_n - 1) // 2) + 3 * n * log_n // 2
        row = {"log_n": log_n, "first_check_ms": first_ms, "first_check_stages_ms": first_stats,
               "cached_check_host_witness_ms": cached_ms, "cached_check_host_witness_stages_ms": cached_stats,
               "cached_check_device_witness_ms": device_ms, "cached_check_kernel_ms": kernel_ms,
               "cached_check_bytes": moved, "cached_check_share_of_8TBps": moved / (kernel_ms * 1e-3) / HBM_BYTES_PER_S,
               "decode_fr_products": products, "decode_fr_products_per_s": products / (first_stats["decode_ms"] * 1e-3),
               "prove_refusal_ms": refusal_ms, "prove_good_witness_ms": prove_ms,
               "refusal_over_cached_check": refusal_ms / cached_ms, "first_check_over_proof": first_ms / prove_ms}
        doc["sizes"].append(row)
        print(json.dumps(row), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

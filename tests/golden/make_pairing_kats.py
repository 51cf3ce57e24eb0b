#!/usr/bin/env python3
"""Extract the numeric literals the reference holds for the extension tower, G2 and the pairing.

Reads the reference's Rust sources AS TEXT (no code is copied, compiled or run) and writes the numeric literals -- inputs and
expected outputs of its unit tests, the G2 generator and Gt::generator() -- to pairing_kats.json, each with the file:line it came
from.  Run where the reference is present only:

    python tests/golden/make_pairing_kats.py /path/to/reference

Every literal is an Fp in the reference's memory form: six 64-bit Montgomery limbs, least significant first.  They are kept as
groups of six in source order; the tests know how many Fp make an Fp2 (2), an Fp6 (6), an Fp12 (12) or a G2 point (4, or 6 with z).
"""
import json
import os
import re
import sys

ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
SRC = os.path.join(ref, "lib/bls12_381/src")

WANT = {
    "fp2.rs": ["test_squaring", "test_multiplication", "test_addition", "test_subtraction", "test_negation", "test_inversion"],
    "fp6.rs": ["test_arithmetic"],
    "fp12.rs": ["test_arithmetic"],
    "g2.rs": ["test_doubling", "test_projective_addition", "test_mixed_addition"],
}
# functions whose body is one literal: (file, signature regex, key)
LITERAL_FNS = [
    ("pairings.rs", r"impl Group for Gt \{.*?fn generator\(\) -> Self \{", "Gt::generator"),
    ("g2.rs", r"pub fn generator\(\) -> G2Affine \{", "G2Affine::generator"),
]

fp_raw = re.compile(r"Fp::from_raw_unchecked\(\[\s*((?:0x[0-9a-fA-F_]+\s*,?\s*){6})\]\)")


def limbs(body):
    return [[hex(int(x.replace("_", ""), 16)) for x in re.findall(r"0x[0-9a-fA-F_]+", g)] for g in fp_raw.findall(body)]


def fn_body(text, start):
    """the text from `start` to the brace that closes the first `{` at or after it"""
    i = text.index("{", start)
    depth = 0
    for j in range(i, len(text)):
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return text[start: j + 1]
    return text[start:]


out = {}
for fname, tests in WANT.items():
    text = open(os.path.join(SRC, fname)).read()
    per = {}
    for t in tests:
        m = re.search(r"fn %s\(\)" % t, text)
        if not m:
            continue
        body = fn_body(text, m.start())
        per[t] = {"source": "lib/bls12_381/src/%s:%d" % (fname, text[:m.start()].count("\n") + 1), "fp": limbs(body)}
    out[fname] = per
for fname, sig, key in LITERAL_FNS:
    text = open(os.path.join(SRC, fname)).read()
    m = re.search(sig, text, re.S)
    body = fn_body(text, m.end() - 1)
    out.setdefault(fname, {})[key] = {"source": "lib/bls12_381/src/%s:%d" % (fname, text[:m.end()].count("\n") + 1), "fp": limbs(body)}

dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pairing_kats.json")
json.dump(out, open(dst, "w"), indent=None, separators=(",", ":"))
print("wrote", dst, {k: {t: len(v["fp"]) for t, v in per.items()} for k, per in out.items()})

"""The device check's case tables on the CPU (tests/devcheck, tests/adversarial.py): every dc_<name> entry point of libdevcheck_host.so
-- the per-case bodies the GPU threads run, compiled for the host with the device's column multiplier -- against Python integers, bit
for bit; the coverage predicates that keep the tables adversarial; and the proof that the tables can fail.  The device library is
only COMPILED here (that it cross-compiles for gfx950 is part of the check); tests/test_gpu_devcheck.py runs it."""
import collections
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from tests import adversarial as A
from tests import bigint_model as M
from tests.bigint_model import P, Q

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "devcheck")


@pytest.fixture(scope="module")
def libs():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    subprocess.check_call(["make", "-C", DIR, "-s", "-j2", "all"])
    return C.CDLL(os.path.join(DIR, "libdevcheck_host.so"))


@pytest.fixture(scope="module")
def tables(libs):
    b = np.zeros(2 * len(A.BOUND_NAMES), dtype=np.uint64)
    libs.devcheck_bounds.restype = None
    libs.devcheck_bounds(C.c_void_p(b.ctypes.data))
    return A.tables(b)


def exported(path):
    """the dc_* names in the library's dynamic string table (ctypes cannot list symbols; every name found must also resolve)"""
    import re
    names = {m.decode() for m in re.findall(rb"\x00dc_([a-z0-9_]+)(?=\x00)", open(path, "rb").read())}
    lib = C.CDLL(path)
    assert all(hasattr(lib, "dc_" + n) for n in names)
    return names


def test_every_wrapper_has_a_case_table(libs, tables):
    for so in ("libdevcheck_host.so", "libdevcheck.so"):
        assert exported(os.path.join(DIR, so)) == set(tables) == set(A.ENTRY), so
    assert all(len(t.rows) > 0 for t in tables.values())


def test_device_library_holds_gfx950_code():
    """libdevcheck.so was built for the card, not a fallback: it embeds a gfx950 code object with the wrappers' kernels"""
    blob = open(os.path.join(DIR, "libdevcheck.so"), "rb").read()
    assert b"gfx950" in blob and b"dck_fp_mul" in blob and b"dck_g1_28_add_coop" in blob


@pytest.mark.parametrize("name", sorted(A.ENTRY))
def test_host_build_equals_python_integers(libs, tables, name):
    t = tables[name]
    compared, bad = A.run_table(libs, t)
    assert compared == len(t.rows)
    assert not bad, "%d of %d cases differ\n%s" % (len(bad), compared, "\n".join(bad[:5]))


def test_inputs_stay_within_the_types_contracts(tables):
    """no case feeds a function limbs outside its static_assert'ed preconditions"""
    B = A.BOUNDS
    l28 = {"fp28_from": ["C28"], "fp28_mul": ["C28"] * 2, "fp28_mul2": ["C28"] * 4, "fp28_chain": ["C28"] * 4, "fp28_neg_mul2": ["MxT3s", "MxT1s", "MxT4", "MxY3"],
           "fp28_mulk12": ["C28"], "fp28_canon": ["M28"], "fp28_invert": ["M28"], "g1_28_add_mixed_raw": ["C28"] * 3 + ["F28n", "PtY28"],
           "g1_28_add_raw": ["C28"] * 6, "g1_28_add_coop": ["C28"] * 6, "g1_28_double_raw": ["C28"] * 3, "g1_28_is_identity": ["C28"] * 3}
    for name, types in l28.items():
        for row in tables[name].rows:
            for j, ty in enumerate(types):
                assert A.in_contract(row[14 * j:14 * j + 14], B[ty]), (name, ty)
    for name, k in (("fr29_add_lazy", 2), ("fr29_sub_lazy", 2), ("fr29_to_sat_canonical", 1), ("fr29_butterfly", 2), ("fr29_radix4", 4)):
        for row in tables[name].rows:
            for j in range(k):
                l = row[9 * j:9 * j + 9]
                assert max(l) <= M.M29 and M.undigits(l, 29) < 2 * Q, name
    for row in tables["fr29_mul"].rows:
        assert max(row[:9]) < 0xC0000000 and M.undigits(row[:9], 29) < 1 << 261 and max(row[9:]) <= M.M29 and M.undigits(row[9:], 29) < Q
    for row in tables["fr29_reduce8"].rows:
        assert max(row) < 1 << 31 and M.undigits(row, 29) < 8 * Q
    for f, m, n in (("fp", P, 12), ("fr", Q, 8)):
        for op in ("mul", "add", "sub"):
            for row in tables["%s_%s" % (f, op)].rows:
                assert M.undigits(row[:n], 32) < m and M.undigits(row[n:], 32) < m


def test_coverage_predicates(tables):
    cnt = collections.Counter((n, tag) for n, t in tables.items() for tags in t.tags for tag in tags)
    A.check_unreachable()
    low = []
    for key in A.required_predicates():
        print("%-24s %-44s %5d" % (key[0], key[1], cnt[key]))
        if cnt[key] < A.MIN_HITS:
            low.append((key, cnt[key]))
    for key, need in A.BOUNDED.items():
        print("%-24s %-44s %5d (all %d that exist)" % (key[0], key[1], cnt[key], need))
        if cnt[key] < need:
            low.append((key, cnt[key]))
    for name, why in A.UNREACHABLE.items():
        print("%-24s %-44s unreachable: %s" % ("-", name, why))
    print("%d cases over %d entry points" % (sum(len(t.rows) for t in tables.values()), len(tables)))
    assert not low, low


# ---- the tables can fail: three deliberately wrong MODELS (test code only) ---------------------------------------------------------
def told_apart(cases, f):
    return any(f(c, None) != f(c, True) for c in cases)


def test_adversarial_tables_tell_wrong_models_apart_where_random_ones_do_not(tables):
    rnd = random.Random(5)
    # 1. the final subtraction skipped when the operand equals the modulus exactly (Mont::reduce_once behind Fp::add)
    adv = [(M.undigits(r[:12], 32), M.undigits(r[12:], 32)) for r in tables["fp_add"].rows]
    uni = [(rnd.randrange(P), rnd.randrange(P)) for _ in adv]
    f1 = lambda c, bug: M.sat_reduce_once(c[0] + c[1], P, None, "skip_sub_when_equal" if bug else None)
    # 2. the reduction digit m[7] of mul28 masked with 2^27 - 1
    adv2 = [(r[:14], r[14:]) for r in tables["fp28_mul"].rows]
    uni2 = [(M.digits(rnd.randrange(P), 28, 14), M.digits(rnd.randrange(P), 28, 14)) for _ in adv2]
    f2 = lambda c, bug: M.mont_cols([(c[0], c[1])], M.P28D, M.INV28, 28, None, "mask_m7" if bug else None)
    # 3. the carry out of limb 12 lost in norm28 (behind sub28<8,30> in the addition's t3)
    def chain(c, bug):
        a, b, cc, d = c
        t0, t1 = M.f28_mul(a, cc), M.f28_mul(b, d)
        return M.f28_norm(M.f28_sub(8, 30, M.f28_mul(M.f28_add(a, b), M.f28_add(cc, d)), M.f28_add(t0, t1)), None, "drop_carry_12" if bug else None)
    adv3 = [(r[:14], r[14:28], r[28:42], r[42:]) for r in tables["fp28_chain"].rows]
    uni3 = [tuple(M.digits(rnd.randrange(P), 28, 14) for _ in range(4)) for _ in adv3]
    res = {"adversarial": (told_apart(adv, f1), told_apart(adv2, f2), told_apart(adv3, chain)),
           "uniform": (told_apart(uni, f1), told_apart(uni2, f2), told_apart(uni3, chain))}
    # (uniform operands do catch the masked digit and the lost carry -- half of all digits have bit 27 set, and the spread form of 8p
    # always carries -- but an operand exactly equal to the modulus has probability 2^-381 per case)
    print(res)
    assert all(res["adversarial"])
    assert not all(res["uniform"]) and not res["uniform"][0]

"""-m gpu: a ceremony's SRS in the 48-byte compressed encoding -- bp_srs_load_compressed48 (G1Affine::from_compressed /
from_compressed_unchecked, g1.rs:326-390), bp_srs_check_subgroup (is_torsion_free, g1.rs:401-411) and bp_srs_export_compressed48
(G1Affine::to_compressed, g1.rs:221-244) -- against the crate's fixtures, the CPU oracle's decoder and plain Python integers."""
import ctypes as C
import hashlib
import os
import random

import numpy as np
import pytest

import baby_plonk_rust_amd as bp
from baby_plonk_rust_amd import _lib
from oracle import oracle as O
from tests import bigint_model as M
from tests.test_srs_compressed_host import H, SIZE_MAX, ec_mul_unreduced, random_curve_point

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
P, Q = M.P, M.Q
COMP = open(os.path.join(GOLDEN, "g1_compressed_valid_test_vectors.dat"), "rb").read()
UNC = open(os.path.join(GOLDEN, "g1_uncompressed_valid_test_vectors.dat"), "rb").read()


@pytest.fixture(scope="module")
def ctx():
    c = bp.Context(0)
    yield c
    c.close()


def load_raw(ctx, recs, checks):
    """(rc, handle or None, first_bad) straight from the C ABI"""
    buf = np.frombuffer(bytes(recs), dtype=np.uint8).copy()
    h, bad = C.c_uint64(0), C.c_size_t(0)
    rc = ctx._lib.bp_srs_load_compressed48(ctx._h, buf.ctypes.data, len(buf) // 48, checks, C.byref(h), C.byref(bad))
    return rc, (h.value if rc == 0 else None), bad.value


def srs_count(ctx):
    """handles a context holds: a rejected load must leave none behind"""
    return sum(ctx._lib.bp_srs_len(ctx._h, h, C.byref(C.c_size_t())) == 0 for h in range(1, 4096))


def outside_point(rnd):
    """on the curve, outside G1: [r] P != O by a double-and-add that does not reduce r"""
    while True:
        q = random_curve_point(rnd)
        if ec_mul_unreduced(Q, q) is not None:
            return q


def test_crate_fixture_round_trip(ctx):
    h = ctx.srs_load_compressed48(COMP, check_subgroup=True)
    assert ctx.srs_len(h) == 1000
    assert ctx.srs_export(h) == UNC
    assert ctx.srs_export_compressed48(h) == COMP
    assert ctx.srs_export_compressed48(h, 331, 340) == COMP[48 * 331: 48 * 671]
    assert ctx.srs_check_subgroup(h) is None
    ctx.srs_free(h)
    h = ctx.srs_load(UNC)                                  # a bp_srs_load handle is checked the same way
    assert ctx.srs_check_subgroup(h) is None and ctx.srs_export_compressed48(h) == COMP
    ctx.srs_free(h)
    h = ctx.srs_load_compressed48(b"")                     # n == 0 as bp_srs_load
    assert ctx.srs_len(h) == 0 and ctx.srs_export_compressed48(h) == b""
    ctx.srs_free(h)


@pytest.mark.parametrize("tables", [False, True])
def test_same_group_elements_downstream(ctx, tables):
    hc, hu = ctx.srs_load_compressed48(COMP), ctx.srs_load(UNC)
    if tables:
        ctx.srs_precompute(hc)
        ctx.srs_precompute(hu)
    sc = O.splitmix_scalars(1000, 0xC0DE + tables)
    want = M.enc96(M.ec_mul(sum(i * s for i, s in enumerate(O.fr_array_to_ints(sc))) % Q))
    assert ctx.msm(hc, sc) == want
    assert ctx.msm_stats()["tables"] == tables
    assert ctx.msm(hu, sc) == want
    ctx.srs_free(hc)
    ctx.srs_free(hu)


def test_scale_2p22_round_trip(ctx):
    n = 1 << 22
    hg = ctx.srs_generate_progression(n, 0x5EED5EED12345, 0xABCDEF987)
    comp = ctx.srs_export_compressed48(hg)
    hc = ctx.srs_load_compressed48(comp, check_subgroup=True)
    chunk = 1 << 18
    for first in range(0, n, chunk):
        a, b = ctx.srs_export(hg, first, chunk), ctx.srs_export(hc, first, chunk)
        assert hashlib.sha256(a).digest() == hashlib.sha256(b).digest(), first
    # independent of the GPU encoder: the host's to_compressed of the 96-byte export on a random sample
    rnd = random.Random(22)
    lib = _lib.load()
    out = np.zeros(48, dtype=np.uint8)
    for i in sorted(rnd.sample(range(n), 1000)):
        u = np.frombuffer(ctx.srs_export(hg, i, 1), dtype=np.uint8).copy()
        assert lib.bp_g1_bytes96_to_compressed48(u.ctypes.data, out.ctypes.data) == 0
        assert bytes(out) == comp[48 * i: 48 * i + 48], i
    ctx.srs_free(hg)
    ctx.srs_free(hc)


def rejection_cases(rnd):
    good = M.enc48(M.ec_mul(777))
    while True:
        x = rnd.randrange(P)
        if pow((x ** 3 + 4) % P, (P - 1) // 2, P) == P - 1:
            break
    nonres = bytearray(x.to_bytes(48, "big"))
    nonres[0] |= 0x80
    return {"compression_clear": (bytes([good[0] & 0x7F]) + good[1:], "encoding"),
            "infinity_with_x": (bytes([good[0] | 0x40]) + good[1:], "encoding"),
            "e0_zeros": (bytes([0xE0]) + bytes(47), "encoding"),
            "40_zeros": (bytes([0x40]) + bytes(47), "encoding"),
            "x_eq_p": (bytes([0x80 | (P >> 376)]) + (P % (1 << 376)).to_bytes(47, "big"), "encoding"),
            "x_all_ones": (bytes([0x9F]) + bytes([0xFF] * 47), "encoding"),
            "non_residue": (bytes(nonres), "curve")}


@pytest.mark.parametrize("case", list(rejection_cases(random.Random(4))))
def test_rejections_name_the_index(ctx, case):
    rec, reason = rejection_cases(random.Random(4))[case]
    before = srs_count(ctx)
    for k in (0, 517, 999):
        recs = bytearray(COMP)
        recs[48 * k: 48 * k + 48] = rec
        for checks in (0, _lib.SRS_CHECK_SUBGROUP):
            rc, h, bad = load_raw(ctx, recs, checks)
            assert (rc, h, bad) == (-3, None, k), (case, k, checks)
            msg = ctx._lib.bp_last_error(ctx._h).decode()
            assert ("point %d " % k) in msg and reason in msg, msg
    with pytest.raises(bp.BpError) as e:
        ctx.srs_load_compressed48(recs)
    assert e.value.code == -3 and e.value.index == 999 and "point 999 " in str(e.value)
    assert srs_count(ctx) == before                        # no handle was created
    rc, h, bad = load_raw(ctx, COMP, _lib.SRS_CHECK_SUBGROUP)  # and the next valid load works
    assert rc == 0 and bad == SIZE_MAX
    assert ctx.srs_export(h) == UNC
    ctx.srs_free(h)


def test_subgroup(ctx):
    rnd = random.Random(5)
    q = outside_point(rnd)
    k, k2 = 123, 801
    for sort in (0, 1):
        rec = bytearray(q[0].to_bytes(48, "big"))
        rec[0] |= 0x80 | (0x20 * sort)
        recs = bytearray(COMP)
        recs[48 * k: 48 * k + 48] = rec
        q2 = outside_point(rnd)
        recs[48 * k2: 48 * k2 + 48] = M.enc48(q2)
        rc, h, bad = load_raw(ctx, recs, _lib.SRS_CHECK_SUBGROUP)
        assert (rc, h, bad) == (-3, None, k)
        assert "subgroup" in ctx._lib.bp_last_error(ctx._h).decode()
        h = ctx.srs_load_compressed48(recs, check_subgroup=False)
        y = q[1] if (q[1] > (P - 1) // 2) == bool(sort) else P - q[1]
        assert ctx.srs_export(h, k, 1) == M.enc96((q[0], y))
        assert ctx.srs_export(h, k2, 1) == M.enc96(q2)
        assert ctx.srs_check_subgroup(h) == k
        assert ctx.srs_check_subgroup(h, first=k + 1) == k2
        assert ctx.srs_check_subgroup(h, first=k2 + 1) is None
        assert ctx.srs_check_subgroup(h, first=0, n=k) is None
        ctx.srs_free(h)
    # 64 random members of G1 made as [h] (random curve point), at random places of the fixture: all pass
    recs = bytearray(COMP)
    for _ in range(64):
        i = rnd.randrange(1000)
        recs[48 * i: 48 * i + 48] = M.enc48(M.ec_mul(H, random_curve_point(rnd)))
    rc, h, bad = load_raw(ctx, recs, _lib.SRS_CHECK_SUBGROUP)
    assert rc == 0 and bad == SIZE_MAX
    assert ctx.srs_check_subgroup(h) is None
    ctx.srs_free(h)


def test_sort_flag_gives_the_negation(ctx):
    recs = bytearray(COMP)
    for i in range(1, 1000, 7):
        recs[48 * i] ^= 0x20
    h = ctx.srs_load_compressed48(recs, check_subgroup=True)
    got = ctx.srs_export(h)
    for i in range(1000):
        pt = M.dec48(COMP[48 * i: 48 * i + 48])
        want = (pt[0], P - pt[1]) if (i % 7 == 1 and pt is not None) else pt
        assert got[96 * i: 96 * i + 96] == M.enc96(want), i
    ctx.srs_free(h)


def test_per_point_agreement_with_the_oracle(ctx):
    """256 random encodings, about half of them on the curve, each loaded alone and unchecked: same decision, same bytes"""
    rnd = random.Random(6)
    accepted = 0
    for t in range(256):
        if t % 2:
            x, y = random_curve_point(rnd)
            rec = bytearray(M.enc48((x, y)))
            rec[0] ^= 0x20 * rnd.randrange(2)
        else:
            rec = bytearray(rnd.randrange(1 << 384).to_bytes(48, "big"))
            rec[0] = (rec[0] & 0x1F) | rnd.choice([0x80, 0xA0, 0x80, 0xA0, 0xC0, 0x00, 0xE0])
        rec = bytes(rec)
        aff, ok = O.g1_from_compressed(rec)
        rc, h, bad = load_raw(ctx, rec, 0)
        assert (rc == 0) == ok, rec.hex()
        if ok:
            accepted += 1
            assert ctx.srs_export(h) == O.g1_to_uncompressed(aff), rec.hex()
            ctx.srs_free(h)
        else:
            assert rc == -3 and bad == 0
    assert 100 < accepted < 200


def test_rehearsal_group_reports_global_indices():
    many = bp.Context([0, 0])
    try:
        rnd = random.Random(8)
        k = 700                                              # second shard (points 500..999)
        recs = bytearray(COMP)
        recs[48 * k: 48 * k + 48] = M.enc48(outside_point(rnd))
        rc, h, bad = load_raw(many, recs, _lib.SRS_CHECK_SUBGROUP)
        assert (rc, h, bad) == (-3, None, k)
        recs2 = bytearray(COMP)
        recs2[48 * 640] ^= 0x80                              # an encoding failure in the second shard
        assert load_raw(many, recs2, 0)[::2] == (-3, 640)
        h = many.srs_load_compressed48(recs, check_subgroup=False)
        assert many.n_shards() == 2 and many.srs_len(h) == 1000
        assert many.srs_check_subgroup(h) == k
        assert many.srs_check_subgroup(h, first=300, n=500) == k            # a range across both shards
        assert many.srs_check_subgroup(h, first=300, n=400) is None
        assert many.srs_export_compressed48(h, 0, k) == COMP[:48 * k]
        many.srs_free(h)
        h = many.srs_load_compressed48(COMP)
        assert many.srs_export(h) == UNC and many.srs_export_compressed48(h) == COMP
        many.srs_free(h)
    finally:
        many.close()

"""-m gpu: bp_srs_scale (one variable-base multiplication per lane, the srs_scale kernel over g1_mul_split28) on the edge scalars of
the split k = k1 x^2 + k0, on identity points, in both scalar formats, from host and device memory and over a two-shard group; and
the ceremony step built on it: Setup.contribute / verify_contribution.  Expected points: Python integers through O.g1_mul."""
import ctypes as C
import random

import numpy as np
import pytest

import baby_plonk_rust_amd as bp
from baby_plonk_rust_amd import BASIS_LAGRANGE, FR_BYTES_LE
from oracle import oracle as O
from tests import adversarial as A
from tests import bigint_model as M
from tests.gpu_common import progression_bytes
from tests.test_scalar_split import X2, edge_scalars

pytestmark = pytest.mark.gpu
Q, P = M.Q, M.P
N = 512
PROG_A, PROG_D = 0x7654321, 0x1F2E3D4C5B6A79
IDENTITY_AT = (5, 300)
ID96 = M.enc96(None)
TAU, S = 0x1F2E3D4C5B6A7988776655, 0xDEADBEEFCAFEF00D1234567
BAD_POINT, BAD_SCALAR, LENGTH = -3, -4, -6


@pytest.fixture(scope="module")
def ctx():
    c = bp.Context(0)
    yield c
    c.close()


def g1_bytes(k):
    return ID96 if k % Q == 0 else bytes(O.g1_bytes96(O.g1_mul(O.g1_generator(), O.fr_from_int(k % Q))))


def scalars():
    """the edges of the split first -- 0, 1, q - 1; x^2 - 1, x^2, x^2 + 1; k0 = 0 and k1 = 0; 2^127 +- 1, 2^128 +- 1; every value of
    tests/test_scalar_split.py's list below q -- then random ones; the two identity points get a non-zero scalar"""
    rnd = random.Random(0x5CA1E)
    edges = [0, 1, Q - 1, X2 - 1, X2, X2 + 1, 7 * X2, (Q // X2) * X2, X2 - 12345, 99, 2**127 - 1, 2**127 + 1, 2**128 - 1, 2**128 + 1]
    edges += [k for k in edge_scalars() if k < Q and k not in edges]
    assert len(edges) < N - 64
    ks = edges + [rnd.randrange(Q) for _ in range(N - len(edges))]
    rnd.shuffle(ks)
    for at in IDENTITY_AT:
        ks[at] = ks[at] or 3
    return ks


def source_bytes():
    pts = bytearray(progression_bytes(N, PROG_A, PROG_D))
    for at in IDENTITY_AT:
        pts[96 * at: 96 * at + 96] = ID96
    return bytes(pts)


@pytest.fixture(scope="module")
def case(ctx):
    """(source handle, scalars, expected bytes, the single-device result bytes): computed once, read by every test"""
    ks = scalars()
    h = ctx.srs_load(source_bytes())
    want = b"".join(ID96 if i in IDENTITY_AT else g1_bytes(k * (PROG_A + i * PROG_D)) for i, k in enumerate(ks))
    out = ctx.srs_scale(h, bp.scalars_from_ints(ks))
    got = ctx.srs_export(out)
    ctx.srs_free(out)
    return h, ks, want, got


def alive(ctx):
    """the SRS handles a context holds: a refused call must leave none behind"""
    return [h for h in range(1, 4096) if ctx._lib.bp_srs_len(ctx._h, h, C.byref(C.c_size_t())) == 0]


def le_bytes(ks):
    return np.frombuffer(b"".join(int(k).to_bytes(32, "little") for k in ks), dtype=np.uint8).reshape(-1, 32).copy()


def test_every_point_is_its_product(ctx, case):
    h, ks, want, got = case
    assert 0 in ks and 1 in ks and Q - 1 in ks and X2 in ks and 2**128 + 1 in ks
    for i in range(N):
        assert got[96 * i: 96 * i + 96] == want[96 * i: 96 * i + 96], (i, hex(ks[i]))
    assert got[96 * ks.index(0): 96 * ks.index(0) + 96] == ID96                      # k = 0 gives the identity
    assert ctx.srs_export(h) == source_bytes()                                        # the source is untouched
    st = ctx.srs_scale_stats()
    assert st["subgroup_ms"] > 0 and st["scale_ms"] > 0 and st["normalise_ms"] > 0


def test_formats_and_memories_agree(ctx, case):
    import torch
    h, ks, want, _ = case
    out = ctx.srs_scale(h, le_bytes(ks), fmt=FR_BYTES_LE)
    assert ctx.srs_export(out) == want and ctx.srs_basis(out) == ctx.srs_basis(h) and ctx.srs_len(out) == N
    ctx.srs_free(out)
    dev = torch.device("cuda", ctx.device)
    mont = torch.from_numpy(bp.scalars_from_ints(ks).view(np.int64)).to(dev)
    canon = torch.from_numpy(le_bytes(ks)).to(dev)
    torch.cuda.synchronize()
    for t, fmt in ((mont, bp.FR_MONT), (canon, FR_BYTES_LE)):
        before = t.clone()
        out = ctx.srs_scale(h, fmt=fmt, device_ptr=t.data_ptr(), n=N)
        assert ctx.srs_export(out) == want and bool((t == before).all())             # the caller's scalars are read, not converted in place
        ctx.srs_free(out)


def test_refusals_make_no_handle(ctx, case):
    h, ks, _, _ = case
    before = alive(ctx)
    for n in (N - 1, N + 1, 0):
        with pytest.raises(bp.BpError) as e:
            ctx.srs_scale(h, bp.scalars_from_ints((ks + [1])[:n]))
        assert e.value.code == LENGTH
    bad = list(ks)
    bad[200] = Q
    with pytest.raises(bp.BpError) as e:
        ctx.srs_scale(h, le_bytes(bad), fmt=FR_BYTES_LE)
    assert e.value.code == BAD_SCALAR
    rnd = random.Random(17)                                       # a curve point outside the subgroup, from the adversarial generator's pieces
    while True:
        x = A.limb_pattern(rnd, 32, 12, P)
        y = A.sqrt_p(x * x * x + 4)
        if y is not None and M.ec_mul_any(Q, (x, y)) is not None:
            break
    pts = bytearray(source_bytes())
    pts[96 * 17: 96 * 18] = M.enc96((x, y))
    outside = ctx.srs_load(bytes(pts))
    assert ctx.srs_check_subgroup(outside) == 17
    with pytest.raises(bp.BpError) as e:
        ctx.srs_scale(outside, bp.scalars_from_ints(ks))
    assert e.value.code == BAD_POINT and e.value.index == 17 and "17" in str(e.value)
    ctx.srs_free(outside)
    assert alive(ctx) == before


def test_group_context_scales_shard_by_shard(case):
    import torch
    _, ks, want, single = case
    group = bp.Context([0, 0])
    h = group.srs_load(source_bytes())
    out = group.srs_scale(h, bp.scalars_from_ints(ks))
    assert group.n_shards() == 2 and group.srs_len(out) == N
    assert group.srs_export(out) == single == want
    mont = torch.from_numpy(bp.scalars_from_ints(ks).view(np.int64)).to(torch.device("cuda", group.device))
    torch.cuda.synchronize()
    out2 = group.srs_scale(h, device_ptr=mont.data_ptr(), n=N)                        # device scalars: the second shard's slice crosses to it
    assert group.srs_export(out2) == want
    bad = list(ks)
    bad[N - 1] = Q                                                                    # a scalar >= q on the second shard
    with pytest.raises(bp.BpError) as e:
        group.srs_scale(h, le_bytes(bad), fmt=FR_BYTES_LE)
    assert e.value.code == BAD_SCALAR
    group.close()


def test_lagrange_basis_is_carried_over(ctx):
    powers = bp.Setup.generate_srs(8, TAU, ctx, tables=False)
    lag = powers.lagrange(8, tables=False)
    out = ctx.srs_scale(lag.handle, bp.scalars_from_ints([2] * 8))
    assert ctx.srs_basis(out) == (BASIS_LAGRANGE, 3)
    assert ctx.srs_export(out, 0, 1) == bp.sum_partials(bp.bytes96_to_partial(lag.powers_of_x()[:96]) * 2)
    ctx.srs_free(out)


def test_contribute_is_the_setup_of_the_product(ctx):
    previous = bp.Setup.generate_srs(64, TAU, ctx, tables=False)
    contributed = previous.contribute(S)
    expected = bp.Setup.generate_srs(64, TAU * S % Q, ctx, tables=False)
    assert contributed.powers_of_x() == expected.powers_of_x()
    assert contributed.x_2 == bp.g2_mul_generator(TAU * S % Q) == expected.x_2
    assert contributed.check_powers() is None and previous.powers_of_x()[96:192] != contributed.powers_of_x()[96:192]
    s_2 = bp.g2_mul_generator(S)
    assert contributed.verify_contribution(previous, s_2) is True
    assert contributed.verify_contribution(previous, bp.g2_mul_generator(S + 1)) is False          # a wrong s_2
    other = bp.Setup.generate_srs(64, TAU + 1, ctx, tables=False)
    assert contributed.verify_contribution(other, s_2) is False                                     # a previous of another tau
    shorter = bp.Setup.generate_srs(63, TAU, ctx, tables=False)
    assert contributed.verify_contribution(shorter, s_2) is False                                   # lengths differ
    broken = bp.Setup.from_points(contributed.powers_of_x()[:96 * 63] + previous.powers_of_x()[96 * 63:], ctx, tables=False, x_2=contributed.x_2)
    assert broken.verify_contribution(previous, s_2) is False                                       # not a clean SRS any more

"""-m gpu: a polynomial, all its cells and all its cell proofs rebuilt from some of the cells (recover_polynomial,
recover_polynomial_device, Setup.recover_cells: bp_kzg_recover, bp_kzg_recover_device, bp_kzg_recover_cells).  The tests draw a
polynomial f themselves and hand some of its cells over: the expected coefficients ARE f, the expected cells and proofs come from
tests/kzg_cells_model.py, the index a corrupted value is reported at and the interpolant of inconsistent cells from
tests/kzg_recover_model.py.  No expectation comes from the library.  Shapes (log_n, log_l): (2,1) r = 2, one cell missing; (3,0) l = 1;
(3,3) one cell, r = 1; (4,2); (7,3); (9,6) the PeerDAS cell, r = 8, four missing; (9,2) r = 128, 64 missing; WALK_SHAPE, chosen from
_lib.KZG_RECOVER_WALK: the smallest r with 2 WALK + 3 missing cells at l = 2 (three slices of the root walk, the last one short, and
more than one workgroup of points); GROUP_SHAPE: 4 WALK + 1 missing cells at l = 1, five slices, so that the products of two
workgroups per point are multiplied by the second pass."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import baby_plonk_rust_amd as bp
from baby_plonk_rust_amd import FR_BYTES_LE, FR_MONT, _lib
from tests import bigint_model as M
from tests import kzg_cells_model as CM
from tests import kzg_model as K
from tests import kzg_recover_model as RM

pytestmark = pytest.mark.gpu
Q = M.Q
TAU = 0x5EED0123456789ABCDEF0F1E2D3C4B5A69788796A5B4C3D2E1F00112233445566 % Q
WALK = _lib.KZG_RECOVER_WALK
SHAPES = ((2, 1), (3, 0), (3, 3), (4, 2), (7, 3), (9, 6), (9, 2))
MISSING = {(2, 1): 1, (3, 0): 4, (3, 3): 0, (4, 2): 2, (7, 3): 8, (9, 6): 4, (9, 2): 64}


def shape_for(missing, log_l):
    """the smallest domain whose r = n / l cells leave at least one present with `missing` of them gone"""
    log_r = missing.bit_length()                                   # 2^log_r > missing
    return log_r + log_l, log_l


WALK_SHAPE, GROUP_SHAPE = shape_for(2 * WALK + 3, 1), shape_for(4 * WALK + 1, 0)
MISSING[WALK_SHAPE], MISSING[GROUP_SHAPE] = 2 * WALK + 3, 4 * WALK + 1
INVALID_ARG, BAD_SCALAR, LENGTH, ASSERT = -1, -4, -6, -11


@pytest.fixture(scope="module")
def ctx():
    c = bp.Context(0)
    yield c
    c.close()


def case(log_n, log_l, d=None, missing=None, seed=0, f=None):
    """(n, l, f, the present indices shuffled, their cells as integers) with deg f < d <= m l"""
    n, l = 1 << log_n, 1 << log_l
    r, rnd = n // l, random.Random(1000 * log_n + 10 * log_l + seed)
    gone = MISSING[(log_n, log_l)] if missing is None else missing
    idx = rnd.sample(range(r), r - gone)                          # a random subset in random order
    d = rnd.randrange(1, len(idx) * l + 1) if d is None else d
    f = [rnd.randrange(Q) for _ in range(d)] if f is None else f
    cells = RM.cells_of(f, n, l)
    return n, l, f, idx, [cells[k] for k in idx]


def mont(cells):
    return bp.scalars_from_ints([v for row in cells for v in row]).reshape(len(cells), -1, 4)


def le_bytes(cells):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for row in cells for v in row), dtype=np.uint8).reshape(len(cells), -1, 32).copy()


def on_device(ctx, cells):
    t = torch.from_numpy(mont(cells).view(np.int64).copy()).to(torch.device("cuda", ctx.device))
    torch.cuda.current_stream().synchronize()
    return t


def ints(poly):
    return bp.scalars_to_ints(poly.values)


# ---- 1. the coefficients are f, by every route -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_l", SHAPES + (WALK_SHAPE, GROUP_SHAPE))
def test_recovers_the_polynomial(ctx, log_n, log_l):
    n, l, f, idx, cells = case(log_n, log_l)
    d = len(f)
    assert ints(bp.recover_polynomial(idx, mont(cells), n, d, ctx)) == f                             # host, Montgomery limbs
    assert ints(bp.recover_polynomial(idx, le_bytes(cells), n, d, ctx, fmt=FR_BYTES_LE)) == f        # canonical bytes in and out
    got = bp.recover_polynomial_device(idx, on_device(ctx, cells), l, n, d, ctx)                    # HBM in and out
    assert len(got) == d and ints(got) == f
    whole = got.t._base.cpu().numpy().view(np.uint64)
    assert whole.shape == (n, 4) and not whole[d:].any()                                            # places d .. n - 1 are zero
    if MISSING[(log_n, log_l)]:
        stats = ctx.kzg_recover_stats()
        assert all(np.isfinite(v) and v >= 0 for v in stats.values()) and len(stats) == 4 and stats["coset_ms"] > 0


@pytest.mark.parametrize("log_n,log_l", SHAPES + (WALK_SHAPE,))
def test_edges_of_the_degree_bound(ctx, log_n, log_l):
    n, l = 1 << log_n, 1 << log_l
    m = n // l - MISSING[(log_n, log_l)]
    rnd = random.Random(log_n)
    runs = {"nothing missing": case(log_n, log_l, missing=0, seed=1),
            "m l == d": case(log_n, log_l, d=m * l, seed=2),
            "d = 1": case(log_n, log_l, d=1, seed=3),
            "shorter than d": case(log_n, log_l, d=m * l, seed=4, f=[rnd.randrange(1, Q) for _ in range(max(m * l // 2, 1))]),
            "zero": case(log_n, log_l, d=max(m * l - 1, 1), seed=5, f=[0] * max(m * l - 1, 1))}
    for name, (_, _, f, idx, cells) in runs.items():
        d = m * l if name == "shorter than d" else len(f)
        got = ints(bp.recover_polynomial(idx, mont(cells), n, d, ctx))
        assert got == f + [0] * (d - len(f)), name
        if name == "nothing missing":
            stats = ctx.kzg_recover_stats()
            assert stats["vanishing_ms"] == 0 and stats["coset_ms"] == 0 and stats["spread_ms"] > 0 and stats["check_ms"] > 0
            assert all(np.isfinite(v) and v >= 0 for v in stats.values())
    if n >= 2:                                                      # the default bound: the rate-1/2 extension, with every cell at hand
        _, _, f, idx, cells = case(log_n, log_l, d=n // 2, missing=0, seed=6)
        assert ints(bp.recover_polynomial(idx, mont(cells), n, None, ctx)) == f


# ---- 2. errors --------------------------------------------------------------------------------------------------------------------------------
def raw(ctx, log_n, log_l, idx, cells, d, fmt=FR_BYTES_LE):
    """bp_kzg_recover itself, outputs pre-filled with 0xA5: (rc, first_bad, the output buffer)"""
    ix = np.array(list(idx) + [0], dtype=np.uint32)
    src = le_bytes(cells) if fmt == FR_BYTES_LE else mont(cells)
    out, bad = np.full(32 << log_n, 0xA5, dtype=np.uint8), C.c_size_t(777)
    rc = ctx._lib.bp_kzg_recover(ctx._h, log_n, log_l, ix.ctypes.data, src.ctypes.data, len(idx), d, fmt, out.ctypes.data, C.byref(bad))
    return rc, bad.value, out


def test_refusals_leave_the_outputs_untouched(ctx):
    log_n, log_l = 4, 2
    n, l, f, idx, cells = case(log_n, log_l, d=5)                   # r = 4, two cells present
    size_max = C.c_size_t(-1).value
    over = [list(row) for row in cells]
    over[1][3] = Q                                                 # a canonical-bytes value >= q, in the cell at position 1
    refusals = {"index >= r": ([idx[0], 4], cells, 5, INVALID_ARG, 1),
                "duplicate": ([idx[0], idx[1], idx[0]], cells + [cells[0]], 5, INVALID_ARG, 2),
                "too few cells": (idx, cells, 9, LENGTH, size_max),
                "n_coeffs == 0": (idx, cells, 0, LENGTH, size_max),
                "a value >= q": (idx, over, 5, BAD_SCALAR, 1)}
    setup = bp.Setup.generate_srs(n, TAU, ctx, tables=False)
    try:
        for name, (ix, rows, d, code, where) in refusals.items():
            rc, bad, out = raw(ctx, log_n, log_l, ix, rows, d)
            assert (rc, bad) == (code, where) and (out == 0xA5).all(), name
            vals, proofs, bad = np.full(32 * n, 0xA5, dtype=np.uint8), np.full((n // l, 96), 0xA5, dtype=np.uint8), C.c_size_t(777)
            ixa, src = np.array(list(ix) + [0], dtype=np.uint32), le_bytes(rows)
            rc = ctx._lib.bp_kzg_recover_cells(ctx._h, setup.handle, log_n, log_l, ixa.ctypes.data, src.ctypes.data, len(ix), d, FR_BYTES_LE,
                                               vals.ctypes.data, proofs.ctypes.data, C.byref(bad))
            assert (rc, bad.value) == (code, where) and (vals == 0xA5).all() and (proofs == 0xA5).all(), name
            if code != BAD_SCALAR:                                 # the device entry takes Montgomery limbs: no such thing as a value >= q
                rows_q = [[v % Q for v in row] for row in rows]
                d_out = torch.full((n, 4), 0x25A5A5A5A5A5A5A5, dtype=torch.int64, device=torch.device("cuda", ctx.device))
                torch.cuda.current_stream().synchronize()
                bad = C.c_size_t(777)
                rc = ctx._lib.bp_kzg_recover_device(ctx._h, log_n, log_l, ixa.ctypes.data, on_device(ctx, rows_q).data_ptr(), len(ix), d,
                                                    d_out.data_ptr(), C.byref(bad))
                assert (rc, bad.value) == (code, where) and bool((d_out == 0x25A5A5A5A5A5A5A5).all()), name
        with pytest.raises(bp.BpError) as e:                       # the Python layer carries the position
            bp.recover_polynomial([idx[0], idx[1], idx[0]], mont(cells + [cells[0]]), n, 5, ctx)
        assert e.value.code == INVALID_ARG and e.value.index == 2
        with pytest.raises(bp.BpError) as e:
            bp.recover_polynomial(idx, mont(cells), n, 9, ctx)
        assert e.value.code == LENGTH and e.value.index is None
        lib, h = ctx._lib, ctx._h
        ixa, src, out = np.array(idx, dtype=np.uint32), mont(cells), np.full(32 * n, 0xA5, dtype=np.uint8)
        assert lib.bp_kzg_recover(h, log_n, log_l, ixa.ctypes.data, src.ctypes.data, 2, 5, 7, out.ctypes.data, None) == -1      # bad format
        assert lib.bp_kzg_recover(h, log_n, log_l, None, src.ctypes.data, 2, 5, FR_MONT, out.ctypes.data, None) == -1          # null indices
        assert lib.bp_kzg_recover(h, log_n, log_l, ixa.ctypes.data, None, 2, 5, FR_MONT, out.ctypes.data, None) == -1          # null values
        assert lib.bp_kzg_recover(h, log_n, log_l, ixa.ctypes.data, src.ctypes.data, 2, 5, FR_MONT, None, None) == -1          # null output
        assert lib.bp_kzg_recover_cells(h, setup.handle, log_n, log_l, ixa.ctypes.data, src.ctypes.data, 2, 5, FR_MONT, None, None, None) == -1
        assert lib.bp_kzg_recover_cells(h, 0xDEAD, log_n, log_l, ixa.ctypes.data, src.ctypes.data, 2, 5, FR_MONT, None, out.ctypes.data, None) == -1
        assert lib.bp_kzg_recover(h, 24, 10, ixa.ctypes.data, src.ctypes.data, 2, 5, FR_MONT, out.ctypes.data, None) == -10
        assert lib.bp_kzg_recover(h, 20, 3, ixa.ctypes.data, src.ctypes.data, 2, 5, FR_MONT, out.ctypes.data, None) == -10     # r = 2^17
        assert (out == 0xA5).all()
        assert lib.bp_kzg_recover(h, log_n, log_l, ixa.ctypes.data, src.ctypes.data, 2, 5, FR_MONT, out.ctypes.data, None) == 0   # first_bad may be NULL
    finally:
        ctx.srs_free(setup.handle)


@pytest.mark.parametrize("log_n,log_l", ((2, 1), (4, 2), (9, 6), WALK_SHAPE))
def test_one_wrong_value(ctx, log_n, log_l):
    """with redundancy: BP_ERR_ASSERT at the model's index, the host output untouched; with m l == d: the model's interpolant"""
    m, rnd = (1 << (log_n - log_l)) - MISSING[(log_n, log_l)], random.Random(log_n)
    d = rnd.randrange(1, m << log_l)                               # d < m l: there is redundancy
    n, l, f, idx, cells = case(log_n, log_l, d=d, seed=7)
    flipped = [list(row) for row in cells]
    i, j = rnd.randrange(m), rnd.randrange(l)
    flipped[i][j] = (flipped[i][j] + 1) % Q
    want, where = RM.recover(n, l, idx, flipped, d)
    assert where is not None and d <= where < m * l
    rc, bad, out = raw(ctx, log_n, log_l, idx, flipped, d)
    assert (rc, bad) == (ASSERT, where) and (out == 0xA5).all()
    with pytest.raises(bp.BpError) as e:
        bp.recover_polynomial_device(idx, on_device(ctx, flipped), l, n, d, ctx)
    assert e.value.code == ASSERT and e.value.index == where
    assert ints(bp.recover_polynomial(idx, mont(flipped), n, m * l, ctx)) == want[:m * l] and not any(want[m * l:])
    assert ints(bp.recover_polynomial(idx, mont(cells), n, d, ctx)) == f      # and the cells as they were are accepted


# ---- 3. all cells and proofs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_recover_cells(ctx, log_n, log_l):
    # (9,6): the rate-1/2 column, 256 coefficients from four cells of 64 -- more than l coefficients, so the quotients are not zero
    n, l, f, idx, cells = case(log_n, log_l, d=256 if (log_n, log_l) == (9, 6) else None, seed=8)
    r = n // l
    setup = bp.Setup.generate_srs(max(n - l, 1), TAU, ctx, tables=False)
    try:
        want_values, want_scalars = CM.all_cells(f, n, l, TAU)
        got_cells, proofs = setup.recover_cells(idx, mont(cells), n, len(f))
        assert got_cells.shape == (r, l, 4) and proofs.shape == (r, 96)
        assert bp.scalars_to_ints(got_cells) == [v for row in want_values for v in row]
        for k in range(r):
            assert bytes(proofs[k]) == K.point96(want_scalars[k]), k
        given = mont(cells)
        for i, k in enumerate(idx):                                 # the present cells come back as given
            assert (got_cells[k] == given[i]).all(), k
        if (log_n, log_l) == (9, 6):                               # the recovered claims pass the batch check of the cell proofs
            com = K.point96(K.horner(f, TAU))
            claims = [bp.CellOpening(com, k, got_cells[k], bytes(proofs[k])) for k in range(r)]
            tau_l_g2 = bp.g2_mul_generator(pow(TAU, l, Q))
            assert setup.verify_cells(claims, n, tau_l_g2) is True
            missing = [k for k in range(r) if k not in idx]
            off = list(claims)
            off[missing[0]] = off[missing[0]]._replace(proof=bytes(proofs[missing[1]]))
            assert setup.verify_cells(off, n, tau_l_g2) is False
        # values_out = NULL is allowed, and canonical bytes in and out
        out, vals, bad = np.zeros((r, 96), dtype=np.uint8), np.zeros(32 * n, dtype=np.uint8), C.c_size_t(0)
        ixa, src = np.array(idx, dtype=np.uint32), le_bytes(cells)
        call = lambda v: ctx._lib.bp_kzg_recover_cells(ctx._h, setup.handle, log_n, log_l, ixa.ctypes.data, src.ctypes.data, len(idx), len(f), FR_BYTES_LE,
                                                      v, out.ctypes.data, C.byref(bad))
        assert call(None) == 0 and (out == proofs).all()
        out[:] = 0
        assert call(vals.ctypes.data) == 0 and (out == proofs).all()
        assert [int.from_bytes(vals[32 * i: 32 * i + 32].tobytes(), "little") for i in range(n)] == [v for row in want_values for v in row]
    finally:
        ctx.srs_free(setup.handle)


def test_recover_cells_needs_the_setup_of_open_cosets(ctx):
    n, l, f, idx, cells = case(4, 2, seed=9)
    short = bp.Setup.generate_srs(8, TAU, ctx, tables=False)       # n - l = 12 points are needed
    lag = ctx.srs_lagrange(short.handle, 3)
    try:
        with pytest.raises(bp.BpError) as e:
            short.recover_cells(idx, mont(cells), n, len(f))
        assert e.value.code == LENGTH and e.value.index is None
        with pytest.raises(bp.BpError) as e:
            bp.Setup(lag, ctx, tables=False).recover_cells(idx, mont(cells), n, len(f))
        assert e.value.code == -5
    finally:
        ctx.srs_free(lag)
        ctx.srs_free(short.handle)


# ---- 4. a group context ------------------------------------------------------------------------------------------------------------------------
def test_group_context(ctx):
    """a two-member rehearsal context {0, 0}: the recovery runs on the primary device, the SRS of the second half is sharded"""
    log_n, log_l = 7, 3
    n, l, f, idx, cells = case(log_n, log_l, seed=10)
    want_values, want_scalars = CM.all_cells(f, n, l, TAU)
    many = bp.Context([0, 0])
    try:
        assert many.n_shards() == 2
        assert ints(bp.recover_polynomial(idx, mont(cells), n, len(f), many)) == f
        assert ints(bp.recover_polynomial_device(idx, on_device(many, cells), l, n, len(f), many)) == f
        setup = bp.Setup.generate_srs(n, TAU, many, tables=False)
        got_cells, proofs = setup.recover_cells(idx, mont(cells), n, len(f))
        assert bp.scalars_to_ints(got_cells) == [v for row in want_values for v in row]
        assert [bytes(p) for p in proofs] == [K.point96(s) for s in want_scalars]
        many.srs_free(setup.handle)
    finally:
        many.close()

"""-m gpu: Fr NTT through the C ABI vs the oracle (faithful O(n^2) restatement of src/utils.rs:63-129 at
small n, its O(n log n) twin elsewhere).  Bit-exact on the Montgomery limbs."""
import random

import numpy as np
import pytest

import baby_plonk_rust_amd as bp
from oracle import oracle as O
from tests import bigint_model as M
from tests.gpu_common import NTHREADS, Q, experiment

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return bp.default_context()


def frs(vals):
    return bp.scalars_from_ints([v % Q for v in vals])


@pytest.mark.parametrize("logn", list(range(0, 13)))
def test_small_sizes_vs_oracle(ctx, logn):
    n = 1 << logn
    a = O.splitmix_scalars(n, 0xF40000 + logn)
    fwd = bp.ntt_381(a, ctx)
    assert (fwd == O.ntt_fast(a)).all()
    inv = bp.i_ntt_381(a, ctx)
    assert (inv == O.ntt_fast(a, inverse=True)).all()
    assert (bp.i_ntt_381(fwd, ctx) == a).all()
    if logn <= 7:                                     # the reference's literal algorithm
        assert (fwd == O.ntt_381(a)).all() and (inv == O.i_ntt_381(a)).all()
    if logn <= 5:                                     # independent big-int DFT
        assert bp.scalars_to_ints(fwd) == M.dft(bp.scalars_to_ints(a))


def test_simple_vectors_and_errors(ctx):
    assert bp.scalars_to_ints(bp.ntt_381(frs([1, 0, 0, 0, 0, 0, 0, 0]), ctx)) == [1] * 8
    assert bp.scalars_to_ints(bp.ntt_381(frs([3, 3]), ctx)) == [6, 0]           # setup.rs:128-135 input
    assert bp.scalars_to_ints(bp.i_ntt_381(frs([6, 0]), ctx)) == [3, 3]
    for bad in (3, 6, 12, 1000):
        with pytest.raises(bp.BpError) as e:
            bp.ntt_381(frs(list(range(bad))), ctx)                              # utils.rs:65 assert!
        assert e.value.code == -2
    # canonical little-endian format
    vals = [5, 7, Q - 1, 0]
    le = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4)
    out = ctx.ntt(le, fmt=bp.FR_BYTES_LE)
    got = [int.from_bytes(out[i].tobytes(), "little") for i in range(4)]
    assert got == M.dft(vals)
    # roots_of_unity (utils.rs:45-52) and test_root_of_unity (utils.rs:239-242)
    w4 = bp.scalar_to_int(bp.root_of_unity(4))
    assert pow(w4, 4, Q) == 1 and pow(w4, 2, Q) != 1
    assert bp.scalars_to_ints(bp.roots_of_unity(8, ctx)) == [pow(M.omega(8), i, Q) for i in range(8)]
    assert (bp.roots_of_unity(1 << 12, ctx) == _roots_oracle(1 << 12)).all()


def _roots_oracle(n):
    out = O.u64((n, 4))
    O.lib.ntt_roots_of_unity(out.ctypes.data, n)
    return out


@pytest.mark.parametrize("logn", [13, 14, 15, 16, 17, 18, 20])
def test_multi_pass_sizes_vs_oracle(ctx, logn):
    """BASELINE configs[1] (2^16) and the 2^20 size, both directions"""
    n = 1 << logn
    a = O.splitmix_scalars(n, 0xF40000 + logn)
    fwd = bp.ntt_381(a, ctx)
    assert (fwd == O.ntt_fast(a, threads=NTHREADS)).all()
    inv = bp.i_ntt_381(a, ctx)
    assert (inv == O.ntt_fast(a, inverse=True, threads=NTHREADS)).all()


def test_batch_columns_and_stride(ctx):
    """independent columns (the multi-GPU sharding unit): batch with a stride larger than the length"""
    for logn, batch, row in ((6, 5, 64), (9, 3, 700), (12, 4, 4096 + 64), (14, 3, 1 << 14)):
        n = 1 << logn
        data = O.splitmix_scalars(batch * row, 0xBA7C4 + logn).reshape(batch, row, 4)
        out = ctx.ntt_batch(data, stride=n)
        for b in range(batch):
            assert (out[b, :n] == O.ntt_fast(data[b, :n])).all()
            assert (out[b, n:] == data[b, n:]).all()            # padding untouched
        back = ctx.ntt_batch(out, inverse=True, stride=n)
        assert (back == data).all()


def test_2p24_round_trip_and_spot_checks(ctx):
    """the 2^24 size: inverse(forward(x)) == x, linearity, and spot outputs against the direct sum"""
    import torch
    logn, n = 24, 1 << 24
    a = O.splitmix_scalars(n, 0xF40018)
    t = torch.from_numpy(a.view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    ctx.ntt_device(t.data_ptr(), logn)
    fwd = t.cpu().numpy().view(np.uint64)
    w = M.omega(n)
    for x in (0, 1, 12345, n // 2 + 77, n - 1):
        # out[x] = sum_y in[y] w^(xy) = polynomial with coefficients `in` evaluated at w^x
        assert (fwd[x] == O.poly_eval(a, O.fr_from_int(pow(w, x, Q)), fast=True)).all()
    ctx.ntt_device(t.data_ptr(), logn, inverse=True)
    assert (t.cpu().numpy().view(np.uint64) == a).all()
    assert ctx.ntt_stats()["passes"] == 3


def test_2p24_full_array_vs_oracle(ctx):
    """the 2^24 size element for element: forward and inverse transforms of 2^24 elements in HBM equal the oracle's
    O(n log n) twin of utils.rs:63-129 on every one of the 2^24 outputs (the twin itself equals the literal O(n^2) restatement up to
    2^10, tests/test_oracle_msm_ntt_poly.py)"""
    import torch
    logn, n = 24, 1 << 24
    a = O.splitmix_scalars(n, 0xF40024)
    t = torch.from_numpy(a.view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    ctx.ntt_device(t.data_ptr(), logn)
    want = O.ntt_fast(a, threads=NTHREADS)
    assert (t.cpu().numpy().view(np.uint64).reshape(-1, 4) == want).all()
    del want
    t.copy_(torch.from_numpy(a.view(np.int64)))
    torch.cuda.synchronize()
    ctx.ntt_device(t.data_ptr(), logn, inverse=True)
    assert (t.cpu().numpy().view(np.uint64).reshape(-1, 4) == O.ntt_fast(a, inverse=True, threads=NTHREADS)).all()


def test_async_transforms_back_to_back(ctx):
    """bp_ntt_fr_device_async: transforms enqueued on the context's stream without a host wait in between"""
    import torch
    x = O.splitmix_scalars(1 << 14, 0xA5)
    t = torch.from_numpy(x.view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    ctx.ntt_device_async(t.data_ptr(), 14)                       # forward, inverse, forward: ends as one forward transform
    ctx.ntt_device_async(t.data_ptr(), 14, inverse=True)
    ctx.ntt_device_async(t.data_ptr(), 14)
    ctx.synchronize()
    assert (t.cpu().numpy().view(np.uint64).reshape(-1, 4) == O.ntt_fast(x)).all()
    st = ctx.ntt_stats()
    assert st["device_ms"] > 0 and st["passes"] == 2
    ctx.ntt_device(t.data_ptr(), 14, inverse=True)               # a blocking call after enqueued ones
    assert (t.cpu().numpy().view(np.uint64).reshape(-1, 4) == x).all()


@experiment
def test_driver_branches_under_knobs(monkeypatch):
    """the branches of the driver (csrc/ntt.hip) that no default-size transform reaches, at the smallest sizes that reach them, forward
    and inverse against the oracle: the two-level lookup drain (by default above 2^24 only), padded 8-column tiles, a single column
    without pad, two- and three-pass splits of the knob's choosing, the middle-digit swap of (a, a, a - 1), and -- all on ONE context, so
    that a later knob meets the inter-pass tables an earlier one built -- the rebuild of a pass table whose (l, s) changed.  The shapes
    themselves are judged on the CPU (tests/test_ntt_plan.py); BP_NTT_LANES_SHIFT and the splits the plan rejects stay there."""
    ctx = bp.Context(0)                 # its own: the default context's tables for these sizes would outlive BP_NTT_FULL_TWIDDLES_MAX_LOG=0
    data = {logn: O.splitmix_scalars(1 << logn, 0xD21E00 + logn) for logn in (11, 12, 13)}
    want = {(logn, inv): O.ntt_fast(a, inverse=inv) for logn, a in data.items() for inv in (False, True)}
    knobs = ("BP_NTT_FULL_TWIDDLES_MAX_LOG", "BP_NTT_SWIZZLE", "BP_NTT_SPLIT", "BP_NTT_THREE_PASS_FROM", "BP_NTT_COLS_LOG_L7")

    def run(logn, passes, **env):
        for name in knobs:
            monkeypatch.delenv(name, raising=False)
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        for inv in (False, True):
            got = bp.i_ntt_381(data[logn], ctx) if inv else bp.ntt_381(data[logn], ctx)
            assert (got == want[logn, inv]).all(), (logn, inv, env)
            assert ctx.ntt_stats()["passes"] == passes, (logn, env)

    run(11, 2, BP_NTT_FULL_TWIDDLES_MAX_LOG="0")       # 6, 5 and 6, 6 with no full table: lo / hi lookup in the drain
    run(12, 2, BP_NTT_FULL_TWIDDLES_MAX_LOG="0")
    run(12, 2)                                         # the same split, now through full tables (built here)
    run(12, 2, BP_NTT_SWIZZLE="0")                     # 2^6 x 8 tiles, padded
    run(11, 2, BP_NTT_SPLIT="11:9,2,0")
    run(12, 2, BP_NTT_SPLIT="12:10,2,0")               # (l, s) = (10, 2) where the table holds (6, 6): rebuilt
    run(13, 3, BP_NTT_SPLIT="13:5,4,4")
    run(11, 3, BP_NTT_THREE_PASS_FROM="11")            # 4, 4, 3 -> 4, 3, 4; pass 1's table held (9, 2)
    run(12, 2, BP_NTT_COLS_LOG_L7="0")                 # one column, no pad; back to (6, 6) from (10, 2)
    run(11, 2)                                         # and the default again, from the three-pass tables
    ctx.close()


# ---- closed-form vectors through the multi-pass kernels ------------------------------------------------------------------------------
# Random data never makes a butterfly difference exactly zero, never walks a sum along the 2q boundary of the lazy representation and
# never leaves a whole pass with a single non-zero row.  These vectors do, and their transforms are known in closed form, so the
# expected values are Python integers (pow), not the oracle.
R256 = 1 << 256


def _mont_rows(vals):
    """Python integers -> the Montgomery limbs the library computes on, [len, 4] u64"""
    return np.frombuffer(b"".join((v % Q * R256 % Q).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def _power_table(n, inverse):
    """row e = omega^e (forward) or omega^-e / n (inverse), e < n"""
    w = M.omega(n)
    v, out = 1, []
    if inverse:
        w, v = M.inv(w, Q), M.inv(n, Q)
    for _ in range(n):
        out.append(v)
        v = v * w % Q
    return _mont_rows(out)


@pytest.mark.parametrize("logn", [13, 14, 15, 16, 17, 18, 20])
def test_multi_pass_closed_form_vectors(ctx, logn):
    n = 1 << logn
    rnd = random.Random(0xC105ED + logn)
    c = rnd.randrange(1, Q)
    # impulses: index n - 1, and 2^b - 1 and 2^b for EVERY bit b, so both sides of every pass boundary whatever the split of the passes
    ks = [n - 1, 1, 3] + [(1 << b) - 1 for b in range(2, logn)] + [1 << b for b in range(1, logn)] + [rnd.randrange(n)]
    j = np.arange(n, dtype=np.int64)
    for inverse in (False, True):
        tab = _power_table(n, inverse)
        scale = M.inv(n, Q) if inverse else 1
        cols, want = [], []

        def column(nonzero, expect_rows):
            x = np.zeros((n, 4), dtype=np.uint64)
            for i, v in nonzero:
                x[i] = v
            cols.append(x)
            want.append(expect_rows)

        def sparse(rows):
            y = np.zeros((n, 4), dtype=np.uint64)
            for i, v in rows:
                y[i] = _mont_rows([v])[0]
            return y

        for cc in (c, Q - 1, 1):                                  # constant vectors: n c (or c) at index 0, zero elsewhere
            cols.append(np.tile(_mont_rows([cc]), (n, 1)))
            want.append(sparse([(0, cc * n * scale)]))
        alt = np.zeros((n, 4), dtype=np.uint64)                    # (0, q-1, 0, q-1, ...): (q-1) n/2 at 0 and n/2 at n/2 (omega^(n/2) = -1)
        alt[1::2] = _mont_rows([Q - 1])[0]
        cols.append(alt)
        want.append(sparse([(0, (Q - 1) * (n // 2) * scale), (n // 2, (n // 2) * scale)]))
        one, minus_one = _mont_rows([1])[0], _mont_rows([Q - 1])[0]
        for i, k in enumerate(ks):                                 # impulse at k: omega^(+-jk) (/ n); with value q - 1: the same shifted by n/2
            if i % 4 == 3:
                column([(k, minus_one)], tab[(j * k + n // 2) % n])
            else:
                column([(k, one)], tab[(j * k) % n])
        while len(cols) % 8:
            cols.append(np.zeros((n, 4), dtype=np.uint64))
            want.append(np.zeros((n, 4), dtype=np.uint64))
        # one column at a time for the first few, then batches of eight
        for b in range(4):
            got = bp.i_ntt_381(cols[b], ctx) if inverse else bp.ntt_381(cols[b], ctx)
            assert (got == want[b]).all(), (logn, inverse, "single column", b)
        for b in range(0, len(cols), 8):
            got = ctx.ntt_batch(np.stack(cols[b:b + 8]), inverse=inverse)
            for i in range(8):
                assert (got[i] == want[b + i]).all(), (logn, inverse, "batch of eight", b + i, np.nonzero((got[i] != want[b + i]).any(axis=1))[0][:4])

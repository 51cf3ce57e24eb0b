"""-m gpu: m cell claims reduced to the A | B record of a pairing check (bp_kzg_verify_cells_reduce, Setup.cell_pairing_inputs) and
decided against [tau^l]_2 (Setup.verify_cells).  Every claim and every expectation is made by tests/kzg_cells_model.py in Python
integers over the oracle's G1 (commitment [f(tau)] G, values by Horner, proof [q_k(tau)] G, the discrete logarithms of A and B);
none comes from the library.  Sizes (log_n, log_l): (7,3) and (9,6), the claims of three polynomials on one SRS with a repeated
cell index and the cells 0 and r - 1 among them."""
import ctypes as C
import random

import numpy as np
import pytest

import baby_plonk_rust_amd as bp
from baby_plonk_rust_amd import FR_BYTES_LE, FR_MONT
from tests import bigint_model as M
from tests import kzg_cells_model as CM
from tests import kzg_model as K

pytestmark = pytest.mark.gpu
Q = M.Q
ID96 = bytes([0x40]) + bytes(95)
TAU = 0x5EED0123456789ABCDEF0F1E2D3C4B5A69788796A5B4C3D2E1F00112233445566 % Q
PAIRS = ((7, 3), (9, 6))
NO_CLAIM = C.c_size_t(-1).value


@pytest.fixture(scope="module")
def ctx():
    c = bp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases(ctx):
    """per (log_n, log_l): the setup, and the model's claims (commitment scalar, k, values, proof scalar) of three polynomials,
    made once and left unchanged"""
    made = {}
    for log_n, log_l in PAIRS:
        n, l, rng = 1 << log_n, 1 << log_l, random.Random(64 * log_n + log_l)
        r = n // l
        setup = bp.Setup.generate_srs(n, TAU, ctx, tables=False)
        claims = []
        for lens, picks in ((n, (0, r - 1, 3)), (n - 5, (0, r // 2)), (l + 1, (r - 1, 3))):      # cell 3 and cells 0, r - 1 repeat
            f = [rng.randrange(Q) for _ in range(lens)]
            com = K.horner(f, TAU)
            for k in picks:
                values, pi = CM.cell(f, n, l, k, TAU)
                claims.append((com, k, values, pi))
        made[(log_n, log_l)] = (setup, n, l, claims)
    yield made
    for setup, _, _, _ in made.values():
        ctx.srs_free(setup.handle)


def records(claims):
    return [bp.CellOpening(K.point96(com), k, bp.scalars_from_ints(values), K.point96(pi)) for com, k, values, pi in claims]


def raw(ctx, handle, log_n, log_l, claims, weights, fmt=FR_BYTES_LE, checks=0, values_bytes=None, index=None, points=None):
    """bp_kzg_verify_cells_reduce itself with canonical bytes: (rc, out192, first_bad)"""
    m = len(claims)
    com, prf = points or (b"".join(K.point96(c[0]) for c in claims), b"".join(K.point96(c[3]) for c in claims))
    com, prf = np.frombuffer(com + bytes(1), dtype=np.uint8).copy(), np.frombuffer(prf + bytes(1), dtype=np.uint8).copy()
    idx = np.array(index if index is not None else [c[1] for c in claims] + [0], dtype=np.uint32)
    vb = values_bytes or b"".join(int(v).to_bytes(32, "little") for c in claims for v in c[2])
    vals = np.frombuffer(vb + bytes(32), dtype=np.uint8).copy()
    w = None if weights is None else np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in weights), dtype=np.uint8).copy()
    out, bad = np.full(192, 0xA5, dtype=np.uint8), C.c_size_t(12345)
    rc = ctx._lib.bp_kzg_verify_cells_reduce(ctx._h, handle, log_n, log_l, com.ctypes.data, idx.ctypes.data, vals.ctypes.data, prf.ctypes.data, m,
                                             None if w is None else w.ctypes.data, fmt, checks, out.ctypes.data, C.byref(bad))
    return rc, bytes(out), bad.value


@pytest.mark.parametrize("pair", PAIRS)
def test_reduce_matches_the_model(ctx, cases, pair):
    setup, n, l, claims = cases[pair]
    rng = random.Random(n + l)
    weights = [rng.getrandbits(128) | 1 << 127 for _ in claims]
    A, B = CM.reduce_scalars([c + (w,) for c, w in zip(claims, weights)], n, TAU)
    want = K.point96(A) + K.point96(B)
    assert (A * pow(TAU, l, Q) - B) % Q == 0                       # the model's own claims hold
    got = setup.cell_pairing_inputs(records(claims), n, bp.scalars_from_ints(weights))
    assert got[0] + got[1] == want
    assert setup.cell_pairing_inputs(records(claims), n, bp.scalars_from_ints(weights), checks=1) == got       # subgroup test on
    rc, out, bad = raw(ctx, setup.handle, *pair, claims, weights)                                   # canonical bytes
    assert rc == 0 and out == want and bad == NO_CLAIM
    # weights NULL: as bp_kzg_verify_reduce, every weight is 1 and only a single claim is accepted
    for c in (claims[0], claims[-1]):
        A1, B1 = CM.reduce_scalars([c + (1,)], n, TAU)
        got = setup.cell_pairing_inputs(records([c]), n)
        assert got[0] + got[1] == K.point96(A1) + K.point96(B1)
        rc, out, bad = raw(ctx, setup.handle, *pair, [c], None)
        assert rc == 0 and out == K.point96(A1) + K.point96(B1)
    rc, out, bad = raw(ctx, setup.handle, *pair, claims, None)
    assert rc == -1 and out == bytes([0xA5]) * 192
    rc, out, bad = raw(ctx, setup.handle, *pair, [], None)         # m = 0: two identities
    assert rc == 0 and out == ID96 + ID96 and bad == NO_CLAIM


@pytest.mark.parametrize("pair", PAIRS)
def test_verify_cells(ctx, cases, pair):
    setup, n, l, claims = cases[pair]
    r = n // l
    tau_l_g2, x_2 = bp.g2_mul_generator(pow(TAU, l, Q)), bp.g2_mul_generator(TAU)
    good = records(claims)
    for on_host in (True, False):
        assert setup.verify_cells(good, n, tau_l_g2, host=on_host) is True
    assert setup.verify_cells(good[0], n, tau_l_g2) is True         # a single claim, weight 1
    off = list(good)                                               # one value off by one
    v = list(claims[1][2])
    v[l - 1] = (v[l - 1] + 1) % Q
    off[1] = good[1]._replace(values=bp.scalars_from_ints(v))
    swapped = list(good)                                           # two proofs swapped between cells
    swapped[0], swapped[1] = good[0]._replace(proof=good[1].proof), good[1]._replace(proof=good[0].proof)
    moved = list(good)                                             # one claim's index changed to a neighbour
    moved[2] = good[2]._replace(index=(good[2].index + 1) % r)
    other = list(good)                                             # another polynomial's commitment
    other[0] = good[0]._replace(commitment=good[3].commitment)
    for name, bad in (("value", off), ("swap", swapped), ("index", moved), ("commitment", other)):
        assert setup.verify_cells(bad, n, tau_l_g2) is False, name
        assert setup.verify_cells(bad, n, tau_l_g2, host=False) is False, name
    assert setup.verify_cells(good, n, x_2) is False               # [tau]_2 where [tau^l]_2 belongs


def test_errors(ctx, cases):
    setup, n, l, claims = cases[(7, 3)]
    r, h = n // l, setup.handle
    weights = list(range(1, len(claims) + 1))
    index = [c[1] for c in claims]
    rc, out, bad = raw(ctx, h, 7, 3, claims, weights, index=index[:4] + [r] + index[5:])
    assert rc == -1 and bad == 4 and out == bytes([0xA5]) * 192                                      # cell_index >= r
    vb = b"".join(int(v).to_bytes(32, "little") for c in claims for v in c[2])
    at = 32 * (2 * l + 5)
    rc, out, bad = raw(ctx, h, 7, 3, claims, weights, values_bytes=vb[:at] + Q.to_bytes(32, "little") + vb[at + 32:])
    assert rc == -4 and bad == 2 and out == bytes([0xA5]) * 192                                      # a value >= q
    rc, out, bad = raw(ctx, h, 7, 3, claims, weights[:3] + [Q + 1] + weights[4:])
    assert rc == -4 and bad == 3                                                                     # a weight >= q
    com, prf = b"".join(K.point96(c[0]) for c in claims), b"".join(K.point96(c[3]) for c in claims)
    broken = prf[:96 * 5 + 95] + bytes([prf[96 * 5 + 95] ^ 1]) + prf[96 * 6:]
    rc, out, bad = raw(ctx, h, 7, 3, claims, weights, points=(com, broken))
    assert rc == -3 and bad == 5 and out == bytes([0xA5]) * 192                                      # a proof off the curve
    with pytest.raises(bp.BpError) as e:
        setup.cell_pairing_inputs(records(claims[:2]) + [records(claims[2:3])[0]._replace(index=r)], n, bp.scalars_from_ints([1, 2, 3]))
    assert e.value.code == -1 and e.value.index == 2
    lag = ctx.srs_lagrange(h, 3)
    small = bp.Setup.generate_srs(4, TAU, ctx, tables=False)
    try:
        assert raw(ctx, lag, 7, 3, claims, weights)[0] == -5                                         # a Lagrange SRS
        assert raw(ctx, small.handle, 7, 3, claims, weights)[0] == -6                                # fewer than l points
        assert raw(ctx, h, 3, 4, claims, weights)[0] == -1                                           # log_l > log_n
        assert raw(ctx, h, 24, 3, claims, weights)[0] == -10
        assert raw(ctx, 0xDEAD, 7, 3, claims, weights)[0] == -1
        assert raw(ctx, h, 7, 3, claims, weights, fmt=7)[0] == -1
    finally:
        ctx.srs_free(lag)
        ctx.srs_free(small.handle)

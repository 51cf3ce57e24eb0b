"""The KZG model of tests/kzg_model.py against itself, on the CPU: its two routes to an opening -- coefficients and synthetic
division, evaluations and the barycentric / pointwise formulas -- agree, on and off the domain, and the scalars of the batch check
satisfy a . tau = b for honest claims and for no claim with one field changed."""
import random

import pytest

from tests import bigint_model as M
from tests import kzg_model as K

Q = M.Q


def _poly(rng, n):
    coeffs = [rng.randrange(Q) for _ in range(n)]
    return coeffs, M.dft(coeffs)


@pytest.mark.parametrize("n", [1, 2, 4, 8, 64])
def test_quotient_routes_agree(n):
    """the Lagrange-form quotient evaluations are the DFT of the synthetic-division quotient; the values agree too"""
    rng = random.Random(n)
    coeffs, evals = _poly(rng, n)
    dom = K.domain(n)
    points = [rng.randrange(Q), 0, dom[0], dom[n // 2], dom[n - 1], M.omega(2 * n)] + (dom if n == 8 else [])      # every in-domain m for n = 8
    for z in points:
        assert K.barycentric(evals, z) == K.horner(coeffs, z)
        q = K.quotient_coeffs(coeffs, z) + [0]
        assert K.quotient_evals(evals, z) == M.dft(q)
        tau = rng.randrange(2, Q)
        assert K.horner(q, tau) == K.proof_scalar(K.horner(coeffs, tau), K.horner(coeffs, z), tau, z)


def test_open_routes_agree_for_many_polynomials():
    rng = random.Random(7)
    n, tau = 16, rng.randrange(2, Q)
    pairs = [_poly(rng, n) for _ in range(3)]
    for z in (rng.randrange(Q), K.domain(n)[5]):
        for nu in (rng.randrange(Q), 0, 1):
            assert K.open_monomial([c for c, _ in pairs], z, nu, tau) == K.open_lagrange([e for _, e in pairs], z, nu, tau)


def _claims(rng, m, count, tau):
    """honest claims: (z, ys, nu, r) and the discrete logarithms of their commitments and proofs"""
    claims, logs = [], []
    for i in range(m):
        # the last claim is the one the test tampers with: no constant there (a constant opens to itself at every z, with W = 0)
        polys = [[rng.randrange(Q) for _ in range(rng.randrange(2 if i == m - 1 else 0, 6))] for _ in range(count)]
        z, nu, r = rng.randrange(Q), rng.randrange(Q), rng.randrange(1, Q)
        ys, w = K.open_monomial(polys, z, nu, tau)
        claims.append((z, ys, nu, r))
        logs.append(([K.horner(p, tau) for p in polys], w))
    return claims, logs


def _holds(claims, logs, tau):
    c, w, g, a = K.reduce_scalars(claims)
    lhs = sum(ai * wi for ai, (_, wi) in zip(a, logs)) * tau
    rhs = g + sum(wi * wl for wi, (_, wl) in zip(w, logs)) + sum(x * cl for row, (cls, _) in zip(c, logs) for x, cl in zip(row, cls))
    return (lhs - rhs) % Q == 0


@pytest.mark.parametrize("m, count", [(1, 1), (2, 3), (5, 2)])
def test_reduce_scalars_decide_the_batch(m, count):
    rng = random.Random(100 * m + count)
    tau = rng.randrange(2, Q)
    claims, logs = _claims(rng, m, count, tau)
    assert _holds(claims, logs, tau)
    i = m - 1
    z, ys, nu, r = claims[i]
    cls, w = logs[i]
    tampered = [("y", (z, [(ys[0] + 1) % Q] + ys[1:], nu, r), logs[i]), ("z", ((z + 1) % Q, ys, nu, r), logs[i]),
                ("w", claims[i], (cls, (w + 1) % Q)), ("c", claims[i], ([(cls[0] + 1) % Q] + cls[1:], w))]
    if count > 1:
        tampered.append(("nu", (z, ys, (nu + 1) % Q, r), logs[i]))
    for what, claim, log in tampered:
        assert not _holds(claims[:i] + [claim], logs[:i] + [log], tau), what

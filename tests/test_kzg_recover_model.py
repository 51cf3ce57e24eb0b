"""CPU checks of tests/kzg_recover_model.py, the integer model behind every expectation of the recovery tests: against direct Lagrange
interpolation of the present points in O(N^2), and for the consistency property the C ABI reports as BP_ERR_ASSERT."""
import random

import pytest

from tests import kzg_cells_model as CM
from tests import kzg_recover_model as RM
from tests.bigint_model import Q, omega

SHAPES = [(1, 0), (2, 1), (3, 0), (3, 1), (3, 3), (4, 2), (5, 0), (5, 2)]


def draws(log_n, log_l, rnd):
    """presence sets of a shape: everything, one cell (where r > 1), half, and random ones, each with shuffled indices"""
    r = 1 << (log_n - log_l)
    counts = sorted({r, 1, max(r // 2, 1)} | {rnd.randrange(1, r + 1) for _ in range(3)})
    for m in counts:
        idx = rnd.sample(range(r), m)
        yield idx


def test_ntt_is_the_definition():
    rnd = random.Random(1)
    for n in (1, 2, 8):
        a, w = [rnd.randrange(Q) for _ in range(n)], omega(n)
        assert RM.ntt(a, w) == [sum(a[k] * pow(w, i * k, Q) for k in range(n)) % Q for i in range(n)]
        assert RM.interpolate(RM.evaluate(a, n)) == a
    f = [rnd.randrange(Q) for _ in range(8)]
    assert RM.cells_of(f, 8, 2) == [CM.cell_values(f, 8, 2, k) for k in range(4)]      # the cell order of the cell-proof model


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_recovers_the_polynomial(log_n, log_l):
    """cells of a polynomial of degree < d come back as that polynomial, with zeros from d on, for every presence set with m l >= d"""
    n, l, rnd = 1 << log_n, 1 << log_l, random.Random(100 * log_n + log_l)
    for idx in draws(log_n, log_l, rnd):
        m = len(idx)
        for d in sorted({1, m * l, rnd.randrange(1, m * l + 1)}):
            f = [rnd.randrange(Q) for _ in range(d)]
            cells = RM.cells_of(f, n, l)
            g, bad = RM.recover(n, l, idx, [cells[k] for k in idx], d)
            assert bad is None and g == f + [0] * (n - d), (idx, d)


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_is_lagrange_interpolation(log_n, log_l):
    """ARBITRARY values: g is the polynomial of degree < m l through the m l present points, by the O(N^2) definition"""
    n, l, rnd = 1 << log_n, 1 << log_l, random.Random(200 * log_n + log_l)
    for idx in draws(log_n, log_l, rnd):
        m = len(idx)
        cells = [[rnd.randrange(Q) for _ in range(l)] for _ in idx]
        xs = [x for k in idx for x in RM.cell_points(n, l, k)]
        want = RM.lagrange(xs, [v for row in cells for v in row])
        g, _ = RM.recover(n, l, idx, cells, m * l)
        assert g == want + [0] * (n - m * l), idx


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_one_wrong_value_is_seen(log_n, log_l):
    """with redundancy (m l > d) one corrupted value always leaves a non-zero coefficient in [d, m l): the error polynomial is a
    non-zero multiple of the vanishing polynomial of the other m l - 1 points, so its degree is exactly m l - 1 >= d"""
    n, l, rnd = 1 << log_n, 1 << log_l, random.Random(300 * log_n + log_l)
    for idx in draws(log_n, log_l, rnd):
        m = len(idx)
        if m * l < 2:
            continue
        d = rnd.randrange(1, m * l)
        f = [rnd.randrange(Q) for _ in range(d)]
        cells = RM.cells_of(f, n, l)
        given = [list(cells[k]) for k in idx]
        i, j = rnd.randrange(m), rnd.randrange(l)
        given[i][j] = (given[i][j] + rnd.randrange(1, Q)) % Q
        g, bad = RM.recover(n, l, idx, given, d)
        assert bad is not None and d <= bad < m * l and g[m * l - 1] != 0 and not any(g[m * l:]), (idx, d)
        assert RM.recover(n, l, idx, given, m * l)[1] is None      # no redundancy: nothing to see


def test_vanishing_sets():
    """zero exactly on the missing cells, never zero on the shifted domain; and Z on the whole domain takes the r values of Z_dom"""
    n, l = 32, 4
    r, w = n // l, omega(n)
    missing = [1, 4, 6]
    z_dom, z_cos = RM.vanishing_sets(n, l, missing)
    assert [k for k in range(r) if z_dom[k] == 0] == missing and all(z_cos)
    z = lambda x: eval_product(x, l, missing, n)
    assert [z(pow(w, t, Q)) for t in range(n)] == [z_dom[t % r] for t in range(n)]
    assert [z(RM.SHIFT * pow(w, t, Q) % Q) for t in range(n)] == [z_cos[t % r] for t in range(n)]
    assert RM.vanishing_sets(n, l, []) == ([1] * r, [1] * r)


def eval_product(x, l, missing, n):
    acc, w_r = 1, pow(omega(n), l, Q)
    for k in missing:
        acc = acc * (pow(x, l, Q) - pow(w_r, k, Q)) % Q
    return acc

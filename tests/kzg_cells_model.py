"""Python-integer model of KZG cell proofs with a known tau, the source of every expectation of the cell tests (none comes from the
library).  n = 2^log_n, l = 2^log_l, r = n / l, w = omega(n): cell k < r is the coset {w^(k + r j) : j < l}, its vanishing polynomial
x^l - a_k with a_k = w^(k l); the proof is the scalar q_k(tau) of the quotient by the schoolbook recurrence, the interpolant comes
from the closed form and is asserted equal to the remainder, and the batch check has the scalars of A and B."""
from tests.bigint_model import Q, omega
from tests.kzg_model import horner, point96  # noqa: F401  (point96: the records of the tests)


def div_binomial(coeffs, l, a):
    """f = q (x^l - a) + rem by the schoolbook recurrence q_i = f_{i+l} + a q_{i+l}: (q, rem) with len(rem) == l"""
    f = list(coeffs) + [0] * max(l - len(coeffs), 0)
    q = [0] * (len(f) - l)
    for i in range(len(q) - 1, -1, -1):
        q[i] = (f[i + l] + a * (q[i + l] if i + l < len(q) else 0)) % Q
    rem = [(f[i] + a * (q[i] if i < len(q) else 0)) % Q for i in range(l)]
    return q, rem


def cell_points(n, l, k):
    """the points of cell k in cell order: w^(k + r j), j < l"""
    w, r = omega(n), n // l
    return [pow(w, k + r * j, Q) for j in range(l)]


def cell_a(n, l, k):
    return pow(omega(n), k * l, Q)


def cell_values(coeffs, n, l, k):
    return [horner(coeffs, z) for z in cell_points(n, l, k)]


def quotient(coeffs, n, l, k):
    return div_binomial(coeffs, l, cell_a(n, l, k))[0]


def proof_scalar(coeffs, n, l, k, tau):
    """q_k(tau)"""
    return horner(quotient(coeffs, n, l, k), tau)


def interpolant(values, n, k):
    """the coefficients c_t = w^(-k t) l^-1 sum_j v_j zeta^(-j t), zeta = w^r, of the polynomial of degree < l with the given values on
    cell k (closed form)"""
    l = len(values)
    w, r = omega(n), n // l
    zeta_inv, w_inv, l_inv = pow(w, -r, Q), pow(w, -k, Q), pow(l, -1, Q)
    return [pow(w_inv, t, Q) * l_inv % Q * sum(v * pow(zeta_inv, j * t, Q) for j, v in enumerate(values)) % Q for t in range(l)]


def cell(coeffs, n, l, k, tau):
    """(values, q_k(tau)) of cell k, with the closed-form interpolant of the values asserted equal to the remainder of the division"""
    q, rem = div_binomial(coeffs, l, cell_a(n, l, k))
    values = cell_values(coeffs, n, l, k)
    assert interpolant(values, n, k) == rem
    return values, horner(q, tau)


def all_cells(coeffs, n, l, tau):
    """([values of cell k], [q_k(tau)]) for every k < n / l"""
    out = [cell(coeffs, n, l, k, tau) for k in range(n // l)]
    return [v for v, _ in out], [s for _, s in out]


def h_double_sum(coeffs, n, l, point_scalars):
    """h_m = sum_{j<l} sum_{u=0}^{r-2-m} f_{(m+1+u) l + j} P_{u l + j} over the scalars of ANY point set (no tau identity), m < r"""
    r, f = n // l, list(coeffs) + [0] * (n - len(coeffs))
    return [sum(f[(m + 1 + u) * l + j] * point_scalars[u * l + j] for j in range(l) for u in range(r - 1 - m)) % Q for m in range(r)]


def proofs_from_h(h, n, l):
    """pi_k = sum_m (w^l)^(k m) h_m"""
    wl, r = pow(omega(n), l, Q), n // l
    return [horner(h, pow(wl, k, Q)) for k in range(r)]


def reduce_scalars(claims, n, tau):
    """claims: (commitment scalar f(tau), k, values, proof scalar, rho) each -> the discrete logarithms (A, B) of
    A = sum rho pi and B = sum rho (C + a_k pi) - sum_t (sum_i rho_i c_it) P_t, P_t = tau^t G"""
    A = B = 0
    for com, k, values, pi, rho in claims:
        l = len(values)
        c = interpolant(values, n, k)
        A = (A + rho * pi) % Q
        B = (B + rho * (com + cell_a(n, l, k) * pi - horner(c, tau))) % Q
    return A, B

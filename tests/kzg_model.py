"""Python-integer model of KZG openings with a known tau, the source of every expectation of the KZG tests (none comes from the
library): values by Horner or by the barycentric formula, the proof as the scalar q(tau) = (g(tau) - y_g) / (tau - z), the quotient
itself by synthetic division and by the evaluation-form formulas, and the scalars of the batch check."""
from tests.bigint_model import Q, omega


def batch_inv(xs):
    """the inverses of non-zero xs from one inversion"""
    pre, acc = [], 1
    for x in xs:
        pre.append(acc)
        acc = acc * x % Q
    inv = pow(acc, -1, Q)
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        out[i] = inv * pre[i] % Q
        inv = inv * xs[i] % Q
    return out


def domain(n):
    w, out, x = omega(n), [], 1
    for _ in range(n):
        out.append(x)
        x = x * w % Q
    return out


def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % Q
    return acc


def barycentric(evals, x):
    """f(x) of the polynomial of degree < n with f(w^i) = evals[i], n = len(evals) a power of two; O(n)"""
    n, dom = len(evals), domain(len(evals))
    if x % Q in dom:
        return evals[dom.index(x % Q)] % Q
    inv = batch_inv([(x - d) % Q for d in dom])
    s = sum(f * d % Q * v for f, d, v in zip(evals, dom, inv)) % Q
    return (pow(x, n, Q) - 1) * pow(n, -1, Q) % Q * s % Q


def combine(vectors, nu):
    """sum_j nu^j v_j of vectors of any lengths (a shorter one is padded with zeros)"""
    out, p = [0] * max([len(v) for v in vectors] + [0]), 1
    for v in vectors:
        for i, x in enumerate(v):
            out[i] = (out[i] + p * x) % Q
        p = p * nu % Q
    return out


def proof_scalar(g_tau, y_g, tau, z):
    """q(tau) for q = (g - y_g) / (x - z); tau != z"""
    return (g_tau - y_g) * pow((tau - z) % Q, -1, Q) % Q


def open_monomial(polys, z, nu, tau):
    """(ys, q(tau)) of coefficient lists `polys` opened at z and combined by nu"""
    ys = [horner(p, z) for p in polys]
    y_g = sum(pow(nu, j, Q) * y for j, y in enumerate(ys)) % Q
    return ys, proof_scalar(horner(combine(polys, nu), tau), y_g, tau, z)


def open_lagrange(cols, z, nu, tau):
    """the same for columns of evaluations over the n-th roots of unity"""
    ys = [barycentric(c, z) for c in cols]
    y_g = sum(pow(nu, j, Q) * y for j, y in enumerate(ys)) % Q
    return ys, proof_scalar(barycentric(combine(cols, nu), tau), y_g, tau, z)


def quotient_coeffs(coeffs, z):
    """synthetic division of coeffs by x - z: the len - 1 quotient coefficients (none squeezed out)"""
    out, acc = [0] * max(len(coeffs) - 1, 0), 0
    for i in range(len(coeffs) - 1, 0, -1):
        acc = (coeffs[i] + acc * z) % Q
        out[i - 1] = acc
    return out


def quotient_evals(evals, z):
    """the evaluation-form route: q_i = (g_i - y) / (w^i - z); for z = w^m the closed form q_m = - sum_{i != m} q_i w^(i-m)"""
    n, dom, y = len(evals), domain(len(evals)), barycentric(evals, z)
    m = dom.index(z % Q) if z % Q in dom else None
    q = [0 if i == m else (evals[i] - y) * pow((dom[i] - z) % Q, -1, Q) % Q for i in range(n)]
    if m is not None:
        q[m] = -sum(q[i] * dom[(i - m) % n] for i in range(n) if i != m) % Q
    return q


def reduce_scalars(claims):
    """claims: (z, ys, nu, r) each -> (c [m][count], w [m], g, a [m]) with A = sum a_i W_i and B = sum c_ij C_ij + sum w_i W_i + g G"""
    c, w, a, g = [], [], [], 0
    for z, ys, nu, r in claims:
        row = [r * pow(nu, j, Q) % Q for j in range(len(ys))]
        c.append(row)
        w.append(r * z % Q)
        a.append(r % Q)
        g = (g - sum(x * y for x, y in zip(row, ys))) % Q
    return c, w, g, a


def point96(k):
    """[k] G as 96 bytes, from the oracle's G1"""
    from oracle import oracle as O
    return O.g1_bytes96(O.g1_mul(O.g1_generator(), O.fr_from_int(k % Q)))

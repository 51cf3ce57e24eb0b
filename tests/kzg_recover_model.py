"""Python-integer model of KZG cell recovery (csrc/kzg_recover.hpp), the source of every expectation of the recovery tests (none comes
from the library).  n = 2^log_n, l = 2^log_l, r = n / l, w = omega(n), w_r = w^l: cell k < r is the coset {w^(k + r j) : j < l} in cell
order.  Given m distinct cell indices with their values and a degree bound d, with M the missing indices and
Z(x) = prod_{k in M} (x^l - w_r^k):
  1  Z_dom[i] = prod_{k in M} (w_r^i - w_r^k), Z_cos[i] = prod_{k in M} (s^l w_r^i - w_r^k), i < r, s = 7
  2  E[i] = v_{k,j} Z_dom[k], k = i mod r, j = i div r, where cell k is present, else 0; inverse transform: the coefficients of f Z
  3  times s^i, forward transform, times 1 / Z_cos[i mod r], inverse transform, times s^-i: g, the interpolant of the present values
  4  the cells agree with a polynomial of degree < d exactly when coefficients d .. n - 1 of g are zero
The transforms are a recursive radix-2 NTT, so that shapes of a few thousand points stay within a second."""
from tests.bigint_model import Q, omega

SHIFT = 7


def ntt(a, w):
    """[sum_k a_k w^(i k)] for i < len(a), a power of two, w a primitive len(a)-th root of unity"""
    n = len(a)
    if n == 1:
        return list(a)
    even, odd = ntt(a[0::2], w * w % Q), ntt(a[1::2], w * w % Q)
    out, t = [0] * n, 1
    for i in range(n // 2):
        x = t * odd[i] % Q
        out[i], out[i + n // 2] = (even[i] + x) % Q, (even[i] - x) % Q
        t = t * w % Q
    return out


def evaluate(coeffs, n):
    """f(w^i), i < n, of a polynomial of at most n coefficients"""
    return ntt(list(coeffs) + [0] * (n - len(coeffs)), omega(n))


def interpolate(values):
    """the coefficients of the polynomial of degree < n with the n values f(w^i)"""
    n = len(values)
    n_inv = pow(n, -1, Q)
    return [v * n_inv % Q for v in ntt(values, pow(omega(n), -1, Q))]


def cells_of(coeffs, n, l):
    """all r cells of a polynomial, cell order: cells[k][j] = f(w^(k + r j))"""
    natural, r = evaluate(coeffs, n), n // l
    return [[natural[k + r * j] for j in range(l)] for k in range(r)]


def vanishing_sets(n, l, missing):
    """(Z_dom, Z_cos), r values each, by the products of step 1"""
    r = n // l
    w_r = pow(omega(n), l, Q)
    roots, base = [pow(w_r, k, Q) for k in missing], pow(SHIFT, l, Q)
    sets = []
    for b in (1, base):
        out = []
        for i in range(r):
            x, acc = b * pow(w_r, i, Q) % Q, 1
            for a in roots:
                acc = acc * (x - a) % Q
            out.append(acc)
        sets.append(out)
    return sets[0], sets[1]


def recover(n, l, indices, cells, d):
    """(g, first_bad): the n coefficients of the interpolant of the given cells (indices[i] names cells[i], any order) and the lowest
    index >= d at which it is not zero, or None: then g[:d] is THE polynomial of degree < d with these cells"""
    r = n // l
    assert len(set(indices)) == len(indices) and all(0 <= k < r for k in indices) and 1 <= d <= min(len(indices) * l, n)
    slot = {k: i for i, k in enumerate(indices)}
    missing = [k for k in range(r) if k not in slot]
    z_dom, z_cos = vanishing_sets(n, l, missing)
    assert all((z_dom[k] == 0) == (k in missing) for k in range(r)) and all(z_cos)
    e = [cells[slot[i % r]][i // r] * z_dom[i % r] % Q if i % r in slot else 0 for i in range(n)]
    g = interpolate(e)
    if missing:
        s_inv = pow(SHIFT, -1, Q)
        on_coset = ntt([c * pow(SHIFT, i, Q) % Q for i, c in enumerate(g)], omega(n))
        z_inv = [pow(z, -1, Q) for z in z_cos]
        g = [c * pow(s_inv, i, Q) % Q for i, c in enumerate(interpolate([v * z_inv[i % r] % Q for i, v in enumerate(on_coset)]))]
    return g, next((i for i in range(d, n) if g[i]), None)


def lagrange(xs, ys):
    """the coefficients of the polynomial of degree < len(xs) through the points (xs[i], ys[i]), by the definition: O(N^2)"""
    big_n = len(xs)
    master = [1]                                                   # prod (x - x_i), low coefficient first
    for x in xs:
        master = [((master[t - 1] if t else 0) - x * (master[t] if t < len(master) else 0)) % Q for t in range(len(master) + 1)]
    out = [0] * big_n
    for x, y in zip(xs, ys):
        q, carry = [0] * big_n, 0                                  # master / (x - x_i) by synthetic division
        for t in range(big_n, 0, -1):
            carry = (master[t] + x * carry) % Q
            q[t - 1] = carry
        denom = 1
        for other in xs:
            if other != x:
                denom = denom * (x - other) % Q
        scale = y * pow(denom, -1, Q) % Q
        out = [(o + scale * c) % Q for o, c in zip(out, q)]
    return out


def cell_points(n, l, k):
    w, r = omega(n), n // l
    return [pow(w, k + r * j, Q) for j in range(l)]

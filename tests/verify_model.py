"""src/verifier.rs:80-192 restated as SCALARS in Python integers: the coefficient of every base of the verifier's two pairing
arguments.  TEST INFRASTRUCTURE for bp_verify_reduce (tests/test_verify_host.py, tests/test_gpu_verify.py); nothing here
calls the library.

  A_j = W_zeta_j + mu_j W_zeta_omega_j
  B_j = zeta_j W_zeta_j + mu_j zeta_j omega W_zeta_omega_j + F_j - E_j                               (verifier.rs:187-191)

L_1(zeta) and PI(zeta) are evaluated BY THE DEFINITION the reference uses (verifier.rs:91-104: the Lagrange column through
i_ntt, then coeffs_evaluate), so zeta = omega^i needs no special case; the closed form omega^i (zeta^n - 1) / (n (zeta -
omega^i)) is cross-checked against it wherever its denominator is not zero."""
import os

from tests import bigint_model as M

Q = M.Q
K1, K2 = 2, 3                                                    # verifier.rs:76-77
POINT_FIELDS = ("a_1", "b_1", "c_1", "z_1", "t_lo_1", "t_mid_1", "t_hi_1", "w_zeta_1", "w_zeta_omega_1")    # verifier.rs:23-40
EVAL_FIELDS = ("a_bar", "b_bar", "c_bar", "s1_bar", "s2_bar", "z_omega_bar")
VK_FIELDS = ("ql", "qr", "qm", "qo", "qc", "s1", "s2", "s3")     # the order bp_circuit_commitments writes
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g1_compressed_valid_test_vectors.dat")


def fixture_points():
    """the crate's fixture: record i = enc48(i G), i < 1000 (record 0 is the identity)"""
    blob = open(FIXTURE, "rb").read()
    assert len(blob) == 48000
    return [blob[48 * i: 48 * i + 48] for i in range(1000)]


def lagrange_column_eval(column, n, zeta):
    """Polynomial::new(column, Lagrange).i_ntt().coeffs_evaluate(zeta) (verifier.rs:95-96, 103-104)"""
    coeffs = M.dft([v % Q for v in column] + [0] * (n - len(column)), inverse=True)
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * zeta + c) % Q
    return acc


def l1_and_pi(n, zeta, public, by_definition=True):
    """(L_1(zeta), PI(zeta)) by the definition; the closed form is asserted to agree where it exists.  by_definition=False
    (the timing tool at n = 2^10, where the O(n^2) interpolation takes seconds) returns the closed form alone and refuses a
    zeta on a root."""
    z_h = (pow(zeta, n, Q) - 1) % Q
    om = M.omega(n)
    lag = lambda i: pow(om, i, Q) * z_h % Q * pow(n * (zeta - pow(om, i, Q)) % Q, Q - 2, Q) % Q
    if not by_definition:
        assert z_h, "the closed form does not exist on a root"
        return lag(0), sum((-x) * lag(i) for i, x in enumerate(public)) % Q
    l1 = lagrange_column_eval([1], n, zeta)
    pi = lagrange_column_eval([(-x) % Q for x in public], n, zeta)
    if z_h:
        assert l1 == lag(0) and pi == sum((-x) * lag(i) for i, x in enumerate(public)) % Q
    else:
        idx = [i for i in range(n) if pow(om, i, Q) == zeta % Q]
        assert len(idx) == 1 and l1 == (1 if idx[0] == 0 else 0)
        assert pi == ((-public[idx[0]]) % Q if idx[0] < len(public) else 0)
    return l1, pi


def coefficients(n, ev, ch, public, by_definition=True):
    """ev: a b c s1 s2 zw; ch: beta gamma alpha zeta nu mu; public: the vector handed to verify().
    Returns (proof9, a2, shared9): coefficients in B_j of the nine proof points (POINT_FIELDS order), coefficients in A_j of
    W_zeta and W_zeta_omega, coefficients in B_j of QL QR QM QO QC S1 S2 S3 G."""
    a, b, c, s1, s2, zw = ev
    beta, gamma, alpha, zeta, nu, mu = ch
    rl = lambda s, o: (s + o * beta + gamma) % Q
    l1, pi = l1_and_pi(n, zeta, public, by_definition)
    zn = pow(zeta, n, Q)
    z_h = (zn - 1) % Q
    om = M.omega(n)
    r_0 = (pi - l1 * alpha * alpha - alpha * rl(a, s1) * rl(b, s2) * (c + gamma) * zw) % Q                  # :114-120
    c_z = (rl(a, zeta) * rl(b, K1 * zeta) * rl(c, K2 * zeta) * alpha + l1 * alpha * alpha + mu) % Q       # :137-143
    c_s3 = (-(rl(a, s1) * rl(b, s2) * alpha * beta * zw)) % Q                                             # :144-149
    e = (nu * a + nu**2 * b + nu**3 * c + nu**4 * s1 + nu**5 * s2 + mu * zw - r_0) % Q                    # :172-179
    proof9 = [nu % Q, pow(nu, 2, Q), pow(nu, 3, Q), c_z, (-z_h) % Q, (-z_h * zn) % Q, (-z_h * zn * zn) % Q,   # :150-153, 164-167
              zeta % Q, mu * zeta * om % Q]                                                               # :187-191
    shared9 = [a % Q, b % Q, a * b % Q, c % Q, 1, pow(nu, 4, Q), pow(nu, 5, Q), c_s3, (-e) % Q]           # :136, 168-169
    return proof9, [1, mu % Q], shared9


def reduce_dlogs(n, records, vk_dlogs, publics, weights, challenges):
    """records: [(nine discrete logs, six evaluations)]; every point is k G.  Returns (a, b) with A = a G, B = b G."""
    a_sum = b_sum = 0
    for j, (dl, ev) in enumerate(records):
        rho = 1 if weights is None else weights[j]
        p9, a2, s9 = coefficients(n, ev, challenges[j], publics[j] if publics else [])
        a_sum += rho * (a2[0] * dl[7] + a2[1] * dl[8])
        b_sum += rho * (sum(cf * k for cf, k in zip(p9, dl)) + sum(cf * k for cf, k in zip(s9, list(vk_dlogs) + [1])))
    return a_sum % Q, b_sum % Q


def pairing_sides(n, pts, ev, ch, vk, public):
    """the two G1Affine arguments of verifier.rs:187-191 for ONE proof of arbitrary points (affine tuples or None)"""
    p9, a2, s9 = coefficients(n, ev, ch, public)
    mul = lambda k, pt: M.ec_mul(k % Q, pt) if pt is not None and k % Q else None
    A = M.ec_add(mul(a2[0], pts["w_zeta_1"]), mul(a2[1], pts["w_zeta_omega_1"]))
    B = None
    for cf, f in zip(p9, POINT_FIELDS):
        B = M.ec_add(B, mul(cf, pts[f]))
    for cf, f in zip(s9, VK_FIELDS):
        B = M.ec_add(B, mul(cf, vk[f]))
    B = M.ec_add(B, mul(s9[8], (M.GX, M.GY)))
    return A, B


def challenges_of(record624):
    """Verifier::compute_challengs (verifier.rs:193-209) through the Python twin of the transcript; also the number of draws
    (challenge_bytes calls) each challenge needed"""
    from tests.merlin_transcript import PlonkTranscript

    class Counting(PlonkTranscript):
        def __init__(self):
            super().__init__()
            self.draws, self._n = [], 0
            inner = self.t.challenge_bytes

            def counted(label, n):
                self._n += 1
                return inner(label, n)
            self.t.challenge_bytes = counted

        def get_and_append_challenge(self, label):
            self._n = 0
            v = super().get_and_append_challenge(label)
            self.draws.append(self._n)
            return v

    t = Counting()
    p = [record624[48 * k: 48 * k + 48] for k in range(9)]
    e = [int.from_bytes(record624[432 + 32 * k: 464 + 32 * k], "little") for k in range(6)]
    beta, gamma = t.round_1(p[0], p[1], p[2])
    alpha = t.round_2(p[3])
    zeta = t.round_3(p[4], p[5], p[6])
    nu = t.round_4(*e)
    mu = t.round_5(p[7], p[8])
    return [beta, gamma, alpha, zeta, nu, mu], t.draws


def le32(values):
    return b"".join((v % Q).to_bytes(32, "little") for v in values)


def public_circuit(n, gates):
    """three public-input rows (x, -, -) with QL = 1 and -x in the public-input column, then a chain of multiplications
    m_k = m_{k-1} * y_k (qm = -1, qo = 1); sigma columns from the restated front-end (program.rs:76-147)"""
    from tests.circuit_frontend import make_gate_polynomials, make_s_polynomials
    wires = [("p0", None, None), ("p1", None, None), ("p2", None, None), ("p0", "p1", "m0"), ("m0", "p2", "m1")]
    wires += [("m%d" % (k - 1), "y%d" % k, "m%d" % k) for k in range(2, gates)]
    sel = [(1, 0, 0, 0, 0)] * 3 + [(0, 0, -1, 1, 0)] * gates
    pk = make_gate_polynomials(sel, n)
    _, sig = make_s_polynomials(wires, n)
    pk.update(s1=sig[0], s2=sig[1], s3=sig[2])

    def witness(rnd):
        val = {"p0": rnd.randrange(Q), "p1": rnd.randrange(Q), "p2": rnd.randrange(Q)}
        val["m0"] = val["p0"] * val["p1"] % Q
        val["m1"] = val["m0"] * val["p2"] % Q
        for k in range(2, gates):
            val["y%d" % k] = rnd.randrange(Q)
            val["m%d" % k] = val["m%d" % (k - 1)] * val["y%d" % k] % Q
        cols = [[val[row[j]] if row[j] else 0 for row in wires] + [0] * (n - len(wires)) for j in range(3)]
        public = [val["p0"], val["p1"], val["p2"]]
        return cols, public, [(-x) % Q for x in public] + [0] * (n - 3)
    return pk, witness

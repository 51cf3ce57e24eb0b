"""Helpers shared by the prover's tests, on the CPU and on the GPU, and by tools/fuzz_prover.py: the reference's prove() restated over
a backend of tests/prover_rounds.py, the verifier's final equation in G1 for a known tau, and the 624-byte proof format.  TEST
INFRASTRUCTURE: Python integers and the oracle only; no call into the library."""
import numpy as np

from oracle import oracle as O
from tests import bigint_model as M
from tests import prover_rounds as PR

Q = M.Q


def decode(b96):
    return None if b96[0] & 0x40 else (int.from_bytes(b96[:48], "big"), int.from_bytes(b96[48:], "big"))


def g1_only_verify(n, tau, proof, ev, ch, vk, public_inputs):
    """src/verifier.rs:80-192 with the pairing check e(A, [tau]_2) == e(B, [1]_2) replaced by tau * A == B"""
    beta, gamma, alpha, zeta, nu, mu = (ch[k] for k in ("beta", "gamma", "alpha", "zeta", "nu", "mu"))
    mul = lambda k, P: M.ec_mul(k % Q, P) if P is not None else None
    add = M.ec_add
    neg = lambda P: None if P is None else (P[0], (-P[1]) % M.P)
    z_h_zeta = (pow(zeta, n, Q) - 1) % Q
    omega = M.omega(n)
    # L_i(zeta) = omega^i (zeta^n - 1) / (n (zeta - omega^i)): the value verifier.rs:91-104 obtains by i_ntt + coeffs_evaluate
    lag = lambda i: pow(omega, i, Q) * z_h_zeta % Q * pow(n * (zeta - pow(omega, i, Q)) % Q, Q - 2, Q) % Q
    l_1_zeta = lag(0)
    pi_eval = sum((-x) * lag(i) for i, x in enumerate(public_inputs)) % Q
    a_bar, b_bar, c_bar, s1_bar, s2_bar, zw_bar = (ev[k] for k in ("a_bar", "b_bar", "c_bar", "s1_bar", "s2_bar", "z_omega_bar"))
    rl = lambda s, o: (s + o * beta + gamma) % Q
    r_0 = (pi_eval - l_1_zeta * alpha * alpha - alpha * rl(a_bar, s1_bar) * rl(b_bar, s2_bar) * (c_bar + gamma) * zw_bar) % Q
    d1 = add(add(add(add(mul(a_bar * b_bar, vk["qm"]), mul(a_bar, vk["ql"])), mul(b_bar, vk["qr"])), mul(c_bar, vk["qo"])), vk["qc"])
    d2 = mul(rl(a_bar, zeta) * rl(b_bar, PR.K1 * zeta) * rl(c_bar, PR.K2 * zeta) * alpha + l_1_zeta * alpha * alpha + mu, proof["z_1"])
    d3 = mul(rl(a_bar, s1_bar) * rl(b_bar, s2_bar) * alpha * beta * zw_bar, vk["s3"])
    d4 = mul(z_h_zeta, add(add(proof["t_lo_1"], mul(pow(zeta, n, Q), proof["t_mid_1"])), mul(pow(zeta, 2 * n, Q), proof["t_hi_1"])))
    d = add(add(add(d1, d2), neg(d3)), neg(d4))
    f = d
    for k, P in enumerate((proof["a_1"], proof["b_1"], proof["c_1"], vk["s1"], vk["s2"]), start=1):
        f = add(f, mul(pow(nu, k, Q), P))
    e_scalar = (nu * a_bar + nu**2 * b_bar + nu**3 * c_bar + nu**4 * s1_bar + nu**5 * s2_bar + mu * zw_bar - r_0) % Q
    e = M.ec_mul(e_scalar)
    lhs = mul(tau, add(proof["w_zeta_1"], mul(mu, proof["w_zeta_omega_1"])))
    rhs = add(add(add(mul(zeta, proof["w_zeta_1"]), mul(mu * zeta * omega, proof["w_zeta_omega_1"])), f), neg(e))
    return lhs == rhs


def prove_with_blinding(B, n, cols, pk, public, blinders, z_fn=None, logging=True):
    """src/prover.rs:106-176 with the blinders as an argument (the reference draws them from thread_rng, :108-110) and the
    Fiat-Shamir challenges from the Merlin transcript exactly as src/transcript.rs derives them"""
    from tests.merlin_transcript import PlonkTranscript
    comp = lambda b96: M.enc48(decode(b96))
    tr = PlonkTranscript()
    st = PR.ProverState(B, n, pk, blinders, logging)
    proof = {}
    proof["a_1"], proof["b_1"], proof["c_1"] = PR.round_1(st, cols[0], cols[1], cols[2], public)
    st.rand["beta"], st.rand["gamma"] = tr.round_1(comp(proof["a_1"]), comp(proof["b_1"]), comp(proof["c_1"]))
    proof["z_1"] = PR.round_2(st)
    st.rand["alpha"] = tr.round_2(comp(proof["z_1"]))
    proof["t_lo_1"], proof["t_mid_1"], proof["t_hi_1"] = PR.round_3(st)
    st.rand["zeta"] = tr.round_3(comp(proof["t_lo_1"]), comp(proof["t_mid_1"]), comp(proof["t_hi_1"]))
    ev = PR.round_4(st)
    st.rand["nu"] = tr.round_4(ev["a_bar"], ev["b_bar"], ev["c_bar"], ev["s1_bar"], ev["s2_bar"], ev["z_omega_bar"])
    proof["w_zeta_1"], proof["w_zeta_omega_1"] = PR.round_5(st)
    order = ("a_1", "b_1", "c_1", "z_1", "t_lo_1", "t_mid_1", "t_hi_1", "w_zeta_1", "w_zeta_omega_1")
    blob = b"".join(comp(proof[k]) for k in order) + b"".join(
        ev[k].to_bytes(32, "little") for k in ("a_bar", "b_bar", "c_bar", "s1_bar", "s2_bar", "z_omega_bar"))
    return proof, ev, blob


def compute_challenges(proof, ev):
    """src/verifier.rs:193-209"""
    from tests.merlin_transcript import PlonkTranscript
    comp = lambda b96: M.enc48(decode(b96))
    tr = PlonkTranscript()
    beta, gamma = tr.round_1(comp(proof["a_1"]), comp(proof["b_1"]), comp(proof["c_1"]))
    alpha = tr.round_2(comp(proof["z_1"]))
    zeta = tr.round_3(comp(proof["t_lo_1"]), comp(proof["t_mid_1"]), comp(proof["t_hi_1"]))
    nu = tr.round_4(ev["a_bar"], ev["b_bar"], ev["c_bar"], ev["s1_bar"], ev["s2_bar"], ev["z_omega_bar"])
    mu = tr.round_5(comp(proof["w_zeta_1"]), comp(proof["w_zeta_omega_1"]))
    return dict(beta=beta, gamma=gamma, alpha=alpha, zeta=zeta, nu=nu, mu=mu)


def split_proof(blob):
    names = ("a_1", "b_1", "c_1", "z_1", "t_lo_1", "t_mid_1", "t_hi_1", "w_zeta_1", "w_zeta_omega_1")
    pts = {k: M.dec48(blob[48 * i: 48 * i + 48]) for i, k in enumerate(names)}
    ev = {k: int.from_bytes(blob[432 + 32 * i: 464 + 32 * i], "little")
          for i, k in enumerate(("a_bar", "b_bar", "c_bar", "s1_bar", "s2_bar", "z_omega_bar"))}
    return pts, ev


def proof_challenges(blob):
    from tests.merlin_transcript import PlonkTranscript
    tr = PlonkTranscript()
    pt = lambda i: blob[48 * i: 48 * i + 48]
    ev = [int.from_bytes(blob[432 + 32 * i: 464 + 32 * i], "little") for i in range(6)]
    beta, gamma = tr.round_1(pt(0), pt(1), pt(2))
    alpha = tr.round_2(pt(3))
    zeta = tr.round_3(pt(4), pt(5), pt(6))
    nu = tr.round_4(*ev)
    mu = tr.round_5(pt(7), pt(8))
    return dict(beta=beta, gamma=gamma, alpha=alpha, zeta=zeta, nu=nu, mu=mu)


def oracle_srs(powers, tau):
    """setup.rs:12-31: sequential cur *= tau"""
    pts, cur, t = [], O.g1_generator(), O.fr_from_int(tau)
    for _ in range(powers):
        pts.append(cur)
        cur = O.g1_mul(cur, t)
    return np.stack(pts)

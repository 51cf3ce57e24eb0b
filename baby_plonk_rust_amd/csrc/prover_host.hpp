// prover_host.hpp -- everything the native prover (prover.hip) decides or computes on the host from numbers alone: the constants of
// the quotient coset, which path a proof takes, and the scalars rounds 3 and 5 hand to their kernels.  Pure field arithmetic over
// host_codec.hpp; no HIP call and no bp_ctx: tests/test_prover_host.py compiles it alone and checks it on the CPU against closed forms.
#pragma once
#include "host_codec.hpp"

namespace bp {

inline fr_t fmul(const fr_t& a, const fr_t& b) { fr_t r; Fr::mul(r, a, b); return r; }
inline fr_t fadd(const fr_t& a, const fr_t& b) { fr_t r; Fr::add(r, a, b); return r; }
inline fr_t fsub(const fr_t& a, const fr_t& b) { fr_t r; Fr::sub(r, a, b); return r; }
inline fr_t fneg(const fr_t& a) { fr_t r; Fr::neg(r, a); return r; }
inline fr_t finv(const fr_t& a) { fr_t r; fr_invert(r, a); return r; }

// ---- the quotient coset g <w_4n> of a circuit of n = 2^log_n gates, as the union of the four cosets s_j <w_n>, s_j = g w_4n^j
constexpr uint64_t COSET_GEN = 7;        // generator of Fr^* (scalar.rs GENERATOR): g^n w^j != 1 for every n-th-root coset used here
struct CosetConsts {
  fr_t g, ginv, w4n, gn, i4, iinv;       // g = 7, 1/g, w_4n, g^n, i4 = w_4n^n (a primitive fourth root of unity), 1/i4
  fr_t s[4], s_inv[4], sn[4];            // s_j, 1/s_j, s_j^n = g^n i4^j: X^n on the whole of coset j
  fr_t zh_inv[4];                        // 1 / (X^n - 1) there: period 4 along g w_4n^i
  fr_t scale[4];                         // g^(-n m) / 4: the recombination of the four residues (prover_kernels.hpp, coset_recombine)
  fr_t n_inv;                            // 1 / n: every coefficient of L1 (l1_coeff = i_ntt(e_0), prover.rs:430)
};
inline CosetConsts coset_consts(uint32_t log_n) {
  const uint64_t n = (uint64_t)1 << log_n;
  CosetConsts c;
  c.g = fr_from_u64(COSET_GEN), c.ginv = finv(c.g), c.n_inv = finv(fr_from_u64(n));
  (void)host_root_of_unity(c.w4n, 4 * n);                            // 4n = 2^k, never 0
  c.gn = fr_pow_u64(c.g, n), c.i4 = fr_pow_u64(c.w4n, n), c.iinv = finv(c.i4);
  const fr_t gn_inv = finv(c.gn);
  for (int j = 0; j < 4; j++) {
    c.s[j] = j ? fmul(c.s[j - 1], c.w4n) : c.g;
    c.sn[j] = j ? fmul(c.sn[j - 1], c.i4) : c.gn;
    c.scale[j] = j ? fmul(c.scale[j - 1], gn_inv) : finv(fr_from_u64(4));
    c.s_inv[j] = finv(c.s[j]);
    c.zh_inv[j] = finv(fsub(c.sn[j], Fr::one()));
  }
  return c;
}

// ---- which path a proof takes: the ONE place the defaults live.  A knob (experiment build only, docs/EXPERIMENTS.md section H) overrides a
// size threshold, never the feasibility: staging needs a host witness on one device, the side stream and the coset split exclude
// each other, the early coset work needs the split.
//   staged  BP_PROVE_STAGED       round 1 uploads the host witness itself, column by column beside the commitments (ctx.hpp, ProveStaged), from
//                                 2^18 gates: 2.2 ms of uploads at 2^20 gates leave 0.8 on the proof's path.
//   split   BP_PROVE_COSET_SPLIT  round 3 by coset over the circuit's shares (group contexts; BP_PROVE_COSET_ONE: one device)
//   side    BP_PROVE_SIDE         round 3's challenge-free transforms on the side stream beside round 2.  That pays while the
//                                 commitment's accumulation leaves the chip partly idle: below 2^20 gates (-0.05 .. -0.15 ms per proof
//                                 at 2^16 / 2^18).  From 2^20 msm_accumulate fills every SIMD for 2 ms and whatever runs beside it only
//                                 delays its workgroups (+0.4 ms per proof), so all five transforms stay in round 3 there.
//   early   BP_PROVE_COSET_EARLY  a, b, c, PI go to the shares right after round 1's blinding, beside the commitments (0: in round 3)
struct ProveKnobs { int staged = -1, split = -1, side = -1, early = -1; };      // -1 unset, 0, 1
struct ProvePaths { bool staged, split, side, early; };
inline int knob_tristate(const char* v) { return v && (*v == '0' || *v == '1') ? *v - '0' : -1; }      // anything else counts as unset
inline ProvePaths prove_paths(uint32_t log_n, bool host_witness, bool group, bool has_split, const ProveKnobs& k) {
  ProvePaths p;
  p.staged = host_witness && !group && (k.staged >= 0 ? k.staged == 1 : log_n >= 18);
  p.split = has_split && k.split != 0;
  p.side = !p.split && (k.side >= 0 ? k.side == 1 : log_n < 20);
  p.early = p.split && k.early != 0;
  return p;
}

// ---- round 3: the scalar arguments of quotient_coset and coset_recombine (prover_kernels.hpp; k1 = 2, k2 = 3, prover.rs:99-100)
struct QuotientArgs { fr_t alpha, alpha2, beta, gamma, beta_k1, beta_k2, one, zh_inv[4]; };
inline QuotientArgs quotient_args(const fr_t& alpha, const fr_t& beta, const fr_t& gamma, const fr_t zh_inv[4]) {
  QuotientArgs q = {alpha, fmul(alpha, alpha), beta, gamma, fmul(beta, fr_from_u64(2)), fmul(beta, fr_from_u64(3)), Fr::one(), {}};
  for (int j = 0; j < 4; j++) q.zh_inv[j] = zh_inv[j];
  return q;
}
struct RecombineArgs { fr_t scale[4], iinv; };
inline RecombineArgs recombine_args(const CosetConsts& c) { return {{c.scale[0], c.scale[1], c.scale[2], c.scale[3]}, c.iinv}; }

// ---- round 5 (prover.rs:543-634): the opening numerator  r(x) + nu (a - a_bar) + ... + nu^5 (s2 - s2_bar)  as ONE linear
// combination sum_k c[k] p_k(x) + constant over the polynomials, in this order:
//   qm ql qr qo qc | z | s3 | t_lo t_mid t_hi | a b c s1 s2
// r = qm a_bar b_bar + ql a_bar + qr b_bar + qo c_bar + PI(zeta) + qc                                                     (r1)
//     + alpha ((a_bar + beta zeta + gamma)(b_bar + 2 beta zeta + gamma)(c_bar + 3 beta zeta + gamma) z
//              - (a_bar + beta s1_bar + gamma)(b_bar + beta s2_bar + gamma)(c_bar + beta s3 + gamma) zw_bar)              (r2)
//     + alpha^2 (z - 1) L1(zeta)  -  (zeta^n - 1)(t_lo + zeta^n t_mid + zeta^2n t_hi)                                     (r3, r4)
struct Round5Scalars { fr_t c[15], constant; };
inline Round5Scalars round5_scalars(uint64_t n, const fr_t& alpha, const fr_t& beta, const fr_t& gamma, const fr_t& zeta, const fr_t& nu,
                                    const fr_t& a_bar, const fr_t& b_bar, const fr_t& c_bar, const fr_t& s1_bar, const fr_t& s2_bar,
                                    const fr_t& zw_bar, const fr_t& pi_zeta) {
  const fr_t one = Fr::one(), zeta_n = fr_pow_u64(zeta, n), zh_zeta = fsub(zeta_n, one);
  // L1(zeta) = (1/n) sum_i zeta^i  (l1_coeff.coeffs_evaluate, :590)
  const fr_t l1_zeta = big_eq(zeta, one) ? one : fmul(zh_zeta, finv(fmul(fr_from_u64(n), fsub(zeta, one))));
  const fr_t bz = fmul(beta, zeta), alpha2 = fmul(alpha, alpha);
  const fr_t f_a = fadd(fadd(a_bar, bz), gamma), f_b = fadd(fadd(b_bar, fmul(bz, fr_from_u64(2))), gamma), f_c = fadd(fadd(c_bar, fmul(bz, fr_from_u64(3))), gamma);
  const fr_t g_a = fadd(fadd(a_bar, fmul(s1_bar, beta)), gamma), g_b = fadd(fadd(b_bar, fmul(s2_bar, beta)), gamma);
  const fr_t perm_s = fmul(alpha, fmul(fmul(g_a, g_b), zw_bar));                     // alpha (..)(..) z_omega_bar
  Round5Scalars r;
  r.c[0] = fmul(a_bar, b_bar); r.c[1] = a_bar; r.c[2] = b_bar; r.c[3] = c_bar; r.c[4] = one;
  r.c[5] = fadd(fmul(alpha, fmul(fmul(f_a, f_b), f_c)), fmul(alpha2, l1_zeta));      // z: alpha r2 and alpha^2 r3
  r.c[6] = fneg(fmul(perm_s, beta));                                                 // s3: -(s3 beta + c_bar + gamma) (..)(..) zw_bar
  r.c[7] = fneg(zh_zeta);                                                            // -r4
  r.c[8] = fneg(fmul(zeta_n, zh_zeta));
  r.c[9] = fneg(fmul(fmul(zeta_n, zeta_n), zh_zeta));
  const fr_t bars[5] = {a_bar, b_bar, c_bar, s1_bar, s2_bar};
  fr_t nu_j = one, open_const = Fr::zero();
  for (int j = 0; j < 5; j++) {                                                      // + nu (a - a_bar) + ... (:623-634)
    nu_j = fmul(nu_j, nu);
    r.c[10 + j] = nu_j;
    open_const = fadd(open_const, fmul(nu_j, bars[j]));
  }
  r.constant = fsub(fsub(fsub(pi_zeta, fmul(perm_s, fadd(c_bar, gamma))), fmul(alpha2, l1_zeta)), open_const);
  return r;
}

}  // namespace bp

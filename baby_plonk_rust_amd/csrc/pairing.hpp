// pairing.hpp -- the optimal ate pairing check of BLS12-381 on top of tower.hpp: the line evaluation, the Miller loop over two
// (G1 point, prepared G2 point) terms and the final exponentiation (pairings.rs:48-176, 554-606, 668-707).  __host__ __device__
// templates over the workspace type: the host check (capi_pairing.hip) and the kernels (pairing_kernels.hpp) run these lines.
//
// A prepared G2 point is PAIRING_LINES = 68 triples of Fp2, one per doubling or addition step of the loop over the bits of |x| / 2
// (g2_host.hpp computes them); the loop here only evaluates them at a G1 point and accumulates.
#pragma once
#include "g1_check.hpp"
#include "tower.hpp"

namespace bp {

constexpr int PAIRING_LINES = 68;
constexpr int PAIRING_TABLE_FP2 = 3 * PAIRING_LINES;
// Fp12 variables of a workspace that runs the whole check: f and seven more for the final exponentiation
constexpr int PAIRING_VARS = 8;
constexpr int PAIRING_SLOTS = tw_slots(PAIRING_VARS);

// One 96-byte G1 record of a pairing check, given as its 24 words as they sit in memory (G1Affine::from_uncompressed_unchecked,
// g1.rs:273-322, then is_on_curve and, where asked, is_torsion_free): canonical coordinates, the flag rules, y^2 = x^3 + 4, the
// subgroup.  out: the device affine form, (0, 0) for the identity and for a rejected record.  Returns 0 or the reason (g1_check.hpp).
// The ONE definition for the host check and the decode kernel.
BP_HD uint32_t pairing_decode_g1_words(g1_affine& out, const uint32_t w[24], bool subgroup) {
  fp_t x, y, t;
#pragma unroll
  for (int k = 0; k < 12; k++) {                                   // big-endian bytes -> little-endian limbs
    x.l[k] = __builtin_bswap32(w[11 - k]);
    y.l[k] = __builtin_bswap32(w[23 - k]);
  }
  const uint32_t flags = x.l[11] >> 29;                            // compression | infinity | sort
  x.l[11] &= 0x1fffffffu;
  out.x = out.y = Fp::zero();
  if (!big_sub(t, x, Fp::modulus()) || !big_sub(t, y, Fp::modulus()) || (flags & 0b101)) return G1_BAD_ENCODING;
  if (flags & 0b010) return big_is_zero(x) && big_is_zero(y) ? 0 : G1_BAD_ENCODING;
  g1_affine p;
  Fp::to_mont(p.x, x);
  Fp::to_mont(p.y, y);
  fp_t lhs, rhs, b4 = Fp::one();
  Fp::sqr(lhs, p.y);
  Fp::sqr(rhs, p.x);
  Fp::mul(rhs, rhs, p.x);
  Fp::dbl(b4, b4);
  Fp::dbl(b4, b4);
  Fp::add(rhs, rhs, b4);
  if (!big_eq(lhs, rhs)) return G1_NOT_ON_CURVE;
  if (subgroup && !g1_is_torsion_free(p)) return G1_NOT_IN_SUBGROUP;
  out = p;
  return 0;
}

// f *= line(P): the triple (l0, l1, l2) becomes the sparse element l2 + (l1 P.x) v + (l0 P.y) v w
template <class W>
BP_HD void pairing_ell(W w, int f, const fp2_t* line, const g1_affine& p) {
  fp2_t t;
  w.st(TW_LINE, line[2]);
  fp2_mul_fp(t, line[1], p.x);
  w.st(TW_LINE + 1, t);
  fp2_mul_fp(t, line[0], p.y);
  w.st(TW_LINE + 2, t);
  fp12w_mul_by_014(w, f);
}

// f = the Miller loop of (p0, tab0) and (p1, tab1); a term whose G1 point is the identity (0, 0) is dropped, as multi_miller_loop
// drops it.  The top bit of |x| / 2 starts the loop; each of the other 62 bits is: the doubling lines, the addition lines where
// the bit is set, one squaring of f shared by both terms.  A last doubling line and the conjugation (x < 0) end it.
template <class W>
BP_HD void pairing_miller2(W w, int f, const fp2_t* tab0, const g1_affine& p0, const fp2_t* tab1, const g1_affine& p1) {
  const bool use0 = !g1_affine_is_identity(p0), use1 = !g1_affine_is_identity(p1);
  constexpr uint64_t HALF_X = TOWER_BLS_X_ABS >> 1;
  fp12w_set_one(w, f);
  int line = 0;
#pragma unroll 1
  for (int b = 61; b >= -1; b--) {
    const int n_lines = b >= 0 && ((HALF_X >> b) & 1) ? 2 : 1;
#pragma unroll 1
    for (int k = 0; k < n_lines; k++, line++) {
      if (use0) pairing_ell(w, f, tab0 + 3 * line, p0);
      if (use1) pairing_ell(w, f, tab1 + 3 * line, p1);
    }
    if (b >= 0) fp12w_sqr(w, f, f);
  }
  fp12w_conjugate(w, f, f);
}

// f = f^e for the exponent e of MillerLoopResult::final_exponentiation: the easy part f^((p^6 - 1)(p^2 + 1)), then the hard part, a
// multiple of (p^4 - p^2 + 1) / q, as the chain in x and p of pairings.rs:142-171, on cyclotomic squarings.  v0..v6 are seven
// further variables of the workspace, all distinct from f and from each other.  A zero f (no Miller loop produces one) gives zero.
// The exponent of the hard part, read off the chain below with m the output of the easy part and x the curve parameter:
//     p^0 : x^5 - 2 x^4 + 2 x^2 - x + 3        (v4:  m^(x^5 - 2x^4 + 2x^2) * m^(2 - x) * m)
//     p^1 : x^4 - 2 x^3 + 2 x - 1              (v6:  m^(x^4 - 2x^3 + 2x) / m)
//     p^2 : x^3 - 2 x^2 + x                    (v3:  m^x * m^(x^3 - 2x^2))
//     p^3 : x^2 - 2 x + 1                      (v1:  m^(x^2 - 2x) * m)
// i.e. l0 + l1 p + l2 p^2 + l3 p^3 with l3 = (x - 1)^2, l2 = x l3, l1 = x l2 - l3, l0 = x l1 + 3, which equals 3 (p^4 - p^2 + 1) / q
// (Hayashida, Hayasaka, Teruya, eprint 2020/875; tests/test_tower_host.py checks the identity in integers).  The factor 3 keeps every
// coefficient an integer polynomial in x and does not change which inputs map to one (3 does not divide q).
template <class W>
BP_HD void pairing_final_exponentiation(W w, int f, int v0, int v1, int v2, int v3, int v4, int v5, int v6) {
  // easy part: v2 = (conj(f) / f)^(p^2 + 1)
  fp12w_conjugate(w, v0, f);
  fp12w_invert(w, v1, f);
  fp12w_mul(w, v1, v0, v1);
  fp12w_frobenius(w, v2, v1);
  fp12w_frobenius(w, v2, v2);
  fp12w_mul(w, v2, v2, v1);                       // m, in the cyclotomic subgroup from here on
  // hard part
  fp12w_cyclotomic_sqr(w, v1, v2);
  fp12w_conjugate(w, v1, v1);                     // m^-2
  fp12w_cyclotomic_exp(w, v3, v2);                // m^x
  fp12w_cyclotomic_sqr(w, v4, v3);                // m^2x
  fp12w_mul(w, v5, v1, v3);                       // m^(x - 2)
  fp12w_cyclotomic_exp(w, v1, v5);                // m^(x^2 - 2x)
  fp12w_cyclotomic_exp(w, v0, v1);                // m^(x^3 - 2x^2)
  fp12w_cyclotomic_exp(w, v6, v0);                // m^(x^4 - 2x^3)
  fp12w_mul(w, v6, v6, v4);                       // m^(x^4 - 2x^3 + 2x)
  fp12w_cyclotomic_exp(w, v4, v6);                // m^(x^5 - 2x^4 + 2x^2)
  fp12w_conjugate(w, v5, v5);                     // m^(2 - x)
  fp12w_mul(w, v5, v5, v2);
  fp12w_mul(w, v4, v4, v5);                       // the p^0 term
  fp12w_conjugate(w, v5, v2);                     // m^-1
  fp12w_mul(w, v1, v1, v2);
  fp12w_frobenius(w, v1, v1);
  fp12w_frobenius(w, v1, v1);
  fp12w_frobenius(w, v1, v1);                     // the p^3 term
  fp12w_mul(w, v6, v6, v5);
  fp12w_frobenius(w, v6, v6);                     // the p^1 term
  fp12w_mul(w, v3, v3, v0);
  fp12w_frobenius(w, v3, v3);
  fp12w_frobenius(w, v3, v3);                     // the p^2 term
  fp12w_mul(w, v3, v3, v1);
  fp12w_mul(w, v3, v3, v6);
  fp12w_mul(w, f, v3, v4);
}

}  // namespace bp

// g1_check.hpp -- what G1Affine::from_compressed (g1.rs:326-331) computes on top of the checks of the uncompressed decoder:
// the square root that recovers y (Fp::sqrt, fp.rs:324-340), the flag rules of from_compressed_unchecked (g1.rs:337-390), the
// subgroup test (is_torsion_free, g1.rs:401-411), and the inverse encoding (G1Affine::to_compressed, g1.rs:221-244).
// Everything is __host__ __device__ with ONE algorithm on both sides (no host/device split as fp_invert has): the CPU test
// (tests/test_srs_compressed_host.py) compiles exactly the code the kernels of srs_kernels.hpp run.
// Variable time: the reference is constant-time (CtOption); these branch on the point (identity, rejection).  SRS points are public.
#pragma once
#include "g1.hpp"

namespace bp {

// limb i of (p + 1) / 4 = (p >> 2) + 1 (p = 3 mod 4, no carry out of limb 0): the square-root exponent, 379 bits
BP_HD constexpr uint32_t fp_sqrt_exp(int i) {
  return ((FpParams::mod(i) >> 2) | (i < 11 ? FpParams::mod(i + 1) << 30 : 0u)) + (i == 0 ? 1u : 0u);
}
// limb i of (p + 1) / 2 = (p >> 1) + 1: y is lexicographically largest iff y >= (p + 1) / 2 (fp.rs:229-248)
BP_HD constexpr uint32_t fp_half_up(int i) {
  return ((FpParams::mod(i) >> 1) | (i < 11 ? FpParams::mod(i + 1) << 31 : 0u)) + (i == 0 ? 1u : 0u);
}
// beta, a primitive cube root of unity in Fp, canonical: 2^((p-1)/3) (2 is not a cube), of it and its square the one with
// phi(G) = -[x^2] G for phi(x, y) = (beta x, y) -- the endomorphism of g1.rs:394-399
BP_TABLE(fp_beta_canonical, 0xfffefffeu, 0x2e01ffffu, 0x620a0002u, 0xde17d813u, 0xe6f89688u, 0xddb3a93bu, 0x6a0f77eau, 0xba69c607u,
         0xdf76ce51u, 0x5f19672fu, 0x00000000u, 0x00000000u)
// |x| for the BLS parameter x = -0xd201000000010000 (BLS_X, BLS_X_IS_NEGATIVE)
constexpr uint64_t BLS_X_ABS = 0xd201000000010000ull;

// y canonical: y > (p - 1) / 2
BP_HD bool fp_lexicographically_largest(const fp_t& y_canonical) {
  fp_t h, t;
#pragma unroll
  for (int i = 0; i < 12; i++) h.l[i] = fp_half_up(i);
  return big_sub(t, y_canonical, h) == 0;
}

// s = a^((p+1)/4); returns s^2 == a (Montgomery in and out).  Fixed 3-bit windows, most significant first: 127 windows (the top
// one is 001), so 6 products for the table a^1 .. a^7, 3 x 126 squarings, one product per non-zero window (115 of 126) and the
// check: 500 Montgomery products against 607 for square-and-multiply (378 + 228 + 1).  The table (7 x 12 limbs) is only indexed
// by compile-time constants -- the digit picks its entry through selects -- so it stays in registers: no scratch.
BP_HD bool fp_sqrt(fp_t& s, const fp_t& a) {
  fp_t tab[7];                                               // tab[j] = a^(j + 1)
  tab[0] = a;
  Fp::sqr(tab[1], a);
#pragma unroll
  for (int j = 2; j < 7; j++) Fp::mul(tab[j], tab[j - 1], a);
  // the exponent shifted left by 3: window k (bits 380 - 3k .. 378 - 3k) is in bits 383..381 after k further shifts by 3
  fp_t e;
#pragma unroll
  for (int i = 0; i < 12; i++) e.l[i] = (fp_sqrt_exp(i) << 3) | (i ? fp_sqrt_exp(i - 1) >> 29 : 0u);
  auto pick = [&](fp_t& m, uint32_t d) {                     // m = a^d, d in 1..7
    m = tab[0];
#pragma unroll
    for (int j = 1; j < 7; j++) big_select(m, d == (uint32_t)(j + 1), tab[j], m);
  };
  fp_t r;
  pick(r, e.l[11] >> 29);
#pragma unroll 1
  for (int k = 1; k < 127; k++) {
#pragma unroll
    for (int i = 11; i > 0; i--) e.l[i] = (e.l[i] << 3) | (e.l[i - 1] >> 29);
    e.l[0] <<= 3;
    Fp::sqr(r, r);
    Fp::sqr(r, r);
    Fp::sqr(r, r);
    const uint32_t d = e.l[11] >> 29;
    if (d) {
      fp_t m;
      pick(m, d);
      Fp::mul(r, r, m);
    }
  }
  s = r;
  fp_t t;
  Fp::sqr(t, r);
  return big_eq(t, a);
}

// Reasons a compressed record is rejected (0 = accepted); the kernels report (index << 2) | reason
constexpr uint32_t G1_BAD_ENCODING = 1, G1_NOT_ON_CURVE = 2, G1_NOT_IN_SUBGROUP = 3;

// from_compressed_unchecked (g1.rs:337-390) of one 48-byte record given as its 12 little-endian 32-bit words as they sit in memory
// (bytes 4j .. 4j+3 in word j).  out: the device affine form (Montgomery; the identity is (0, 0), also for a rejected record).
BP_HD uint32_t g1_decode48(g1_affine& out, const uint32_t w[12]) {
  fp_t x;
#pragma unroll
  for (int k = 0; k < 12; k++) x.l[k] = __builtin_bswap32(w[11 - k]);     // big-endian bytes -> little-endian limbs
  const uint32_t flags = x.l[11] >> 29;                     // compression | infinity | sort = bits 7, 6, 5 of byte 0
  x.l[11] &= 0x1fffffffu;
  out.x = Fp::zero();
  out.y = Fp::zero();
  fp_t t;
  if (!(flags & 4) || !big_sub(t, x, Fp::modulus())) return G1_BAD_ENCODING;    // compression flag clear, or x >= p (fp.rs:179-190)
  if (flags & 2) return (flags & 1) || !big_is_zero(x) ? G1_BAD_ENCODING : 0;   // identity: 0xc0 then zeros, nothing else
  fp_t xm, rhs, b4 = Fp::one(), y;
  Fp::to_mont(xm, x);
  Fp::sqr(rhs, xm);
  Fp::mul(rhs, rhs, xm);
  Fp::dbl(b4, b4);
  Fp::dbl(b4, b4);
  Fp::add(rhs, rhs, b4);                                    // x^3 + 4
  if (!fp_sqrt(y, rhs)) return G1_NOT_ON_CURVE;
  Fp::from_mont(t, y);
  if (fp_lexicographically_largest(t) != ((flags & 1) != 0)) Fp::neg(y, y);    // y.lexicographically_largest() ^ sort_flag
  out.x = xm;
  out.y = y;
  return 0;
}

// G1Affine::to_compressed (g1.rs:221-244) of a device affine point into the 12 words of its 48-byte record
BP_HD void g1_encode48(uint32_t w[12], const g1_affine& p) {
  fp_t x, y;
  Fp::from_mont(x, p.x);
  Fp::from_mont(y, p.y);
  const bool inf = g1_affine_is_identity(p);
  x.l[11] |= inf ? 0xc0000000u : (0x80000000u | (fp_lexicographically_largest(y) ? 0x20000000u : 0u));
#pragma unroll
  for (int k = 0; k < 12; k++) w[11 - k] = __builtin_bswap32(x.l[k]);
}

// r = [|x|] p: G1Projective::mul_by_x (g1.rs:777-795) without its final negation.  The reference walks the bits of |x| from the
// bottom; here the top bit is p itself and the other 63 are doublings with an addition of p at the 5 other set bits: 63 x 8 +
// 5 x 12 = 564 products on the complete formulas, which keep the identity the identity.
BP_HD void g1_mul_by_x(g1_proj& r, const g1_proj& p) {
  g1_proj acc = p;
#pragma unroll 1
  for (int i = 62; i >= 0; i--) {
    g1_double(acc, acc);
    if ((BLS_X_ABS >> i) & 1) g1_add(acc, acc, p);
  }
  r = acc;
}

// is_torsion_free (g1.rs:401-411): phi(P) == -[x^2] P.  Both mul_by_x negate, so the signs cancel: [|x|^2] P (two g1_mul_by_x)
// is compared projectively with -phi(P) = (beta x, -y).  The identity passes.  1 132 products.
BP_HD bool g1_is_torsion_free(const g1_affine& p) {
  g1_proj q = g1_from_affine(p);
#pragma unroll 1
  for (int k = 0; k < 2; k++) g1_mul_by_x(q, q);
  fp_t beta, bx, ny, t, u;
#pragma unroll
  for (int i = 0; i < 12; i++) beta.l[i] = fp_beta_canonical(i);
  Fp::to_mont(beta, beta);
  Fp::mul(bx, p.x, beta);
  Fp::neg(ny, p.y);
  Fp::mul(t, bx, q.z);
  Fp::mul(u, ny, q.z);
  return g1_affine_is_identity(p) || (!big_is_zero(q.z) && big_eq(t, q.x) && big_eq(u, q.y));
}

}  // namespace bp

// g2_host.hpp -- G2 of BLS12-381 (y^2 = x^3 + 4 (u + 1) over Fp2) on the HOST only: the 192-byte wire format, the curve and subgroup
// tests, Jacobian doubling / addition / scalar multiplication, and the prepared line coefficients the Miller loop consumes
// (pairing.hpp).  No G2 arithmetic runs on the GPU: both G2 arguments of every pairing check are fixed, so the device only reads
// two tables of PAIRING_TABLE_FP2 Fp2 each.  Variable time: every input is public.
#pragma once
#include <stdint.h>
#include <string.h>

#include "host_codec.hpp"
#include "pairing.hpp"

namespace bp {

struct g2_affine {
  fp2_t x, y;
  bool infinity;
};
// Jacobian coordinates: (X / Z^2, Y / Z^3); Z = 0 is the identity
struct g2_jac {
  fp2_t x, y, z;
};

// the fixed generator (g2.rs:210), Montgomery limbs
BP_TABLE(g2_gen_x0, 0x02940a10u, 0xf5f28fa2u, 0x87b4961au, 0xb3f5fb26u, 0x3e2ae580u, 0xa1a893b5u, 0x1a3caee9u, 0x9894999du, 0x1863366bu,
         0x6f67b763u, 0x4350bcd7u, 0x05819192u)
BP_TABLE(g2_gen_x1, 0x9e23f606u, 0xa5a9c075u, 0xbccd60c3u, 0xaaa0c59du, 0xe2867806u, 0x3bb17e18u, 0x8541b367u, 0x1b1ab6ccu, 0xf2158547u,
         0xc2b6ed0eu, 0x7360edf3u, 0x11922a09u)
BP_TABLE(g2_gen_y0, 0x60494c4au, 0x4c730af8u, 0x5e369c5au, 0x597cfa1fu, 0xaa0a635au, 0xe7e6856cu, 0x6e0d495fu, 0xbbefb5e9u, 0xf0ef25a2u,
         0x07d3a975u, 0x7e80dae5u, 0x0083fd8eu)
BP_TABLE(g2_gen_y1, 0xdf64b05du, 0xadc0fc92u, 0x2b1461dcu, 0x18aa270au, 0x3be4eba0u, 0x86adac6au, 0xc93da33au, 0x79495c4eu, 0xa43ccaedu,
         0xe7175850u, 0x63de1bf2u, 0x0b2bc2a1u)
BP_FP_CONST(fp_g2_gen_x0, g2_gen_x0)
BP_FP_CONST(fp_g2_gen_x1, g2_gen_x1)
BP_FP_CONST(fp_g2_gen_y0, g2_gen_y0)
BP_FP_CONST(fp_g2_gen_y1, g2_gen_y1)

inline g2_affine g2_generator() { return g2_affine{fp2_t{fp_g2_gen_x0(), fp_g2_gen_x1()}, fp2_t{fp_g2_gen_y0(), fp_g2_gen_y1()}, false}; }
inline g2_affine g2_affine_identity() { return g2_affine{fp2_zero(), fp2_one(), true}; }
inline g2_jac g2_jac_identity() { return g2_jac{fp2_zero(), fp2_one(), fp2_zero()}; }
inline bool g2_jac_is_identity(const g2_jac& p) { return fp2_is_zero(p.z); }
inline g2_jac g2_from_affine(const g2_affine& p) { return p.infinity ? g2_jac_identity() : g2_jac{p.x, p.y, fp2_one()}; }

// ---- 192 bytes: x.c1 | x.c0 | y.c1 | y.c0, each 48 big-endian bytes, the three flag bits of G1 in the top of byte 0
// G2Affine::to_uncompressed (g2.rs:284-303)
inline void g2_encode192(uint8_t out[192], const g2_affine& p) {
  memset(out, 0, 192);
  if (p.infinity) {
    out[0] = 0x40;
    return;
  }
  const fp_t* c[4] = {&p.x.c1, &p.x.c0, &p.y.c1, &p.y.c0};
  for (int k = 0; k < 4; k++) {
    fp_t v;
    Fp::from_mont(v, *c[k]);
    fp_to_be48_host(out + 48 * k, v);
  }
}
// G2Affine::from_uncompressed_unchecked (g2.rs:305-330): canonical coordinates and the flag rules, NO curve check
inline bool g2_decode192(g2_affine& out, const uint8_t in[192]) {
  uint8_t buf[192];
  memcpy(buf, in, 192);
  const uint32_t flags = buf[0] >> 5;
  buf[0] &= 0x1f;
  fp_t v[4], t;
  bool all_zero = true;
  for (int k = 0; k < 4; k++) {
    v[k] = fp_from_be48_host(buf + 48 * k);
    if (!big_sub(t, v[k], Fp::modulus())) return false;
    all_zero = all_zero && big_is_zero(v[k]);
  }
  if (flags & 0b101) return false;
  if (flags & 0b010) {
    if (!all_zero) return false;
    out = g2_affine_identity();
    return true;
  }
  Fp::to_mont(out.x.c1, v[0]);
  Fp::to_mont(out.x.c0, v[1]);
  Fp::to_mont(out.y.c1, v[2]);
  Fp::to_mont(out.y.c0, v[3]);
  out.infinity = false;
  return true;
}
// y^2 = x^3 + 4 (u + 1); the identity passes
inline bool g2_on_curve(const g2_affine& p) {
  if (p.infinity) return true;
  fp2_t lhs, rhs, b = fp2_one();
  fp2_dbl(b, b);
  fp2_dbl(b, b);
  fp2_mul_by_nonresidue(b, b);
  fp2_sqr(lhs, p.y);
  fp2_sqr(rhs, p.x);
  fp2_mul(rhs, rhs, p.x);
  fp2_add(rhs, rhs, b);
  return fp2_eq(lhs, rhs);
}

// ---- group law
// 2 P for a = 0: with A = X^2, B = Y^2, C = B^2, D = 2 ((X + B)^2 - A - C), E = 3 A: X' = E^2 - 2 D, Y' = E (D - X') - 8 C, Z' = 2 Y Z
inline void g2_double(g2_jac& r, const g2_jac& p) {
  fp2_t A, B, C, D, E, t;
  g2_jac o;
  fp2_sqr(A, p.x);
  fp2_sqr(B, p.y);
  fp2_sqr(C, B);
  fp2_add(D, p.x, B);
  fp2_sqr(D, D);
  fp2_sub(D, D, A);
  fp2_sub(D, D, C);
  fp2_dbl(D, D);
  fp2_dbl(E, A);
  fp2_add(E, E, A);
  fp2_sqr(o.x, E);
  fp2_sub(o.x, o.x, D);
  fp2_sub(o.x, o.x, D);
  fp2_mul(o.z, p.y, p.z);
  fp2_dbl(o.z, o.z);
  fp2_sub(t, D, o.x);
  fp2_mul(o.y, E, t);
  fp2_dbl(C, C);
  fp2_dbl(C, C);
  fp2_dbl(C, C);
  fp2_sub(o.y, o.y, C);
  r = o;                                   // Z = 0 gives Z' = 0: the identity stays the identity
}
inline void g2_add(g2_jac& r, const g2_jac& a, const g2_jac& b) {
  if (g2_jac_is_identity(a)) {
    r = b;
    return;
  }
  if (g2_jac_is_identity(b)) {
    r = a;
    return;
  }
  fp2_t z1z1, z2z2, u1, u2, s1, s2, H, I, J, rr, V, t;
  fp2_sqr(z1z1, a.z);
  fp2_sqr(z2z2, b.z);
  fp2_mul(u1, a.x, z2z2);
  fp2_mul(u2, b.x, z1z1);
  fp2_mul(s1, a.y, b.z);
  fp2_mul(s1, s1, z2z2);
  fp2_mul(s2, b.y, a.z);
  fp2_mul(s2, s2, z1z1);
  if (fp2_eq(u1, u2)) {
    if (fp2_eq(s1, s2))
      g2_double(r, a);
    else
      r = g2_jac_identity();
    return;
  }
  g2_jac o;
  fp2_sub(H, u2, u1);
  fp2_dbl(I, H);
  fp2_sqr(I, I);
  fp2_mul(J, H, I);
  fp2_sub(rr, s2, s1);
  fp2_dbl(rr, rr);
  fp2_mul(V, u1, I);
  fp2_sqr(o.x, rr);
  fp2_sub(o.x, o.x, J);
  fp2_sub(o.x, o.x, V);
  fp2_sub(o.x, o.x, V);
  fp2_sub(t, V, o.x);
  fp2_mul(o.y, rr, t);
  fp2_mul(t, s1, J);
  fp2_dbl(t, t);
  fp2_sub(o.y, o.y, t);
  fp2_add(o.z, a.z, b.z);
  fp2_sqr(o.z, o.z);
  fp2_sub(o.z, o.z, z1z1);
  fp2_sub(o.z, o.z, z2z2);
  fp2_mul(o.z, o.z, H);
  r = o;
}
// [k] P, k as nlimbs 32-bit limbs (little endian), double-and-add from the top bit
inline g2_jac g2_mul(const g2_affine& p, const uint32_t* k, int nlimbs) {
  const g2_jac base = g2_from_affine(p);
  g2_jac acc = g2_jac_identity();
  for (int i = 32 * nlimbs - 1; i >= 0; i--) {
    g2_double(acc, acc);
    if ((k[i >> 5] >> (i & 31)) & 1) g2_add(acc, acc, base);
  }
  return acc;
}
inline g2_affine g2_to_affine(const g2_jac& p) {
  if (g2_jac_is_identity(p)) return g2_affine_identity();
  fp2_t zi, zi2;
  fp2_invert(zi, p.z);
  fp2_sqr(zi2, zi);
  g2_affine r;
  fp2_mul(r.x, p.x, zi2);
  fp2_mul(zi2, zi2, zi);
  fp2_mul(r.y, p.y, zi2);
  r.infinity = false;
  return r;
}
// [q] P == 0, plainly (g2.rs uses the psi endomorphism for the same answer); once per call on one point
inline bool g2_is_torsion_free(const g2_affine& p) {
  uint32_t q[8];
  for (int i = 0; i < 8; i++) q[i] = FrParams::mod(i);
  return g2_jac_is_identity(g2_mul(p, q, 8));
}

// ---- the lines of the Miller loop (Costello, Lange, Naehrig, eprint 2010/354, the a = 0 doubling and mixed addition in Jacobian
// coordinates with the tangent / chord through the point kept).  A triple (l0, l1, l2) stands for the line l2 + l1 x_P v + l0 y_P v w.
// tangent at R, then R = 2 R
inline void g2_line_double(g2_jac& r, fp2_t line[3]) {
  fp2_t A, B, C, D, E, F, zz, t;
  fp2_sqr(A, r.x);
  fp2_sqr(B, r.y);
  fp2_sqr(C, B);
  fp2_sqr(zz, r.z);
  fp2_add(D, r.x, B);
  fp2_sqr(D, D);
  fp2_sub(D, D, A);
  fp2_sub(D, D, C);
  fp2_dbl(D, D);                           // 4 X Y^2
  fp2_dbl(E, A);
  fp2_add(E, E, A);                        // 3 X^2
  fp2_sqr(F, E);
  // l2 = (X + E)^2 - A - F - 4 B = 2 X E - 4 Y^2 = 6 X^3 - 4 Y^2
  fp2_add(t, r.x, E);
  fp2_sqr(t, t);
  fp2_sub(t, t, A);
  fp2_sub(t, t, F);
  fp2_dbl(line[2], B);
  fp2_dbl(line[2], line[2]);
  fp2_sub(line[2], t, line[2]);
  // l1 = -2 E Z^2
  fp2_mul(t, E, zz);
  fp2_dbl(t, t);
  fp2_neg(line[1], t);
  g2_jac o;
  fp2_sub(o.x, F, D);
  fp2_sub(o.x, o.x, D);
  fp2_add(o.z, r.z, r.y);
  fp2_sqr(o.z, o.z);
  fp2_sub(o.z, o.z, B);
  fp2_sub(o.z, o.z, zz);                   // 2 Y Z
  fp2_sub(t, D, o.x);
  fp2_mul(o.y, t, E);
  fp2_dbl(C, C);
  fp2_dbl(C, C);
  fp2_dbl(C, C);
  fp2_sub(o.y, o.y, C);
  // l0 = 2 Z' Z^2
  fp2_mul(t, o.z, zz);
  fp2_dbl(line[0], t);
  r = o;
}
// chord through R and Q, then R = R + Q (R != +-Q, R and Q not the identity: true along the loop for a point of prime order)
inline void g2_line_add(g2_jac& r, const g2_affine& q, fp2_t line[3]) {
  fp2_t zz, yy, U, S2, H, HH, I, J, rr, V, t, u;
  fp2_sqr(zz, r.z);
  fp2_sqr(yy, q.y);
  fp2_mul(U, q.x, zz);                     // x_Q Z^2
  fp2_add(S2, q.y, r.z);
  fp2_sqr(S2, S2);
  fp2_sub(S2, S2, yy);
  fp2_sub(S2, S2, zz);
  fp2_mul(S2, S2, zz);                     // 2 y_Q Z^3
  fp2_sub(H, U, r.x);
  fp2_sqr(HH, H);
  fp2_dbl(I, HH);
  fp2_dbl(I, I);
  fp2_mul(J, I, H);
  fp2_sub(rr, S2, r.y);
  fp2_sub(rr, rr, r.y);                    // 2 (y_Q Z^3 - Y)
  fp2_mul(V, I, r.x);
  g2_jac o;
  fp2_sqr(o.x, rr);
  fp2_sub(o.x, o.x, J);
  fp2_sub(o.x, o.x, V);
  fp2_sub(o.x, o.x, V);
  fp2_add(o.z, r.z, H);
  fp2_sqr(o.z, o.z);
  fp2_sub(o.z, o.z, zz);
  fp2_sub(o.z, o.z, HH);                   // 2 Z H
  fp2_sub(t, V, o.x);
  fp2_mul(o.y, t, rr);
  fp2_mul(t, r.y, J);
  fp2_dbl(t, t);
  fp2_sub(o.y, o.y, t);
  // l2 = 2 rr x_Q - 2 y_Q Z'
  fp2_add(t, q.y, o.z);
  fp2_sqr(t, t);
  fp2_sub(t, t, yy);
  fp2_sqr(u, o.z);
  fp2_sub(t, t, u);                        // 2 y_Q Z'
  fp2_mul(u, rr, q.x);
  fp2_dbl(u, u);
  fp2_sub(line[2], u, t);
  fp2_dbl(line[0], o.z);
  fp2_dbl(t, rr);
  fp2_neg(line[1], t);
  r = o;
}
// The PAIRING_LINES triples of q (not the identity), in the order pairing_miller2 consumes them: what G2Prepared holds
// (pairings.rs:504-546)
inline void g2_prepare(fp2_t out[PAIRING_TABLE_FP2], const g2_affine& q) {
  constexpr uint64_t HALF_X = TOWER_BLS_X_ABS >> 1;
  g2_jac r = g2_from_affine(q);
  int line = 0;
  for (int b = 61; b >= -1; b--) {
    g2_line_double(r, out + 3 * line++);
    if (b >= 0 && ((HALF_X >> b) & 1)) g2_line_add(r, q, out + 3 * line++);
  }
}

}  // namespace bp

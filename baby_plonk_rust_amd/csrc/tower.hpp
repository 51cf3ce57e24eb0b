// tower.hpp -- the extension tower of BLS12-381 over Fp = Mont<FpParams>:
//   Fp2  = Fp[u]  / (u^2 + 1)          (fp2.rs)
//   Fp6  = Fp2[v] / (v^3 - (u + 1))    (fp6.rs)
//   Fp12 = Fp6[w] / (w^2 - v)          (fp12.rs)
// Every function computes the unique reduced field element the reference computes; the routes (Karatsuba products, the complex
// squaring, the adjugate inversions) are this file's own.  Everything is __host__ __device__: the same lines run in the host
// pairing check, in the CPU tests (tests/cpp/tower_host.hip) and in the kernels of pairing_kernels.hpp.
//
// Two layers.
//   1. Fp2 and Fp6 are plain structs (24 and 72 dwords) and their functions are inlined: the values live in registers.
//   2. An Fp12 is 144 dwords, and the pairing keeps eight of them alive: far more than a lane's registers.  Fp12 values therefore
//      live in a WORKSPACE of Fp2 slots that the caller provides, and the Fp12 functions take slot numbers.  A workspace type W has
//          fp2_t ld(int slot) const;      void st(int slot, const fp2_t&) const;
//      HostWs below is an array of fp2_t; the kernels use a per-lane view of HBM laid out limb-major by lane (LaneWs,
//      pairing_kernels.hpp), so that the 64 lanes of a wave touch 64 consecutive dwords.  On the device each layer-2 function is a
//      real function (not inlined): it takes a pointer and a few integers, so a call costs nothing beside the 10^4 instructions
//      it runs, every routine exists once in the code object, and no Fp12 ever sits on the compiler's stack.
//      Slots 0..8 are the scratch of the layer-2 functions themselves, slots 9..11 hold the line that mul_by_014 multiplies by;
//      Fp12 variable k of the caller is slots 12 + 6 k .. 17 + 6 k (c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2).
#pragma once
#include "fields.hpp"

namespace bp {

struct fp2_t {
  fp_t c0, c1;
};
struct fp6_t {
  fp2_t c0, c1, c2;
};
struct fp12_t {
  fp6_t c0, c1;
};

// Frobenius constants, Montgomery form: xi^((p-1)/3) = FROB6_C1 u, xi^((2p-2)/3) = FROB6_C2 (in Fp), xi^((p-1)/6) = FROB12 (xi = u + 1)
BP_TABLE(frob6_c1_u, 0x8671f071u, 0xcd03c9e4u, 0x1fcda5d2u, 0x5dab2246u, 0xd3851b95u, 0x587042afu, 0x01bacb9eu, 0x8eb60ebeu, 0x83d050d2u,
         0x03f97d6eu, 0x54638741u, 0x18f02065u)
BP_TABLE(frob6_c2_re, 0x867545c3u, 0x890dc9e4u, 0x3285a5d5u, 0x2af32253u, 0x309b7e2cu, 0x50880866u, 0x7e881024u, 0xa20d1b8cu, 0xe2db9068u,
         0x14e4f04fu, 0x1564853au, 0x14e56d3fu)
BP_TABLE(frob12_re, 0xb319d465u, 0x07089552u, 0xb50a8313u, 0xc6695f92u, 0xd117228fu, 0x97e83cccu, 0xb2dc29eeu, 0xa35baecau, 0x5daace4du,
         0x1ce393eau, 0xb0fb66ebu, 0x08f2220fu)
BP_TABLE(frob12_im, 0x4ce5d646u, 0xb2f66aadu, 0xfc497cecu, 0x5842a06bu, 0x2599d394u, 0xcf4895d4u, 0x40a8e8d0u, 0xc11b9cbau, 0xe5a0de89u,
         0x2e3813cbu, 0x88847fafu, 0x110eefdau)
#define BP_FP_CONST(name, table)                     \
  BP_HD fp_t name() {                                \
    fp_t r;                                          \
    _Pragma("unroll") for (int i = 0; i < 12; i++) r.l[i] = table(i); \
    return r;                                        \
  }
BP_FP_CONST(fp_frob6_c1_u, frob6_c1_u)
BP_FP_CONST(fp_frob6_c2_re, frob6_c2_re)
BP_FP_CONST(fp_frob12_re, frob12_re)
BP_FP_CONST(fp_frob12_im, frob12_im)

// ---- Fp2 ------------------------------------------------------------------------------------------------------------------------
BP_HD fp2_t fp2_zero() { return fp2_t{Fp::zero(), Fp::zero()}; }
BP_HD fp2_t fp2_one() { return fp2_t{Fp::one(), Fp::zero()}; }
BP_HD bool fp2_is_zero(const fp2_t& a) { return big_is_zero(a.c0) && big_is_zero(a.c1); }
BP_HD bool fp2_eq(const fp2_t& a, const fp2_t& b) { return big_eq(a.c0, b.c0) && big_eq(a.c1, b.c1); }
BP_HD void fp2_add(fp2_t& r, const fp2_t& a, const fp2_t& b) {
  Fp::add(r.c0, a.c0, b.c0);
  Fp::add(r.c1, a.c1, b.c1);
}
BP_HD void fp2_sub(fp2_t& r, const fp2_t& a, const fp2_t& b) {
  Fp::sub(r.c0, a.c0, b.c0);
  Fp::sub(r.c1, a.c1, b.c1);
}
BP_HD void fp2_dbl(fp2_t& r, const fp2_t& a) { fp2_add(r, a, a); }
BP_HD void fp2_neg(fp2_t& r, const fp2_t& a) {
  Fp::neg(r.c0, a.c0);
  Fp::neg(r.c1, a.c1);
}
BP_HD void fp2_conjugate(fp2_t& r, const fp2_t& a) {
  r.c0 = a.c0;
  Fp::neg(r.c1, a.c1);
}
// x -> x^p on Fp2 is the conjugation (u^p = -u as p = 3 mod 4)
BP_HD void fp2_frobenius(fp2_t& r, const fp2_t& a) { fp2_conjugate(r, a); }
// (a0 + a1 u)(b0 + b1 u) with three products: a0 b0 - a1 b1 + ((a0 + a1)(b0 + b1) - a0 b0 - a1 b1) u
BP_HD void fp2_mul(fp2_t& r, const fp2_t& a, const fp2_t& b) {
  fp_t p0, p1, sa, sb, m;
  Fp::mul(p0, a.c0, b.c0);
  Fp::mul(p1, a.c1, b.c1);
  Fp::add(sa, a.c0, a.c1);
  Fp::add(sb, b.c0, b.c1);
  Fp::mul(m, sa, sb);
  Fp::sub(r.c0, p0, p1);
  Fp::sub(m, m, p0);
  Fp::sub(r.c1, m, p1);
}
// (a0 + a1)(a0 - a1) + 2 a0 a1 u
BP_HD void fp2_sqr(fp2_t& r, const fp2_t& a) {
  fp_t s, d, m;
  Fp::add(s, a.c0, a.c1);
  Fp::sub(d, a.c0, a.c1);
  Fp::mul(m, a.c0, a.c1);
  Fp::mul(r.c0, s, d);
  Fp::dbl(r.c1, m);
}
BP_HD void fp2_mul_fp(fp2_t& r, const fp2_t& a, const fp_t& s) {
  Fp::mul(r.c0, a.c0, s);
  Fp::mul(r.c1, a.c1, s);
}
// times xi = u + 1: (a0 - a1) + (a0 + a1) u
BP_HD void fp2_mul_by_nonresidue(fp2_t& r, const fp2_t& a) {
  fp_t t;
  Fp::sub(t, a.c0, a.c1);
  Fp::add(r.c1, a.c0, a.c1);
  r.c0 = t;
}
// conj(a) / (a0^2 + a1^2); 0 -> 0
BP_HD void fp2_invert(fp2_t& r, const fp2_t& a) {
  fp_t n, t;
  Fp::sqr(n, a.c0);
  Fp::sqr(t, a.c1);
  Fp::add(n, n, t);
  fp_invert(n, n);
  Fp::mul(r.c0, a.c0, n);
  Fp::mul(t, a.c1, n);
  Fp::neg(r.c1, t);
}

// ---- Fp6 ------------------------------------------------------------------------------------------------------------------------
BP_HD fp6_t fp6_zero() { return fp6_t{fp2_zero(), fp2_zero(), fp2_zero()}; }
BP_HD fp6_t fp6_one() { return fp6_t{fp2_one(), fp2_zero(), fp2_zero()}; }
BP_HD bool fp6_eq(const fp6_t& a, const fp6_t& b) { return fp2_eq(a.c0, b.c0) && fp2_eq(a.c1, b.c1) && fp2_eq(a.c2, b.c2); }
BP_HD void fp6_add(fp6_t& r, const fp6_t& a, const fp6_t& b) {
  fp2_add(r.c0, a.c0, b.c0);
  fp2_add(r.c1, a.c1, b.c1);
  fp2_add(r.c2, a.c2, b.c2);
}
BP_HD void fp6_sub(fp6_t& r, const fp6_t& a, const fp6_t& b) {
  fp2_sub(r.c0, a.c0, b.c0);
  fp2_sub(r.c1, a.c1, b.c1);
  fp2_sub(r.c2, a.c2, b.c2);
}
BP_HD void fp6_neg(fp6_t& r, const fp6_t& a) {
  fp2_neg(r.c0, a.c0);
  fp2_neg(r.c1, a.c1);
  fp2_neg(r.c2, a.c2);
}
// times v: (xi a2, a0, a1)
BP_HD void fp6_mul_by_nonresidue(fp6_t& r, const fp6_t& a) {
  fp2_t t;
  fp2_mul_by_nonresidue(t, a.c2);
  r.c2 = a.c1;
  r.c1 = a.c0;
  r.c0 = t;
}
// six Fp2 products: v_i = a_i b_i and the three cross sums, reduced by v^3 = xi
BP_HD void fp6_mul(fp6_t& r, const fp6_t& a, const fp6_t& b) {
  fp2_t v0, v1, v2, s, t, x;
  fp2_mul(v0, a.c0, b.c0);
  fp2_mul(v1, a.c1, b.c1);
  fp2_mul(v2, a.c2, b.c2);
  fp6_t o;
  fp2_add(s, a.c1, a.c2);
  fp2_add(t, b.c1, b.c2);
  fp2_mul(x, s, t);
  fp2_sub(x, x, v1);
  fp2_sub(x, x, v2);
  fp2_mul_by_nonresidue(x, x);
  fp2_add(o.c0, x, v0);
  fp2_add(s, a.c0, a.c1);
  fp2_add(t, b.c0, b.c1);
  fp2_mul(x, s, t);
  fp2_sub(x, x, v0);
  fp2_sub(x, x, v1);
  fp2_mul_by_nonresidue(s, v2);
  fp2_add(o.c1, x, s);
  fp2_add(s, a.c0, a.c2);
  fp2_add(t, b.c0, b.c2);
  fp2_mul(x, s, t);
  fp2_sub(x, x, v0);
  fp2_sub(x, x, v2);
  fp2_add(o.c2, x, v1);
  r = o;
}
// three squarings and two products: with s0 = a0^2, s1 = 2 a0 a1, s2 = (a0 - a1 + a2)^2, s3 = 2 a1 a2, s4 = a2^2 the square is
// (s0 + xi s3, s1 + xi s4, s1 + s2 + s3 - s0 - s4)
BP_HD void fp6_sqr(fp6_t& r, const fp6_t& a) {
  fp2_t s0, s1, s2, s3, s4, t;
  fp2_sqr(s0, a.c0);
  fp2_mul(s1, a.c0, a.c1);
  fp2_dbl(s1, s1);
  fp2_sub(t, a.c0, a.c1);
  fp2_add(t, t, a.c2);
  fp2_sqr(s2, t);
  fp2_mul(s3, a.c1, a.c2);
  fp2_dbl(s3, s3);
  fp2_sqr(s4, a.c2);
  fp2_mul_by_nonresidue(t, s3);
  fp2_add(r.c0, t, s0);
  fp2_mul_by_nonresidue(t, s4);
  fp2_add(r.c1, t, s1);
  fp2_add(t, s1, s2);
  fp2_add(t, t, s3);
  fp2_sub(t, t, s0);
  fp2_sub(r.c2, t, s4);
}
// a * (c1 v): (xi a2 c1, a0 c1, a1 c1)
BP_HD void fp6_mul_by_1(fp6_t& r, const fp6_t& a, const fp2_t& c1) {
  fp6_t o;
  fp2_mul(o.c0, a.c2, c1);
  fp2_mul_by_nonresidue(o.c0, o.c0);
  fp2_mul(o.c1, a.c0, c1);
  fp2_mul(o.c2, a.c1, c1);
  r = o;
}
// a * (c0 + c1 v), five Fp2 products
BP_HD void fp6_mul_by_01(fp6_t& r, const fp6_t& a, const fp2_t& c0, const fp2_t& c1) {
  fp2_t p0, p1, s, t, x;
  fp6_t o;
  fp2_mul(p0, a.c0, c0);
  fp2_mul(p1, a.c1, c1);
  fp2_mul(x, a.c2, c1);
  fp2_mul_by_nonresidue(x, x);
  fp2_add(o.c0, x, p0);
  fp2_add(s, a.c0, a.c1);
  fp2_add(t, c0, c1);
  fp2_mul(x, s, t);
  fp2_sub(x, x, p0);
  fp2_sub(o.c1, x, p1);
  fp2_mul(x, a.c2, c0);
  fp2_add(o.c2, x, p1);
  r = o;
}
// x -> x^p: conjugate every coefficient, then v^p = xi^((p-1)/3) v and v^2p = xi^((2p-2)/3) v^2
BP_HD void fp6_frobenius(fp6_t& r, const fp6_t& a) {
  fp2_t t;
  fp2_conjugate(r.c0, a.c0);
  fp2_conjugate(t, a.c1);
  const fp_t g = fp_frob6_c1_u();                       // (x + y u)(g u) = -y g + x g u
  fp_t re;
  Fp::mul(re, t.c1, g);
  Fp::neg(re, re);
  Fp::mul(r.c1.c1, t.c0, g);
  r.c1.c0 = re;
  fp2_conjugate(t, a.c2);
  fp2_mul_fp(r.c2, t, fp_frob6_c2_re());
}
// the adjugate: with A = a0^2 - xi a1 a2, B = xi a2^2 - a0 a1, C = a1^2 - a0 a2 and d = a0 A + xi (a2 B + a1 C), a^-1 = (A, B, C) / d
BP_HD void fp6_invert(fp6_t& r, const fp6_t& a) {
  fp2_t A, B, C, d, t;
  fp2_mul(t, a.c1, a.c2);
  fp2_mul_by_nonresidue(t, t);
  fp2_sqr(A, a.c0);
  fp2_sub(A, A, t);
  fp2_sqr(B, a.c2);
  fp2_mul_by_nonresidue(B, B);
  fp2_mul(t, a.c0, a.c1);
  fp2_sub(B, B, t);
  fp2_sqr(C, a.c1);
  fp2_mul(t, a.c0, a.c2);
  fp2_sub(C, C, t);
  fp2_mul(d, a.c2, B);
  fp2_mul(t, a.c1, C);
  fp2_add(d, d, t);
  fp2_mul_by_nonresidue(d, d);
  fp2_mul(t, a.c0, A);
  fp2_add(d, d, t);
  fp2_invert(d, d);
  fp2_mul(r.c0, A, d);
  fp2_mul(r.c1, B, d);
  fp2_mul(r.c2, C, d);
}

// ---- workspaces and Fp12 --------------------------------------------------------------------------------------------------------
constexpr int TW_T0 = 0, TW_T1 = 3, TW_T2 = 6;       // three Fp6 of scratch for the functions below
constexpr int TW_LINE = 9;                           // c0, c1, c4 of the sparse factor of fp12w_mul_by_014
constexpr int TW_VAR0 = 12;                          // the caller's Fp12 variables start here
BP_HD constexpr int tw_var(int k) { return TW_VAR0 + 6 * k; }
BP_HD constexpr int tw_slots(int vars) { return TW_VAR0 + 6 * vars; }

struct HostWs {
  fp2_t* s;
  BP_HD fp2_t ld(int slot) const { return s[slot]; }
  BP_HD void st(int slot, const fp2_t& v) const { s[slot] = v; }
};

// layer-2 functions: real calls on the device (see the head of this file), inlined into the host code
#if defined(__HIP_DEVICE_COMPILE__)
#define BP_TW static __host__ __device__ __noinline__
#else
#define BP_TW static inline __host__ __device__
#endif

template <class W>
BP_HD fp6_t tw_ld6(const W& w, int s) {
  return fp6_t{w.ld(s), w.ld(s + 1), w.ld(s + 2)};
}
template <class W>
BP_HD void tw_st6(const W& w, int s, const fp6_t& v) {
  w.st(s, v.c0);
  w.st(s + 1, v.c1);
  w.st(s + 2, v.c2);
}

template <class W>
BP_TW void fp6w_mul(W w, int r, int a, int b) {
  const fp6_t x = tw_ld6(w, a), y = tw_ld6(w, b);
  fp6_t z;
  fp6_mul(z, x, y);
  tw_st6(w, r, z);
}
template <class W>
BP_TW void fp12w_copy(W w, int r, int a) {
#pragma unroll 1
  for (int k = 0; k < 6; k++) w.st(r + k, w.ld(a + k));
}
template <class W>
BP_TW void fp12w_set_one(W w, int r) {
  w.st(r, fp2_one());
#pragma unroll 1
  for (int k = 1; k < 6; k++) w.st(r + k, fp2_zero());
}
template <class W>
BP_TW bool fp12w_is_one(W w, int a) {
  bool ok = fp2_eq(w.ld(a), fp2_one());
#pragma unroll 1
  for (int k = 1; k < 6; k++) ok = ok && fp2_is_zero(w.ld(a + k));
  return ok;
}
// a0 - a1 w: the inverse of a unitary element, and x -> x^(p^6)
template <class W>
BP_TW void fp12w_conjugate(W w, int r, int a) {
#pragma unroll 1
  for (int k = 0; k < 3; k++) {
    fp2_t t = w.ld(a + 3 + k);
    fp2_neg(t, t);
    w.st(r + k, w.ld(a + k));
    w.st(r + 3 + k, t);
  }
}
// (a0 + a1 w)(b0 + b1 w) = a0 b0 + v a1 b1 + ((a0 + a1)(b0 + b1) - a0 b0 - a1 b1) w: three Fp6 products
template <class W>
BP_TW void fp12w_mul(W w, int r, int a, int b) {
  fp6_t x = tw_ld6(w, a), y = tw_ld6(w, a + 3);
  fp6_add(x, x, y);
  tw_st6(w, TW_T0, x);
  x = tw_ld6(w, b);
  y = tw_ld6(w, b + 3);
  fp6_add(x, x, y);
  tw_st6(w, TW_T1, x);
  fp6w_mul(w, TW_T0, TW_T0, TW_T1);
  fp6w_mul(w, TW_T1, a, b);
  fp6w_mul(w, TW_T2, a + 3, b + 3);
  x = tw_ld6(w, TW_T1);
  y = tw_ld6(w, TW_T2);
  fp6_t z = tw_ld6(w, TW_T0);
  fp6_sub(z, z, x);
  fp6_sub(z, z, y);
  tw_st6(w, r + 3, z);
  fp6_mul_by_nonresidue(y, y);
  fp6_add(x, x, y);
  tw_st6(w, r, x);
}
// (a0 + a1 w)^2 = (a0 + a1)(a0 + v a1) - m - v m + 2 m w with m = a0 a1: two Fp6 products
template <class W>
BP_TW void fp12w_sqr(W w, int r, int a) {
  const fp6_t x = tw_ld6(w, a), y = tw_ld6(w, a + 3);
  fp6_t s, t;
  fp6_add(s, x, y);
  tw_st6(w, TW_T0, s);
  fp6_mul_by_nonresidue(t, y);
  fp6_add(t, t, x);
  tw_st6(w, TW_T1, t);
  fp6w_mul(w, TW_T0, TW_T0, TW_T1);
  fp6w_mul(w, TW_T1, a, a + 3);
  const fp6_t m = tw_ld6(w, TW_T1);
  s = tw_ld6(w, TW_T0);
  fp6_sub(s, s, m);
  fp6_mul_by_nonresidue(t, m);
  fp6_sub(s, s, t);
  tw_st6(w, r, s);
  fp6_add(t, m, m);
  tw_st6(w, r + 3, t);
}
// f *= c0 + c1 v + c4 v w, the three Fp2 in slots TW_LINE .. TW_LINE + 2: thirteen Fp2 products instead of eighteen
template <class W>
BP_TW void fp12w_mul_by_014(W w, int f) {
  const fp2_t c0 = w.ld(TW_LINE), c1 = w.ld(TW_LINE + 1), c4 = w.ld(TW_LINE + 2);
  fp6_t x = tw_ld6(w, f), y = tw_ld6(w, f + 3), t;
  fp6_mul_by_01(t, x, c0, c1);
  tw_st6(w, TW_T0, t);                                       // f0 (c0 + c1 v)
  fp6_mul_by_1(t, y, c4);
  tw_st6(w, TW_T1, t);                                       // f1 c4 v
  fp6_add(x, x, y);
  fp2_t o;
  fp2_add(o, c1, c4);
  fp6_mul_by_01(x, x, c0, o);
  y = tw_ld6(w, TW_T0);
  t = tw_ld6(w, TW_T1);
  fp6_sub(x, x, y);
  fp6_sub(x, x, t);
  tw_st6(w, f + 3, x);
  fp6_mul_by_nonresidue(t, t);
  fp6_add(t, t, y);
  tw_st6(w, f, t);
}
// x -> x^p: the Fp6 map on both halves, then w^p = xi^((p-1)/6) w
template <class W>
BP_TW void fp12w_frobenius(W w, int r, int a) {
  fp6_t x = tw_ld6(w, a);
  fp6_frobenius(x, x);
  tw_st6(w, r, x);
  x = tw_ld6(w, a + 3);
  fp6_frobenius(x, x);
  const fp2_t g{fp_frob12_re(), fp_frob12_im()};
  fp2_mul(x.c0, x.c0, g);
  fp2_mul(x.c1, x.c1, g);
  fp2_mul(x.c2, x.c2, g);
  tw_st6(w, r + 3, x);
}
// (a0 - a1 w) / (a0^2 - v a1^2); 0 -> 0.  One Fp inversion at the bottom.
template <class W>
BP_TW void fp12w_invert(W w, int r, int a) {
  fp6_t x = tw_ld6(w, a), y = tw_ld6(w, a + 3);
  fp6_sqr(x, x);
  fp6_sqr(y, y);
  fp6_mul_by_nonresidue(y, y);
  fp6_sub(x, x, y);
  fp6_invert(x, x);
  tw_st6(w, TW_T2, x);
  fp6w_mul(w, TW_T0, a, TW_T2);
  fp6w_mul(w, TW_T1, a + 3, TW_T2);
  y = tw_ld6(w, TW_T1);
  fp6_neg(y, y);
  tw_st6(w, r + 3, y);
  tw_st6(w, r, tw_ld6(w, TW_T0));
}

// (a + b s)^2 in Fp4 = Fp2[s] / (s^2 - xi): a^2 + xi b^2, 2 a b (as (a + b)^2 - a^2 - b^2)
BP_HD void fp4_sqr(fp2_t& r0, fp2_t& r1, const fp2_t& a, const fp2_t& b) {
  fp2_t a2, b2, t;
  fp2_sqr(a2, a);
  fp2_sqr(b2, b);
  fp2_add(t, a, b);
  fp2_sqr(t, t);
  fp2_sub(t, t, a2);
  fp2_sub(r1, t, b2);
  fp2_mul_by_nonresidue(t, b2);
  fp2_add(r0, t, a2);
}
// The square of an element of the cyclotomic subgroup (one already raised to (p^6 - 1)(p^2 + 1)), Granger-Scott (eprint 2009/565):
// the element is three Fp4 pairs (g0, g4), (g3, g2), (g1, g5) over the slots g0..g5; each pair is squared in Fp4 and the result is
// 3 S -/+ 2 g.  Nine Fp2 squarings against the twelve Fp2 products of fp12w_sqr.
template <class W>
BP_TW void fp12w_cyclotomic_sqr(W w, int r, int a) {
  fp2_t s0, s1, g, h, t;
  auto out_minus = [&](int slot, const fp2_t& s, const fp2_t& old) {      // 3 s - 2 old
    fp2_sub(t, s, old);
    fp2_dbl(t, t);
    fp2_add(t, t, s);
    w.st(slot, t);
  };
  auto out_plus = [&](int slot, const fp2_t& s, const fp2_t& old) {       // 3 s + 2 old
    fp2_add(t, s, old);
    fp2_dbl(t, t);
    fp2_add(t, t, s);
    w.st(slot, t);
  };
  const fp2_t g2 = w.ld(a + 2), g3 = w.ld(a + 3);                         // read before slot r + 3 is written (r may be a)
  g = w.ld(a);
  h = w.ld(a + 4);
  fp4_sqr(s0, s1, g, h);
  out_minus(r, s0, g);
  out_plus(r + 4, s1, h);
  g = w.ld(a + 1);
  h = w.ld(a + 5);
  fp2_t u0, u1;
  fp4_sqr(u0, u1, g, h);                                                  // pair (g1, g5), feeds g3 and g2
  fp4_sqr(s0, s1, g3, g2);                                                // pair (g3, g2), feeds g1 and g5
  out_minus(r + 1, s0, g);
  out_plus(r + 5, s1, h);
  fp2_mul_by_nonresidue(u1, u1);
  out_plus(r + 3, u1, g3);
  out_minus(r + 2, u0, g2);
}
// |x| of the curve parameter x = -0xd201000000010000
constexpr uint64_t TOWER_BLS_X_ABS = 0xd201000000010000ull;
// r = a^x for a in the cyclotomic subgroup: a^|x| by square-and-multiply from the top bit, then the conjugate (x < 0).  r != a.
template <class W>
BP_TW void fp12w_cyclotomic_exp(W w, int r, int a) {
  fp12w_copy(w, r, a);
#pragma unroll 1
  for (int b = 62; b >= 0; b--) {
    fp12w_cyclotomic_sqr(w, r, r);
    if ((TOWER_BLS_X_ABS >> b) & 1) fp12w_mul(w, r, r, a);
  }
  fp12w_conjugate(w, r, r);
}

}  // namespace bp

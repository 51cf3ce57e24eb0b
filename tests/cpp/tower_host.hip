// tower_host.hip -- test-only host shim over csrc/tower.hpp, csrc/g2_host.hpp and csrc/pairing_host.hpp (tests/test_tower_host.py,
// tests/test_pairing_host.py): hipcc --offload-host-only -shared.  Field elements cross the boundary as Montgomery memory images
// (48 bytes per Fp, so 96 / 288 / 576 per Fp2 / Fp6 / Fp12), points and pairs in their wire formats.
#include <string.h>

#include "../../baby_plonk_rust_amd/csrc/pairing_host.hpp"
using namespace bp;

static fp2_t ld2(const uint8_t* p) {
  fp2_t v;
  memcpy(&v, p, 96);
  return v;
}
static fp6_t ld6(const uint8_t* p) {
  fp6_t v;
  memcpy(&v, p, 288);
  return v;
}

extern "C" {

// r = op(a, b) on Fp2; unary operations ignore b
int tw_fp2(const char* op, const uint8_t* a, const uint8_t* b, uint8_t* r) {
  const fp2_t x = ld2(a), y = ld2(b);
  fp2_t z;
  if (!strcmp(op, "add")) fp2_add(z, x, y);
  else if (!strcmp(op, "sub")) fp2_sub(z, x, y);
  else if (!strcmp(op, "neg")) fp2_neg(z, x);
  else if (!strcmp(op, "mul")) fp2_mul(z, x, y);
  else if (!strcmp(op, "square")) fp2_sqr(z, x);
  else if (!strcmp(op, "mul_by_nonresidue")) fp2_mul_by_nonresidue(z, x);
  else if (!strcmp(op, "conjugate")) fp2_conjugate(z, x);
  else if (!strcmp(op, "frobenius")) fp2_frobenius(z, x);
  else if (!strcmp(op, "invert")) fp2_invert(z, x);
  else return -1;
  memcpy(r, &z, 96);
  return 0;
}
// r = op(a, b) on Fp6; c0, c1: the Fp2 arguments of the sparse products
int tw_fp6(const char* op, const uint8_t* a, const uint8_t* b, const uint8_t* c0, const uint8_t* c1, uint8_t* r) {
  const fp6_t x = ld6(a), y = ld6(b);
  fp6_t z;
  if (!strcmp(op, "mul")) fp6_mul(z, x, y);
  else if (!strcmp(op, "square")) fp6_sqr(z, x);
  else if (!strcmp(op, "mul_by_1")) fp6_mul_by_1(z, x, ld2(c1));
  else if (!strcmp(op, "mul_by_01")) fp6_mul_by_01(z, x, ld2(c0), ld2(c1));
  else if (!strcmp(op, "mul_by_nonresidue")) fp6_mul_by_nonresidue(z, x);
  else if (!strcmp(op, "frobenius")) fp6_frobenius(z, x);
  else if (!strcmp(op, "invert")) fp6_invert(z, x);
  else if (!strcmp(op, "add")) fp6_add(z, x, y);
  else if (!strcmp(op, "sub")) fp6_sub(z, x, y);
  else if (!strcmp(op, "neg")) fp6_neg(z, x);
  else return -1;
  memcpy(r, &z, 288);
  return 0;
}
// r = op(a, b) on Fp12 through a host workspace, the result variable aliased with `a` when in_place is set; line: three Fp2 (c0, c1,
// c4) for mul_by_014.  Returns 0, or 1 / 0 for is_one, or -1 for an unknown name.
int tw_fp12(const char* op, const uint8_t* a, const uint8_t* b, const uint8_t* line, int in_place, uint8_t* r) {
  fp2_t slots[tw_slots(3)];
  const HostWs w{slots};
  const int va = tw_var(0), vb = tw_var(1), vr = in_place ? va : tw_var(2);
  memcpy(&slots[va], a, 576);
  memcpy(&slots[vb], b, 576);
  memset(&slots[tw_var(2)], 0xEE, 576);
  int rc = 0;
  if (!strcmp(op, "mul")) fp12w_mul(w, vr, va, vb);
  else if (!strcmp(op, "square")) fp12w_sqr(w, vr, va);
  else if (!strcmp(op, "mul_by_014")) {
    memcpy(&slots[TW_LINE], line, 288);
    fp12w_mul_by_014(w, va);
    if (!in_place) fp12w_copy(w, vr, va);
  } else if (!strcmp(op, "conjugate")) fp12w_conjugate(w, vr, va);
  else if (!strcmp(op, "frobenius")) fp12w_frobenius(w, vr, va);
  else if (!strcmp(op, "invert")) fp12w_invert(w, vr, va);
  else if (!strcmp(op, "cyclotomic_square")) fp12w_cyclotomic_sqr(w, vr, va);
  else if (!strcmp(op, "cyclotomic_exp")) {                      // r != a by contract
    fp12w_cyclotomic_exp(w, tw_var(2), va);
    if (in_place) fp12w_copy(w, vr, tw_var(2));
  } else if (!strcmp(op, "is_one")) rc = fp12w_is_one(w, va) ? 1 : 0;
  else if (!strcmp(op, "one")) fp12w_set_one(w, vr);
  else return -1;
  memcpy(r, &slots[vr], 576);
  return rc;
}
// f *= line(P) for the triple `line` (three Fp2) and the affine point p (x | y Montgomery images)
void tw_ell(const uint8_t* f, const uint8_t* line, const uint8_t* p96m, uint8_t* r) {
  fp2_t slots[tw_slots(1)];
  const HostWs w{slots};
  memcpy(&slots[tw_var(0)], f, 576);
  fp2_t l[3];
  memcpy(l, line, 288);
  g1_affine p;
  memcpy(&p, p96m, 96);
  pairing_ell(w, tw_var(0), l, p);
  memcpy(r, &slots[tw_var(0)], 576);
}

// ---- G2
int tw_g2_decode(const uint8_t* in192, uint8_t* x_y_mont192, int* infinity) {
  g2_affine p;
  if (!g2_decode192(p, in192)) return 0;
  memcpy(x_y_mont192, &p.x, 96);
  memcpy(x_y_mont192 + 96, &p.y, 96);
  *infinity = p.infinity;
  return 1;
}
int tw_g2_on_curve(const uint8_t* in192) {
  g2_affine p;
  return g2_decode192(p, in192) ? (g2_on_curve(p) ? 1 : 0) : -1;
}
int tw_g2_is_torsion_free(const uint8_t* in192) {
  g2_affine p;
  return g2_decode192(p, in192) ? (g2_is_torsion_free(p) ? 1 : 0) : -1;
}
// out = a + b (op 0), 2 a (op 1), with a taken through a Jacobian form scaled by the Fp2 z (Montgomery image) first
int tw_g2_op(int op, const uint8_t* a192, const uint8_t* b192, const uint8_t* z96m, uint8_t* out192) {
  g2_affine a, b;
  if (!g2_decode192(a, a192) || !g2_decode192(b, b192)) return -1;
  g2_jac ja = g2_from_affine(a), jb = g2_from_affine(b), r;
  const fp2_t z = ld2(z96m);
  if (!a.infinity) {                                             // (x z^2, y z^3, z)
    fp2_t z2, z3;
    fp2_sqr(z2, z);
    fp2_mul(z3, z2, z);
    fp2_mul(ja.x, ja.x, z2);
    fp2_mul(ja.y, ja.y, z3);
    ja.z = z;
  }
  if (op == 0) g2_add(r, ja, jb);
  else g2_double(r, ja);
  g2_encode192(out192, g2_to_affine(r));
  return 0;
}
// the 68 prepared triples of a point (not the identity)
int tw_g2_prepare(const uint8_t* in192, uint8_t* out) {
  g2_affine p;
  if (!g2_decode192(p, in192) || p.infinity) return -1;
  fp2_t t[PAIRING_TABLE_FP2];
  g2_prepare(t, p);
  memcpy(out, t, sizeof t);
  return 0;
}

// ---- the host entry points as the library exports them
int tw_g2_mul_generator(const uint8_t* k32, uint8_t* out192) { return host_g2_mul_generator(k32, out192); }
int tw_pairing_gt(const uint8_t* p96, const uint8_t* q192, uint8_t* gt576) { return host_pairing_gt(p96, q192, gt576); }
int tw_pairing_check(const uint8_t* x2, const uint8_t* pairs, size_t n, uint32_t checks, uint8_t* verdicts, uint8_t* gt, size_t* first_bad) {
  return host_pairing_check(x2, pairs, n, checks, verdicts, gt, first_bad);
}
}

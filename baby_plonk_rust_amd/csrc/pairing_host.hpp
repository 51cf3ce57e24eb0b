// pairing_host.hpp -- the host side of the pairing entry points, with no HIP call and no bp_ctx: decoding and checking the inputs,
// the prepared tables, and the whole check on the CPU (bp_pairing_gt_host, bp_pairing_check_host; capi_pairing.hip adds the GPU
// path over the same pairing.hpp).  The CPU tests and the stand-alone sanitizer program compile this header alone.
#pragma once
#include <mutex>
#include <vector>

#include "g2_host.hpp"

namespace bp {

constexpr uint32_t PAIRING_CHECK_G1_SUBGROUP = 1, PAIRING_CHECK_G2_SUBGROUP = 2;
constexpr size_t GT_BYTES = 576;

// the lines of the fixed generator: computed once per process
inline const fp2_t* g2_generator_lines() {
  static std::once_flag once;
  static fp2_t table[PAIRING_TABLE_FP2];
  std::call_once(once, [] { g2_prepare(table, g2_generator()); });
  return table;
}

// one 96-byte G1 record through the decoder the kernel runs (pairing.hpp); returns 0 or the reason (g1_check.hpp)
inline uint32_t pairing_decode_g1(g1_affine& out, const uint8_t in96[96], bool subgroup) {
  uint32_t w[24];
  memcpy(w, in96, 96);
  return pairing_decode_g1_words(out, w, subgroup);
}
// x_2 of a setup: decoded, on the curve, in the subgroup where asked, and not the identity
inline int pairing_decode_x2(g2_affine& out, const uint8_t x2_192[192], uint32_t checks) {
  if (!g2_decode192(out, x2_192) || !g2_on_curve(out)) return BP_ERR_BAD_POINT;
  if (out.infinity) return BP_ERR_INVALID_ARG;
  if ((checks & PAIRING_CHECK_G2_SUBGROUP) && !g2_is_torsion_free(out)) return BP_ERR_BAD_POINT;
  return BP_OK;
}

// the memory image of Gt: twelve Fp of six little-endian u64 Montgomery limbs = the six Fp2 slots of the variable as they are
inline void gt_store(uint8_t out[GT_BYTES], const HostWs& w, int var) {
  for (int k = 0; k < 6; k++) {
    const fp2_t v = w.ld(var + k);
    memcpy(out + 96 * k, &v, 96);
  }
}

// MillerLoop((a, x_2), (-b, G2)).final_exponentiation() of decoded points, tables given; returns is_one and optionally the image
inline bool pairing_check_one(const g1_affine& a, const g1_affine& b, const fp2_t* x2_lines, const fp2_t* gen_lines, uint8_t* gt576_or_null) {
  fp2_t slots[PAIRING_SLOTS];
  const HostWs w{slots};
  g1_affine nb;
  g1_neg_affine(nb, b);
  const int f = tw_var(0);
  pairing_miller2(w, f, x2_lines, a, gen_lines, nb);
  pairing_final_exponentiation(w, f, tw_var(1), tw_var(2), tw_var(3), tw_var(4), tw_var(5), tw_var(6), tw_var(7));
  if (gt576_or_null) gt_store(gt576_or_null, w, f);
  return fp12w_is_one(w, f);
}

// bls12_381::pairing(p, q): an identity on either side gives one
inline int host_pairing_gt(const uint8_t p96[96], const uint8_t q192[192], uint8_t gt576[GT_BYTES]) {
  g1_affine p;
  g2_affine q;
  if (pairing_decode_g1(p, p96, false)) return BP_ERR_BAD_POINT;
  if (!g2_decode192(q, q192) || !g2_on_curve(q)) return BP_ERR_BAD_POINT;
  fp2_t slots[PAIRING_SLOTS];
  const HostWs w{slots};
  const int f = tw_var(0);
  if (g1_affine_is_identity(p) || q.infinity) {
    fp12w_set_one(w, f);
  } else {
    std::vector<fp2_t> lines(PAIRING_TABLE_FP2);
    g2_prepare(lines.data(), q);
    const g1_affine none{Fp::zero(), Fp::zero()};
    pairing_miller2(w, f, lines.data(), p, lines.data(), none);
    pairing_final_exponentiation(w, f, tw_var(1), tw_var(2), tw_var(3), tw_var(4), tw_var(5), tw_var(6), tw_var(7));
  }
  gt_store(gt576, w, f);
  return BP_OK;
}

// the argument rules shared by bp_pairing_check_host and bp_pairing_check
inline bool pairing_args_ok(const uint8_t* x2_192, const uint8_t* pairs192, size_t n, const uint8_t* verdicts, const size_t* first_bad) {
  return x2_192 && first_bad && (n == 0 || (pairs192 && verdicts));
}

inline int host_pairing_check(const uint8_t x2_192[192], const uint8_t* pairs192, size_t n, uint32_t checks, uint8_t* verdicts,
                              uint8_t* gt576_or_null, size_t* first_bad) {
  if (!pairing_args_ok(x2_192, pairs192, n, verdicts, first_bad)) return BP_ERR_INVALID_ARG;
  *first_bad = SIZE_MAX;
  g2_affine x2;
  const int rc = pairing_decode_x2(x2, x2_192, checks);
  if (rc != BP_OK) return rc;
  std::vector<g1_affine> pts(2 * n);
  for (size_t i = 0; i < 2 * n; i++)
    if (pairing_decode_g1(pts[i], pairs192 + 96 * i, (checks & PAIRING_CHECK_G1_SUBGROUP) != 0)) {
      *first_bad = i / 2;
      return BP_ERR_BAD_POINT;
    }
  if (n == 0) return BP_OK;
  std::vector<fp2_t> lines(PAIRING_TABLE_FP2);
  g2_prepare(lines.data(), x2);
  const fp2_t* gen = g2_generator_lines();
  for (size_t i = 0; i < n; i++)
    verdicts[i] = pairing_check_one(pts[2 * i], pts[2 * i + 1], lines.data(), gen, gt576_or_null ? gt576_or_null + GT_BYTES * i : nullptr) ? 1 : 0;
  return BP_OK;
}

// x_2 = k * G2 for a canonical little-endian k < q (setup.rs:20)
inline int host_g2_mul_generator(const uint8_t k32[32], uint8_t out192[192]) {
  if (!fr_is_canonical(k32)) return BP_ERR_BAD_SCALAR;
  uint32_t k[8];
  memcpy(k, k32, 32);
  g2_encode192(out192, g2_to_affine(g2_mul(g2_generator(), k, 8)));
  return BP_OK;
}
// k * Q for any point Q of the curve (curve-checked here, not subgroup-checked) and a canonical little-endian k < q: x_2 of a
// ceremony contribution is s * x_2.  An identity Q or k = 0 gives the identity encoding.
inline int host_g2_mul(const uint8_t q192[192], const uint8_t k32[32], uint8_t out192[192]) {
  g2_affine q;
  if (!g2_decode192(q, q192) || !g2_on_curve(q)) return BP_ERR_BAD_POINT;
  if (!fr_is_canonical(k32)) return BP_ERR_BAD_SCALAR;
  uint32_t k[8];
  memcpy(k, k32, 32);
  g2_encode192(out192, g2_to_affine(g2_mul(q, k, 8)));
  return BP_OK;
}

}  // namespace bp

// g1_mul_split28.hpp -- one variable-base multiplication k P on the 28-bit limbs of fp28.hpp / g1_28.hpp, for kernels that run one
// product per lane: verify_seg_mul (verify_segments_kernels.hpp) and srs_scale (srs_kernels.hpp).  g1_mul_split28 writes
// k = k1 x^2 + k0 (scalar_split.hpp) and runs ONE joint double-and-add over P, [x^2] P = (beta x, -y) and their sum: 128 steps of one
// doubling and one complete addition, no data-dependent branch.  Exact only where the endomorphism is [x^2], that is inside the
// prime-order subgroup: the caller has tested its points.
#pragma once
#include "g1_28.hpp"
#include "g1_check.hpp"
#include "scalar_split.hpp"

namespace bp {

#if defined(__HIPCC__)
__device__ __forceinline__ C28 seg_one28() {
  C28 r;
#pragma unroll
  for (int i = 0; i < N28; i++) r.l[i] = One28::limb(i);
  return r;
}

// k P for a canonical k < 2^255 and an affine P of the prime-order subgroup, or the identity (0, 0)
__device__ __forceinline__ g1_proj28 g1_mul_split28(const g1_affine& p, const fr_t& k) {
  uint32_t k0[4], k1[4];
  scalar_split_x2(k0, k1, k.l);
  const bool id = g1_affine_is_identity(p);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    k0[i] = id ? 0u : k0[i];
    k1[i] = id ? 0u : k1[i];
  }
  fp_t beta, bx;
#pragma unroll
  for (int i = 0; i < 12; i++) beta.l[i] = fp_beta_canonical(i);
  Fp::to_mont(beta, beta);
  Fp::mul(bx, p.x, beta);
  const F28n y0 = fp_to_28(p.y);
  const C28 one = seg_one28();
  g1_proj28 P0, P1, P01;                                        // P, [x^2] P = -phi(P) = (beta x, -y), and their sum
  P0.x = widen28<C28>(fp_to_28(p.x));
  P0.y = widen28<C28>(y0);
  P0.z = one;
  P1.x = widen28<C28>(fp_to_28(bx));
  P1.y = widen28<C28>(pt_y_signed(y0, true));
  P1.z = one;
  g1_add28(P01, P0, P1);
  g1_proj28 acc = g1_identity28();
#pragma unroll 1
  for (int step = 0; step < SCALAR_SPLIT_BITS; step++) {
    const uint32_t sel = (k0[3] >> 31) | ((k1[3] >> 31) << 1);
#pragma unroll
    for (int i = 3; i > 0; i--) {
      k0[i] = (k0[i] << 1) | (k0[i - 1] >> 31);
      k1[i] = (k1[i] << 1) | (k1[i - 1] >> 31);
    }
    k0[0] <<= 1;
    k1[0] <<= 1;
    g1_double28(acc, acc);
    g1_proj28 op;                                               // 0: the identity, 1: P, 2: [x^2] P, 3: both
#pragma unroll
    for (int i = 0; i < N28; i++) {
      op.x.l[i] = sel == 1 ? P0.x.l[i] : sel == 2 ? P1.x.l[i] : sel == 3 ? P01.x.l[i] : 0u;
      op.y.l[i] = sel == 1 ? P0.y.l[i] : sel == 2 ? P1.y.l[i] : sel == 3 ? P01.y.l[i] : one.l[i];
      op.z.l[i] = sel == 3 ? P01.z.l[i] : sel == 0 ? 0u : one.l[i];
    }
    g1_add28(acc, acc, op);
  }
  return acc;
}
#endif  // __HIPCC__

}  // namespace bp

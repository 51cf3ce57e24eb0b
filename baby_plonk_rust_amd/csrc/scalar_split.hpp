// scalar_split.hpp -- k = k1 x^2 + k0 for the BLS parameter x: the scalar decomposition behind the endomorphism form of the
// variable-base multiplication of verify_segments_kernels.hpp, as __host__ __device__ lines (the kernel and the CPU check of
// tests/test_scalar_split.py run the same ones, as with msm_digits.hpp).
//
// phi(x, y) = (beta x, y) acts on the prime-order subgroup as -[x^2] (g1.rs:394-411, g1_check.hpp), so [x^2] P = (beta x, -y) costs one
// field product and k P = k0 P + k1 [x^2] P needs only as many doublings as the longer half has bits.  x^2 is a 128-bit number
// and q = x^4 - x^2 + 1, so the plain quotient and remainder of k by x^2 are already balanced: for every k < 2^255 both are below
// 2^128 (k1 <= (2^255 - 1) / x^2 < 2^127.6, k0 < x^2 < 2^127.5).  No lattice, no rounding, no signs.
#pragma once
#include <stdint.h>

#include "bigint.hpp"

namespace bp {

// x^2 = 0xd201000000010000^2, little-endian 32-bit limbs
BP_HD constexpr uint32_t bls_x2_limb(int i) {
  constexpr uint32_t t[4] = {0x00000000u, 0x00000001u, 0x0001a402u, 0xac45a401u};
  return t[i];
}
constexpr int SCALAR_SPLIT_BITS = 128;                       // loop count of the joint double-and-add: both halves are < 2^128

// k (8 limbs, < 2^255) -> k0 = k mod x^2, k1 = k div x^2 (4 limbs each).  Restoring division, one quotient bit per step: the
// top 128 bits of k are below 2^127 < x^2, so they are the first partial remainder as they stand and 128 steps are left.  The
// partial remainder r < x^2 < 2^128 doubles to less than 2^129: the bit shifted out of the top limb is kept and decides, with the
// borrow of r - x^2, whether the subtraction is taken.  About 25 limb operations per step, against the ~10 000 instructions of one
// step of the multiplication this feeds.
BP_HD void scalar_split_x2(uint32_t k0[4], uint32_t k1[4], const uint32_t k[8]) {
  uint32_t r[4] = {k[4], k[5], k[6], k[7]}, q[4] = {0, 0, 0, 0};
#pragma unroll
  for (int w = 3; w >= 0; w--) {
    const uint32_t word = k[w];
    uint32_t qw = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int b = 31; b >= 0; b--) {
      const uint32_t out = r[3] >> 31;
      r[3] = (r[3] << 1) | (r[2] >> 31);
      r[2] = (r[2] << 1) | (r[1] >> 31);
      r[1] = (r[1] << 1) | (r[0] >> 31);
      r[0] = (r[0] << 1) | ((word >> b) & 1u);
      uint32_t t[4];
      uint64_t borrow = 0;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const uint64_t d = (uint64_t)r[i] - bls_x2_limb(i) - borrow;
        t[i] = (uint32_t)d;
        borrow = (d >> 32) & 1u;
      }
      const bool ge = out || !borrow;
#pragma unroll
      for (int i = 0; i < 4; i++) r[i] = ge ? t[i] : r[i];
      qw |= (ge ? 1u : 0u) << b;
    }
    q[w] = qw;
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    k0[i] = r[i];
    k1[i] = q[i];
  }
}

}  // namespace bp

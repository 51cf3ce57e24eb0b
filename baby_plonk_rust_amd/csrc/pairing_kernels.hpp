// pairing_kernels.hpp -- bp_pairing_check on the GPU: one pairing check per lane, one wave per workgroup.
//   pairing_decode : 2 n G1 records (A_0, B_0, A_1, ...) -> Montgomery affine points, B negated; canonical coordinates, flags, the
//                    curve and, where asked, the subgroup; a failing lane does one atomicMin of (pair << 2) | reason
//   pairing_miller : f = MillerLoop((A, x_2), (-B, G2)) from the two tables of prepared lines (pairing.hpp, pairing_miller2)
//   pairing_final  : f = f^e (pairing_final_exponentiation), the verdict f == 1 and, where asked, the 576-byte image of f
// Storage.  An Fp12 is 144 dwords and the final exponentiation keeps eight alive; a lane has 512 registers.  Every Fp12 lives in the
// lane's WORKSPACE in HBM (tower.hpp): PAIRING_SLOTS Fp2 slots of 24 dwords, laid out limb-major by lane -- dword k of slot s of
// lane i is ws[(24 s + k) * stride + i] -- so the 64 lanes of a wave read and write 64 consecutive dwords, one 256-byte line per
// instruction.  The arithmetic runs at Fp2 / Fp6 granularity in registers; the Fp12 routines are real functions that take slot
// numbers, so each exists once in the code object and none keeps an Fp12 on the stack.  Both kernels share the workspace: the
// Miller loop leaves f in variable 0.  The line tables (2 x 68 x 3 Fp2, 39 KB) are read at a wave-uniform index.
#pragma once
#include "g1_check.hpp"
#include "pairing.hpp"

namespace bp {

struct LaneWs {
  uint32_t* base;            // dword 0 of this lane
  size_t stride;             // lanes of the workspace
  BP_HD fp2_t ld(int slot) const {
    fp2_t v;
    const uint32_t* p = base + (size_t)(24 * slot) * stride;
#pragma unroll
    for (int k = 0; k < 12; k++) {
      v.c0.l[k] = p[(size_t)k * stride];
      v.c1.l[k] = p[(size_t)(12 + k) * stride];
    }
    return v;
  }
  BP_HD void st(int slot, const fp2_t& v) const {
    uint32_t* p = base + (size_t)(24 * slot) * stride;
#pragma unroll
    for (int k = 0; k < 12; k++) {
      p[(size_t)k * stride] = v.c0.l[k];
      p[(size_t)(12 + k) * stride] = v.c1.l[k];
    }
  }
};
// dwords of a workspace of `stride` lanes
inline size_t pairing_ws_dwords(size_t stride) { return (size_t)PAIRING_SLOTS * 24 * stride; }

// pairing_decode_g1_words (pairing.hpp: the decoder the host check runs) of record j of `recs` (2 n records of 96 bytes, 4-byte
// aligned); odd records (the B of a pair) are stored negated.  The identity is (0, 0), as in every device buffer.
__global__ void __launch_bounds__(64) pairing_decode(const uint8_t* __restrict__ recs, size_t n_points, uint32_t subgroup,
                                                      g1_affine* __restrict__ out, unsigned long long* __restrict__ status) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_points) return;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(recs + 96 * j);
  uint32_t w[24];
#pragma unroll
  for (int k = 0; k < 24; k++) w[k] = src[k];
  g1_affine p;
  const uint32_t bad = pairing_decode_g1_words(p, w, subgroup != 0);
  if (bad) atomicMin(status, ((unsigned long long)(j >> 1) << 2) | bad);
  if (j & 1) Fp::neg(p.y, p.y);                                    // (0, 0) stays (0, 0)
  out[j] = p;
}

// lanes [first, first + count) of the call; lane i of the kernel owns column i of the workspace
__global__ void __launch_bounds__(64) pairing_miller(const g1_affine* __restrict__ pts, size_t first, size_t count,
                                                      const fp2_t* __restrict__ lines_x2, const fp2_t* __restrict__ lines_gen,
                                                      uint32_t* __restrict__ ws, size_t stride) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const LaneWs w{ws + i, stride};
  const g1_affine a = pts[2 * (first + i)], nb = pts[2 * (first + i) + 1];
  pairing_miller2(w, tw_var(0), lines_x2, a, lines_gen, nb);
}

__global__ void __launch_bounds__(64) pairing_final(size_t first, size_t count, uint32_t* __restrict__ ws, size_t stride,
                                                     uint8_t* __restrict__ verdicts, uint32_t* __restrict__ gt_or_null) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const LaneWs w{ws + i, stride};
  const int f = tw_var(0);
  pairing_final_exponentiation(w, f, tw_var(1), tw_var(2), tw_var(3), tw_var(4), tw_var(5), tw_var(6), tw_var(7));
  verdicts[first + i] = fp12w_is_one(w, f) ? 1 : 0;
  if (gt_or_null) {
    uint32_t* dst = gt_or_null + (first + i) * 144;
#pragma unroll 1
    for (int k = 0; k < 6; k++) {
      const fp2_t v = w.ld(f + k);
#pragma unroll
      for (int l = 0; l < 12; l++) {
        dst[24 * k + l] = v.c0.l[l];
        dst[24 * k + 12 + l] = v.c1.l[l];
      }
    }
  }
}

}  // namespace bp

// verify_segments_kernels.hpp -- stage 4 of bp_verify_reduce_segments: the scalars and points of verify_kernels.hpp turned into one
// pair (A_s, B_s) per SEGMENT of the batch instead of one pair for all of it.  That is T = 11 m + 9 S independent products
// scalar x point followed by short sums -- the bucket MSM has nothing to offer a 20-term sum -- so the work is laid out one term
// per lane:
//   verify_seg_shared_sum : the nine shared-base scalars of every segment (a segmented Fr sum of verify_scalars' `shared`)
//   verify_seg_mul        : one variable-base multiplication per lane on the 28-bit limbs of fp28.hpp / g1_28.hpp
//   verify_seg_proof_sum  : A_j (2 terms) and B_j (9 terms) of every proof
//   verify_seg_tree       : one level of the segment sums: neighbours 2^l apart inside one segment are added, the rest stay
//   verify_seg_add_shared : B_s += the segment's nine shared-base products
//   verify_seg_encode     : affine form with one inversion per group of points, and the 96-byte encoding
//
// Projective points between the kernels are 42 words (x | y | z, 14 limbs each) stored word-major: word w of element i sits at
// w * count + i, so the lanes of a wave read and write neighbouring addresses.
//
// The multiplication.  g1_mul_split28 (g1_mul_split28.hpp: srs_scale runs it too) writes k = k1 x^2 + k0 (scalar_split.hpp) and
// runs ONE joint double-and-add over P, [x^2] P = (beta x, -y) and their sum: 128 steps of one doubling and one complete addition.
// g1_mul_plain28 is the
// 255-step double-and-add it is measured against (docs/EXPERIMENTS.md).  The split form is exact only where the endomorphism is
// [x^2], that is inside the prime-order subgroup: proof points are subgroup-checked in stage 3, the verifier key's are not, so the
// host tests those eight points once per call and sends the shared-base terms through the plain form if one of them fails.
// Neither form has a data-dependent branch: every step adds an operand picked limb by limb -- the identity (0 : 1 : 0) where the
// bits are clear -- with the complete formulas, and an input point that is the identity clears its scalar first.
#pragma once
#include "g1_28.hpp"
#include "g1_check.hpp"
#include "g1_mul_split28.hpp"
#include "scalar_split.hpp"
#include "verify_kernels.hpp"

namespace bp {

#if defined(__HIPCC__)
constexpr int SEG_PT_WORDS = 3 * N28;

__device__ __forceinline__ void seg_store_coord(uint32_t* __restrict__ base, size_t count, size_t i, int coord, const uint32_t* l) {
#pragma unroll
  for (int w = 0; w < N28; w++) base[(size_t)(coord * N28 + w) * count + i] = l[w];
}
__device__ __forceinline__ void seg_load_coord(uint32_t* l, const uint32_t* __restrict__ base, size_t count, size_t i, int coord) {
#pragma unroll
  for (int w = 0; w < N28; w++) l[w] = base[(size_t)(coord * N28 + w) * count + i];
}
__device__ __forceinline__ void seg_store_pt(uint32_t* __restrict__ base, size_t count, size_t i, const g1_proj28& p) {
  seg_store_coord(base, count, i, 0, p.x.l);
  seg_store_coord(base, count, i, 1, p.y.l);
  seg_store_coord(base, count, i, 2, p.z.l);
}
__device__ __forceinline__ g1_proj28 seg_load_pt(const uint32_t* __restrict__ base, size_t count, size_t i) {
  g1_proj28 p;
  seg_load_coord(p.x.l, base, count, i, 0);
  seg_load_coord(p.y.l, base, count, i, 1);
  seg_load_coord(p.z.l, base, count, i, 2);
  return p;
}

// the product of g1_mul_split28 by 255 doublings and selected mixed additions: any affine point of the curve, or the identity (0, 0)
__device__ __forceinline__ g1_proj28 g1_mul_plain28(const g1_affine& p, const fr_t& k) {
  const bool id = g1_affine_is_identity(p);
  const F28n x = fp_to_28(p.x);
  const PtY28 y = pt_y_signed(fp_to_28(p.y), false);
  uint32_t e[8];
#pragma unroll
  for (int i = 7; i > 0; i--) e[i] = (k.l[i] << 1) | (k.l[i - 1] >> 31);      // k < 2^255: bit 254 to the top
  e[0] = k.l[0] << 1;
  g1_proj28 acc = g1_identity28();
#pragma unroll 1
  for (int step = 0; step < 255; step++) {
    const bool take = (e[7] >> 31) != 0 && !id;
#pragma unroll
    for (int i = 7; i > 0; i--) e[i] = (e[i] << 1) | (e[i - 1] >> 31);
    e[0] <<= 1;
    g1_double28(acc, acc);
    g1_proj28 sum = acc;
    g1_add_mixed28(sum, x, y);
#pragma unroll
    for (int i = 0; i < N28; i++) {
      acc.x.l[i] = take ? sum.x.l[i] : acc.x.l[i];
      acc.y.l[i] = take ? sum.y.l[i] : acc.y.l[i];
      acc.z.l[i] = take ? sum.z.l[i] : acc.z.l[i];
    }
  }
  return acc;
}

// out[k S + s] = sum of shared[k m + j] over the proofs j of segment s.  A unit (k, s) is summed by L lanes (a power of two,
// <= 256, chosen by the host from the segment length): they stride over the segment, then a tree in LDS.  256 / L units per block.
__global__ void __launch_bounds__(256) verify_seg_shared_sum(const fr_t* __restrict__ shared, size_t m, size_t seg, size_t S, uint32_t L,
                                                              fr_t* __restrict__ out) {
  __shared__ uint32_t part[256 * 8];
  const uint32_t per = 256 / L, g = threadIdx.x / L, l = threadIdx.x % L;
  const size_t u = (size_t)blockIdx.x * per + g;
  const bool valid = u < (size_t)VERIFY_SHARED * S;
  fr_t acc = Fr::zero();
  if (valid) {
    const size_t k = u / S, s = u - k * S;
    const size_t begin = s * seg, end = begin + seg < m ? begin + seg : m;
    for (size_t j = begin + l; j < end; j += L) {
      fr_t v;
      (void)verify_load_fr(v, shared + k * m + j, BP_FR_MONT);
      Fr::add(acc, acc, v);
    }
  }
  for (uint32_t stride = L >> 1; stride > 0; stride >>= 1) {      // L is the same for the whole grid: every lane meets every barrier
#pragma unroll
    for (int i = 0; i < 8; i++) part[i * 256 + threadIdx.x] = acc.l[i];
    __syncthreads();
    if (l < stride) {
      fr_t v;
#pragma unroll
      for (int i = 0; i < 8; i++) v.l[i] = part[i * 256 + threadIdx.x + stride];
      Fr::add(acc, acc, v);
    }
    __syncthreads();
  }
  if (valid && l == 0) verify_store_fr(out + u, acc);
}

// Term t of [first, last) -> prod[t] (T = 11 m + 9 S elements).  t < 9 m: scal_b[t] x pts[t], the B terms, column-major;
// 9 m <= t < 11 m: scal_a[t - 9 m] x pts[t - 2 m], W_zeta and W_zeta_omega in A; then seg_scal[u] x pts[9 m + u / S], the
// shared bases of segment u % S.  Scalars are Montgomery.
template <bool SPLIT>
__global__ void __launch_bounds__(64) verify_seg_mul(const g1_affine* __restrict__ pts, const fr_t* __restrict__ scal_b, const fr_t* __restrict__ scal_a,
                                                      const fr_t* __restrict__ seg_scal, size_t m, size_t S, size_t first, size_t last,
                                                      uint32_t* __restrict__ prod) {
  const size_t t = first + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= last) return;
  const size_t nb = (size_t)VERIFY_POINTS * m, na = 2 * m, T = nb + na + (size_t)VERIFY_SHARED * S;
  size_t pi;
  const fr_t* sp;
  if (t < nb) {
    pi = t;
    sp = scal_b + t;
  } else if (t < nb + na) {
    pi = t - na;
    sp = scal_a + (t - nb);
  } else {
    const size_t u = t - nb - na;
    pi = nb + u / S;
    sp = seg_scal + u;
  }
  fr_t k;
  (void)verify_load_fr(k, sp, BP_FR_MONT);
  Fr::from_mont(k, k);
  const g1_affine p = pts[pi];
  const g1_proj28 r = SPLIT ? g1_mul_split28(p, k) : g1_mul_plain28(p, k);
  seg_store_pt(prod, T, t, r);
}

// node[j] = A_j = prod[9 m + j] + prod[10 m + j],  node[m + j] = B_j = sum_{k < 9} prod[k m + j]
__global__ void __launch_bounds__(64) verify_seg_proof_sum(const uint32_t* __restrict__ prod, size_t T, size_t m, uint32_t* __restrict__ node) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 2 * m) return;
  const bool is_b = e >= m;
  const size_t j = is_b ? e - m : e, first = is_b ? j : (size_t)VERIFY_POINTS * m + j;
  const int count = is_b ? VERIFY_POINTS : 2;
  g1_proj28 acc = seg_load_pt(prod, T, first);
#pragma unroll 1
  for (int i = 1; i < count; i++) {
    const g1_proj28 q = seg_load_pt(prod, T, first + (size_t)i * m);
    g1_add28(acc, acc, q);
  }
  seg_store_pt(node, 2 * m, e, acc);
}

// One level: inside every segment, the element at local index i (a multiple of 2 d) takes in the one at i + d, if the segment
// reaches that far.  After ceil(log2(seg)) levels the first element of a segment holds its sum.  slots = ceil(seg / 2 d).
__global__ void __launch_bounds__(64) verify_seg_tree(uint32_t* __restrict__ node, size_t m, size_t seg, size_t S, size_t d, size_t slots) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, half = S * slots;
  if (tid >= 2 * half) return;
  const size_t which = tid >= half ? 1 : 0, r = tid - which * half, s = r / slots, i = (r - s * slots) * 2 * d;
  const size_t begin = s * seg, end = begin + seg < m ? begin + seg : m, j = begin + i;
  if (j + d >= end) return;
  const size_t at = which * m + j;
  g1_proj28 a = seg_load_pt(node, 2 * m, at);
  const g1_proj28 b = seg_load_pt(node, 2 * m, at + d);
  g1_add28(a, a, b);
  seg_store_pt(node, 2 * m, at, a);
}

// B_s (at node[m + s seg]) += the nine shared-base products of segment s
__global__ void __launch_bounds__(64) verify_seg_add_shared(uint32_t* __restrict__ node, size_t m, size_t seg, size_t S, const uint32_t* __restrict__ prod,
                                                             size_t T) {
  const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const size_t at = m + s * seg;
  g1_proj28 acc = seg_load_pt(node, 2 * m, at);
#pragma unroll 1
  for (int k = 0; k < VERIFY_SHARED; k++) {
    const g1_proj28 q = seg_load_pt(prod, T, (size_t)(VERIFY_POINTS + 2) * m + (size_t)k * S + s);
    g1_add28(acc, acc, q);
  }
  seg_store_pt(node, 2 * m, at, acc);
}

// Point e of the 2 S results (A_s: e = 2 s at node[s seg], B_s: e = 2 s + 1 at node[m + s seg]) -> out[96 e ..], the encoding of
// G1Affine::to_uncompressed (the identity: 0x40 then zeros).  A lane normalises `group` points, `lanes` apart, with one shared
// inversion (Montgomery's trick as in srs_from_projective): the running products z'_0 .. z'_j wait in run[e] (14 words, word-major
// over 2 S), z' = z, or 1 where z = 0.
__global__ void __launch_bounds__(64) verify_seg_encode(const uint32_t* __restrict__ node, size_t m, size_t seg, size_t S, uint32_t group,
                                                         uint32_t* __restrict__ run, uint8_t* __restrict__ out) {
  const size_t n = 2 * S, lanes = (n + group - 1) / group;
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= lanes) return;
  auto where = [&](size_t e) { return (e & 1) * m + (e >> 1) * seg; };
  const C28 one = seg_one28();
  auto z_or_one = [&](C28& z) {                                  // -> was z zero?
    const bool zero = big_is_zero(fp_from_28(z));
#pragma unroll
    for (int i = 0; i < N28; i++) z.l[i] = zero ? one.l[i] : z.l[i];
    return zero;
  };
  M28 acc;
#pragma unroll
  for (int i = 0; i < N28; i++) acc.l[i] = One28::limb(i);
  uint32_t cnt = 0;
  for (size_t e = lane; e < n; e += lanes, cnt++) {
    C28 z;
    seg_load_coord(z.l, node, 2 * m, where(e), 2);
    (void)z_or_one(z);
    acc = mul28(acc, z);
    seg_store_coord(run, n, e, 0, acc.l);
  }
  M28 inv = fp28_invert(acc);
  for (uint32_t j = cnt; j-- > 0;) {
    const size_t e = lane + (size_t)j * lanes;
    g1_proj28 p = seg_load_pt(node, 2 * m, where(e));
    const bool inf = z_or_one(p.z);
    M28 zinv = inv;
    if (j) {
      M28 before;
      seg_load_coord(before.l, run, n, e - lanes, 0);
      zinv = mul28(inv, before);
    }
    inv = mul28(inv, p.z);
    fp_t x = fp_from_28(mul28(p.x, zinv)), y = fp_from_28(mul28(p.y, zinv));
    Fp::from_mont(x, x);
    Fp::from_mont(y, y);
    uint32_t w[24];
#pragma unroll
    for (int i = 0; i < 12; i++) {
      w[i] = inf ? 0u : __builtin_bswap32(x.l[11 - i]);
      w[12 + i] = inf ? 0u : __builtin_bswap32(y.l[11 - i]);
    }
    if (inf) w[0] = 0x40u;                                       // byte 0 of the record
    uint4* dst = reinterpret_cast<uint4*>(out + 96 * e);
#pragma unroll
    for (int i = 0; i < 6; i++) dst[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
  }
}
#endif  // __HIPCC__

}  // namespace bp
